"""What tests/test_fused_guard_gpu.py and tests/test_sa_options_gpu.py share: the descriptor-filling helpers of the fused eval-mode
kernels (layers folded and embedded behind guard words, the three output layouts, the SA inputs and the one SA launch), the two
assertions every result meets — err <= R * Y against float64 and the 1e-4 contract against the float32 oracle — and the table of
documented refusals. A plain module: no fixtures, no tests; tests/guard.py has the guard words, tests/fused_ref.py the cases."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from ptt_amd import ops
from tests import fused_ref as FR
from tests import guard
from tests.guard import check_guard, embed, guarded

F32, I32 = torch.float32, torch.int32

R_RATIO = 4.0               # twice the worst measured err / Y (1.98: the table in tests/test_fused_guard_gpu.py), one significant digit


class Ratios(dict):
    """case -> worst err / Y of its runs. Each test file keeps one of its own and reports it in its test_zz_ratio_report."""

    def note(self, case, err, Y):
        r = err / Y
        self[case] = max(self.get(case, 0.0), r)
        print("RATIO %-44s err %.3e  Y %.3e  err/Y %.2f" % (case, err, Y, r))
        return r

    def bound(self, case, got, ref64, ref32, Y):
        """(a) and (b) for one result (a host tensor)."""
        r = self.note(case, FR.rel_err(got, ref64), Y)
        assert r <= R_RATIO, "%s: %.2f x the float32 oracle's own distance from float64 (R = %g)" % (case, r, R_RATIO)
        np.testing.assert_allclose(got.numpy(), ref32.numpy(), **FR.TOL)

    def report(self):
        """Prints the table of the run (pytest -s) -> the worst ratio."""
        worst = max(self.values()) if self else 0.0
        for k in sorted(self):
            print("REPORT %-44s %.2f" % (k, self[k]))
        print("REPORT worst err/Y %.2f over %d results; R = %g" % (worst, len(self), R_RATIO))
        return worst


def put(t, dev, **kw):
    return embed(t.to(dev).contiguous(), **kw)


def bits(t):
    return t.contiguous().view(I32)


def same_bits(a, b, what):
    assert a.shape == b.shape and torch.equal(bits(a), bits(b)), "%s: not the same bits" % what


def untouched_inputs(ins):
    for v in ins:
        check_guard(v, all_written=False)


def fold(layers, dev, scale_in_weights):
    """oracle layer dicts -> (wpacked, scale | None, shift, cin, cout, relu) with no channel rotation (tests.util.fold_layers
    rotates the first layer it is given: right for a whole SA stack, wrong for the REMAINING layers of a split layer 0)."""
    out = []
    for L in layers:
        w = L["conv_weight"].to(dev)
        scale = L["bn_weight"] / torch.sqrt(L["bn_var"] + L["eps"])
        shift = (L["bn_bias"] - L["bn_mean"] * scale).to(dev).contiguous()
        if scale_in_weights:
            out.append((ops.pack_weight(w * scale.to(dev).view(-1, 1, 1, 1)), None, shift, w.shape[1], w.shape[0], True))
        else:
            out.append((ops.pack_weight(w), scale.to(dev).contiguous(), shift, w.shape[1], w.shape[0], True))
    return out


def embed_layers(layers, ins):
    """Every packed weight, scale and shift vector behind NaN words (1-D: lead and tail, 16-byte aligned)."""
    out = []
    for wp, sc, sh, cin, cout, relu in layers:
        e = [embed(t) if t is not None else None for t in (wp, sc, sh)]
        ins.extend(v for v in e if v is not None)
        out.append((e[0], e[1], e[2], cin, cout, relu))
    return out


def fill_layers(d, layers):
    d.n_layers = len(layers)
    for i, (wp, sc, sh, cin, co, relu) in enumerate(layers):
        L = d.layers[i]
        L.Wpacked = wp.data_ptr()
        L.scale = sc.data_ptr() if sc is not None else None
        L.shift = sh.data_ptr() if sh is not None else None
        L.Cin, L.Cout, L.relu = int(cin), int(co), int(bool(relu))


def out_view(dev, lay, B, rows, cout, planes=1, plane_gap=0):
    """A guarded output of a (B, cout, rows) result in layout A, B or C -> (the guarded tensor, (sb, sc, sm) element strides,
    fn: the guarded tensor -> the logical (planes * B, cout, rows) result). planes = 2 with plane_gap > 0: the two halves of the
    split xcorr form behind ONE guard, plane stride = B * sb + plane_gap."""
    if lay in ("A", "B"):
        ld = cout if lay == "A" else cout + 8
        bs = rows * ld + (0 if lay == "A" else 16)
        if planes == 1:
            v = guarded((B, rows, cout), F32, ld=ld, col_off=0 if lay == "A" else 4, batch_stride=bs, device=dev)
            return v, (bs, 1, ld), lambda t: t.transpose(1, 2)
        # the halves' batches are laid out back to back (bs = rows * ld), the halves `plane_gap` elements apart
        v = guarded((planes, B * rows, cout), F32, ld=ld, col_off=0 if lay == "A" else 4, batch_stride=B * rows * ld + plane_gap, device=dev)
        return v, (rows * ld, 1, ld), lambda t: t.reshape(planes * B, rows, cout).transpose(1, 2)
    ld = rows + 3
    if planes == 1:
        v = guarded((B, cout, rows), F32, ld=ld, device=dev)
        return v, (cout * ld, ld, 1), lambda t: t
    v = guarded((planes, B * cout, rows), F32, ld=ld, batch_stride=B * cout * ld + plane_gap, device=dev)
    return v, (cout * ld, ld, 1), lambda t: t.reshape(planes * B, cout, rows)


# ======================================================================================================= set abstraction
def sa_kernel_layers(layers, relu, dev, scale_in_weights, rot_first):
    """fused_ref layer dicts (any form of fused_ref.FORMS) -> the (wpacked, scale | None, shift | None, cin, cout, relu) tuples of
    ptt_sa_layer, formed as tests.util.fold_layers forms them: scale and shift in float32 on the host (fused_ref.layer_affine),
    scale_in_weights multiplies the scale into the weights on the device. rot_first: the rotation layer 0 is packed with."""
    out = []
    for li, (L, r) in enumerate(zip(layers, relu)):
        w = L["conv_weight"].to(dev)
        scale, shift = FR.layer_affine(L)
        shift = shift.to(dev).contiguous() if shift is not None else None
        if scale is not None and scale_in_weights:
            w, scale = w * scale.to(dev).view(-1, 1, 1, 1), None
        scale = scale.to(dev).contiguous() if scale is not None else None
        out.append((ops.pack_weight(w, rot_first if li == 0 else 0), scale, shift, w.shape[1], w.shape[0], bool(r)))
    return out


class SaInputs(object):
    """The device inputs of one SA case (fused_ref.sa_case / sa_option_case) in one feature layout, every one embedded."""

    def __init__(self, c, dev, feat_layout):
        self.c, self.ins = c, []
        e = lambda t, **kw: self._keep(put(t, dev, **kw))
        self.xyz, self.new_xyz = e(c.xyz), e(c.new_xyz)
        idx_dev = ops.ball_query(c.new_xyz.to(dev), c.xyz.to(dev), c.radius, c.ns)
        assert torch.equal(idx_dev.cpu(), c.idx), "the device index table is not the oracle's"
        self.idx = e(c.idx)
        self.feat, self.term, self.wx = None, None, None
        if c.hoist:
            # as tests/test_dense_gpu.py::test_sa_fused_hoisted_layer0: layer 0's feature half once per point on the linear kernel
            w0 = c.layers[0]["conv_weight"].reshape(c.spec[1], c.spec[0]).to(dev)
            scale0, shift0 = (t.to(dev).contiguous() if t is not None else None for t in FR.layer_affine(c.layers[0]))
            rows = c.feats.to(dev).transpose(1, 2).contiguous()
            term = ops.linear(rows, ops.pack_weight(w0[:, 3:].contiguous()), c.spec[1], scale0, shift0, relu=False)
            self.term = self._keep(embed(term.contiguous()))
            wx = w0[:, 0:3] * scale0[:, None] if scale0 is not None else w0[:, 0:3]
            self.wx = self._keep(embed(wx.t().contiguous()))
            layers = sa_kernel_layers(c.layers[1:], c.relu[1:], dev, c.scale_in_weights, 0)
        else:
            # the kernel's rows are [features | xyz]: layer 0 is packed with rot = 3 when both are there, rot = 0 otherwise
            layers = sa_kernel_layers(c.layers, c.relu, dev, c.scale_in_weights, 3 if (c.use_xyz and c.C > 0) else 0)
            if c.feats is not None:
                if feat_layout == "point":          # (B,N,C) storage, rows 16-byte aligned: vec_gather where C % 4 == 0
                    v = e(c.feats.transpose(1, 2), ld=c.C + 4, col_off=4, batch_stride=c.N * (c.C + 4) + 8)
                    self.feat, self.fstr = v, (v.stride(0), 1, v.stride(1))
                else:                               # (B,C,N) storage with ld = N + 1: the scalar gather
                    v = e(c.feats, ld=c.N + 1)
                    self.feat, self.fstr = v, (v.stride(0), v.stride(1), 1)
        self.layers = embed_layers(layers, self.ins)

    def _keep(self, v):
        self.ins.append(v)
        return v


def sa_desc(s, out, strides):
    """The ptt_sa_desc of a case's inputs `s` and a guarded output: every flag from the case."""
    c = s.c
    d = ops.SaDesc()
    d.xyz, d.new_xyz, d.idx = s.xyz.data_ptr(), s.new_xyz.data_ptr(), s.idx.data_ptr()
    if s.feat is not None:
        d.feat, d.C = s.feat.data_ptr(), c.C
        d.feat_sb, d.feat_sc, d.feat_sn = s.fstr
    d.out, (d.out_sb, d.out_sc, d.out_sm) = out.data_ptr(), strides
    d.B, d.N, d.M, d.nsample = c.B, c.N, c.M, c.ns
    d.radius, d.use_xyz, d.normalize_xyz = float(c.radius), int(c.use_xyz), int(c.normalize_xyz)
    fill_layers(d, s.layers)
    if c.hoist:
        d.l0_point_term, d.l0_xyz_weight, d.l0_channels, d.l0_relu = s.term.data_ptr(), s.wx.data_ptr(), c.spec[1], int(c.relu[0])
    return d


def sa_run(dev, s, lay, compact=False):
    """One launch -> the (B, Cout, M) result on the host; (c) is checked here."""
    c = s.c
    out, strides, logical = out_view(dev, lay, c.B, c.M, c.spec[-1])
    d = sa_desc(s, out, strides)
    ws = None
    if compact:
        n = int(ops._host("ptt_sa_compact_workspace", c.B, c.M))
        ws = guard.workspace(n, device=dev)
        d.compact_ws, d.compact_ws_bytes = ws.data_ptr(), n
    guard.launch("ptt_sa_fused_fwd_f32", dev, ctypes.byref(d))
    torch.cuda.synchronize()
    check_guard(out)
    if ws is not None:
        check_guard(ws, all_written=False)
    untouched_inputs(s.ins)
    return logical(out).cpu().contiguous()


def run_sa_case(dev, c, label, ratios):
    """(a) - (f) for one SA case (fused_ref.sa_case / sa_option_case): every feature layout x output layouts A, B, C."""
    feat_layouts = ["point", "channel"] if (c.feats is not None and not c.hoist) else ["none"]
    first = None
    for fl in feat_layouts:
        s = SaInputs(c, dev, fl)
        for lay in "ABC":
            got = sa_run(dev, s, lay)
            ratios.bound("%s feat=%s out=%s" % (label, fl, lay), got, c.ref64, c.ref32, c.Y)          # (a), (b); (c) in sa_run
            if first is None:
                first = got
                same_bits(sa_run(dev, s, lay), first, "%s: second run" % label)                     # (e)
            same_bits(got, first, "%s: feature layout %s, output layout %s against the first run" % (label, fl, lay))   # (d)
            if c.compact:
                same_bits(sa_run(dev, s, lay, compact=True), first, "%s: compact run, layout %s" % (label, lay))     # (f)


def _header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "ptt_hip.h")) as fh:
        return " ".join(re.sub(r"^\s*\*", " ", fh.read(), flags=re.M).split())


# refusal -> (status, the words of include/ptt_hip.h it follows from)
REFUSALS = {
    "pair_odd_N":        ("PTT_EUNSUPPORTED", "N must be even (a tile holds two points of one cloud; PTT_EUNSUPPORTED otherwise)"),
    "xcorr_Nt_65":       ("PTT_EUNSUPPORTED", "(Nt % 64 == 0, PTT_EUNSUPPORTED otherwise)"),
    "sa_nsample_8":      ("PTT_EUNSUPPORTED", "nsample 16, 32 or 64 (PTT_EUNSUPPORTED otherwise)"),
    "sa_Cout_48":        ("PTT_EUNSUPPORTED", "multiple of 32, <= 256 (PTT_EUNSUPPORTED otherwise)"),
    "xcorr_split_BNs":   ("PTT_EINVAL", "B * Ns % 8 == 0; sim_out NULL (PTT_EINVAL otherwise)"),
    "compact_ws_short":  ("PTT_EWORKSPACE", "workspace of at least ptt_sa_compact_workspace(B, M) bytes, 16-byte aligned (PTT_EWORKSPACE otherwise)"),
    "compact_ws_align":  ("PTT_EWORKSPACE", "workspace of at least ptt_sa_compact_workspace(B, M) bytes, 16-byte aligned (PTT_EWORKSPACE otherwise)"),
    "sa_noxyz_C0":       ("PTT_EINVAL", "with C == 0 it must be 1: a level needs the coordinates or point features (PTT_EINVAL otherwise)"),
    "sa_noxyz_hoist":    ("PTT_EINVAL", "When l0_point_term != NULL: use_xyz must be 1 (PTT_EINVAL otherwise)"),
}


def refused(what, fn, *outputs):
    status, words = REFUSALS[what]
    assert words in _header(), "%s: include/ptt_hip.h does not document this refusal" % what
    with pytest.raises(RuntimeError, match=status):
        fn()
    torch.cuda.synchronize()
    guard.assert_untouched(*outputs)
