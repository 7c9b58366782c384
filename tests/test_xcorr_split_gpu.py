"""ptt_xcorr_split_f32, ops.xcorr_split and CosineSimAug.precision = 'bf16x2' on the GPU, against the split arithmetic in float64
(tests/xcorr_split_ref.py), behind guard bands (tests/guard.py) — launched as tests/test_sa_split_gpu.py launches its kernel:
outputs from out_view(...), every input embed(...)-ded, check_guard / untouched_inputs after every launch.

  (a) generic cases (1,1,64) / (3,5,192) / (2,3,128): max|got - split64| / max|split64| <= R * Y, Y = max(e32, 4u) from the
      float32 run of the same emulation, R = R_RATIO = 4 (cap 8); output layouts A, B (point-major) and C (channel-major), which
      agree bit for bit; relu2 on and off, shifts given and NULL, and a changed flag changes a bit. (An fp32 kernel sits within a
      few Y of split64 on these cases too: (a) cannot tell it apart, (b) does.)
  (b) the split is really there: on the planted cases max|got - split64| <= 0.3 * max|split64 - exact64| — between the
      reference's own 0.15 and the 0.9 of an fp32 kernel, both pinned by tests/test_xcorr_split_cpu.py.
  (c) a second run gives the same bits; a refused descriptor (NULL W2s, a misaligned P, Nt = 96) leaves the guarded output
      untouched; empty launches write nothing.
  (d) ops.xcorr_split equals the raw launch bit for bit.
  (e) module at B = 3, f = 20, n1 = 64, n2 = 192, MLP.CHANNELS [24, 256, 256, 256]: 'bf16x2' equals ops.xcorr_split on the
      module's own packs (trailing convolutions applied to both) bit for bit, differs from fp32, notes nothing, lies within
      fused_ref.TOL of the float64 oracle; back in 'fp32' the bits of a module whose attribute was never set and no split pack;
      at B = 1, n2 = 128 (the one-frame form) 'bf16x2' gives the fp32 bits, one fallback entry, one warning.
  (f) graphs: a GraphedHotPath of the full KITTI tracker at B = 8 in fp32, after set_precision(..., scope=('similarity',)), and
      back.

Measured on an MI355X, err / Y (the output layouts agree bit for bit; relu2 = 0 gives the err / Y of relu2 = 1):
  case        shifts given   shifts NULL      Y (given / NULL)
  (1,1,64)    1.15           0.89             1.05e-6 / 1.20e-6
  (3,5,192)   1.03           1.46             2.31e-6 / 1.81e-6
  (2,3,128)   1.55           0.94             1.58e-6 / 2.30e-6
  planted     (1,1,64) 1.86, (3,5,192) 2.12   (Y = 4u = 2.4e-7)
Worst err / Y 2.12 (planted (3,5,192)) over 33 results: no case came near the bar of 4, R stays 4. (b)'s ratio max|got - split64| /
max|split64 - exact64|: planted (1,1,64) 0.118, planted (3,5,192) 0.130 (bar 0.3; the float32 emulation 0.079 / 0.114, an fp32
evaluation 1.06 / 1.10). Module at (3, 20, 64, 192): 'bf16x2' at 0.41 of TOL from the float64 oracle, 'fp32' at 0.030.
"""
import ctypes
import warnings

import numpy as np
import pytest
import torch

from oracle import dense_ref as R
from ptt_amd import ops, synth
from ptt_amd.hot_path import AttrDict
from ptt_amd.models.backbones_3d.pointnet2 import pytorch_utils as layer_utils
from ptt_amd.models.similarity_modules.p2b_xcoor import CosineSimAug
from ptt_amd.precision import set_precision
from tests import fused_ref as FR
from tests import guard
from tests import xcorr_split_ref as XS
from tests.fused_launch import I32, R_RATIO, Ratios, out_view, put, same_bits, untouched_inputs
from tests.guard import check_guard, embed
from tests.util import cosine_sim_params, load_cosine_sim, mlp_layers

pytestmark = pytest.mark.gpu
SPLIT_SHARE = 0.3
RATIOS = Ratios()


def test_r_is_within_its_cap():
    assert R_RATIO <= 8


class Inputs(object):
    """The device operands of one parameter set (xcorr_split_ref.inputs / planted_case(...).p), every one embedded."""

    def __init__(self, p, dev):
        self.p, self.ins = p, []
        keep = lambda v: (self.ins.append(v), v)[1]
        self.cos, self.P, self.w_sim = keep(put(p.cos, dev)), keep(put(p.P, dev)), keep(put(p.w_sim, dev))
        self.W1s = keep(embed(ops.pack_weight_split(p.W1.to(dev)).view(I32)))
        self.W2s = keep(embed(ops.pack_weight_split(p.W2.to(dev)).view(I32)))
        self.sh1, self.sh2 = keep(put(p.sh1, dev)), keep(put(p.sh2, dev))

    def desc(self, out, strides, relu2=True, shifts=True):
        p, d = self.p, ops.XcorrSplitDesc()
        d.cos_t, d.P, d.w_sim = self.cos.data_ptr(), self.P.data_ptr(), self.w_sim.data_ptr()
        d.W1s, d.W2s, d.relu2 = self.W1s.data_ptr(), self.W2s.data_ptr(), int(relu2)
        d.shift1 = self.sh1.data_ptr() if shifts else None
        d.shift2 = self.sh2.data_ptr() if shifts else None
        d.out, (d.out_sb, d.out_sc, d.out_sn) = out.data_ptr(), strides
        d.B, d.Ns, d.Nt = p.B, p.Ns, p.Nt
        return d

    def run(self, dev, lay, relu2=True, shifts=True):
        p = self.p
        out, strides, logical = out_view(dev, lay, p.B, p.Ns, 256)
        d = self.desc(out, strides, relu2, shifts)
        guard.launch("ptt_xcorr_split_f32", dev, ctypes.byref(d))
        torch.cuda.synchronize()
        check_guard(out)
        untouched_inputs(self.ins)
        return logical(out).cpu().contiguous()


def bound(case, got, ref64, Y):
    r = RATIOS.note(case, FR.rel_err(got, ref64), Y)
    assert r <= R_RATIO, "%s: %.2f x the float32 emulation's own distance from float64 (R = %g)" % (case, r, R_RATIO)


FLAGS = [dict(), dict(relu2=False), dict(shifts=False), dict(relu2=False, shifts=False)]


# ================================================================================================================ kernel
@pytest.mark.parametrize("shape", XS.GENERIC)
def test_generic(dev, shape):
    s = Inputs(XS.inputs(*shape), dev)
    first = None
    for flags in FLAGS:
        g = XS.generic_case(*shape, **flags)
        tag = "%s %s" % (g.p.name, ",".join("%s=0" % k for k in flags) or "all on")
        for lay in ("ABC" if not flags else "AC"):
            got = s.run(dev, lay, **flags)
            bound("%s out=%s" % (tag, lay), got, g.split64, g.Y)                                        # (a)
            if not flags:
                if first is None:
                    first = got
                    same_bits(s.run(dev, lay), first, "%s: second run" % tag)                         # (c)
                same_bits(got, first, "%s: output layout %s against the first run" % (tag, lay))
            elif lay == "A":
                flagged = got
            else:
                same_bits(got, flagged, "%s: output layout C against A" % tag)
        if flags:
            assert not torch.equal(got, first), "%s: the flag changed no bit" % tag


@pytest.mark.parametrize("shape", XS.PLANTED)
def test_the_split_is_there(dev, shape):
    c = XS.planted_case(*shape)
    s = Inputs(c.p, dev)
    own = float((c.split64 - c.exact64).abs().max())
    key = "%s share" % c.p.name
    for lay in "AC":
        got = s.run(dev, lay)
        d = float((got.double() - c.split64).abs().max())
        print("SPLIT %-20s out=%s |got - split64| %.3e  |split64 - exact64| %.3e  ratio %.3f" % (c.p.name, lay, d, own, d / own))
        RATIOS[key] = max(RATIOS.get(key, 0.0), d / own)
        assert d <= SPLIT_SHARE * own, "%s: %.3e from the split arithmetic, which itself lies %.3e from exact" % (c.p.name, d, own)   # (b)
        bound("%s out=%s" % (c.p.name, lay), got, c.split64, c.Y)


@pytest.mark.parametrize("what,status", [("null_W2s", "PTT_EINVAL"), ("misaligned_P", "PTT_EINVAL"), ("Nt_96", "PTT_EUNSUPPORTED")])
def test_refusals_write_nothing(dev, what, status):
    p = XS.inputs(3, 5, 192)
    s = Inputs(p, dev)
    out, strides, _ = out_view(dev, "A", p.B, p.Ns, 256)
    d = s.desc(out, strides)
    if what == "null_W2s":
        d.W2s = None
    elif what == "misaligned_P":
        d.P = s.P.data_ptr() + 4
    else:
        d.Nt = 96
    with pytest.raises(RuntimeError, match=status):
        guard.launch("ptt_xcorr_split_f32", dev, ctypes.byref(d))
    torch.cuda.synchronize()
    guard.assert_untouched(out)
    untouched_inputs(s.ins)


def test_empty_launches_write_nothing(dev):
    p = XS.inputs(3, 5, 192)
    s = Inputs(p, dev)
    out, strides, _ = out_view(dev, "A", p.B, p.Ns, 256)
    for B, Ns in ((0, p.Ns), (p.B, 0)):
        d = s.desc(out, strides)
        d.B, d.Ns = B, Ns
        guard.launch("ptt_xcorr_split_f32", dev, ctypes.byref(d))
    torch.cuda.synchronize()
    guard.assert_untouched(out)


def test_ops_wrapper_equals_the_raw_launch(dev):
    p = XS.inputs(3, 5, 192)
    s = Inputs(p, dev)
    raw = s.run(dev, "A")
    w1s, w2s = ops.pack_weight_split(p.W1.to(dev)), ops.pack_weight_split(p.W2.to(dev))
    got = ops.xcorr_split(s.cos, s.P, s.w_sim, w1s, s.sh1, w2s, s.sh2)
    assert got.shape == (p.B, 256, p.Ns) and got.stride(1) == 1                   # point-major storage
    same_bits(got.cpu(), raw, "ops.xcorr_split against the raw launch")
    out = torch.empty((p.B, 256, p.Ns), dtype=torch.float32, device=dev)
    assert ops.xcorr_split(s.cos, s.P, s.w_sim, w1s, s.sh1, w2s, s.sh2, out=out) is out
    same_bits(out.cpu(), raw, "channel-major output")
    same_bits(ops.xcorr_split(s.cos, s.P, s.w_sim, w1s, None, w2s, None, relu2=False).cpu(), s.run(dev, "A", relu2=False, shifts=False),
              "no shifts, no ReLU")
    for bad in ((w1s[:-2], w2s), (w1s, w2s.float()), (w1s, None)):
        with pytest.raises(ValueError):
            ops.xcorr_split(s.cos, s.P, s.w_sim, bad[0], s.sh1, bad[1], s.sh2)
    with pytest.raises(ValueError):
        ops.xcorr_split(s.cos, s.P, s.w_sim, w1s, s.sh1[:128].contiguous(), w2s, s.sh2)


# ================================================================================================================ module
MODULE_F, MODULE_SEED = 20, 31


def _module(dev, mlp, conv, precision=None):
    m = CosineSimAug(AttrDict.wrap(dict(DEBUG=False, MLP=dict(CHANNELS=[4 + MODULE_F, 256, 256, 256], BN=True),
                                        CONV=dict(CHANNELS=[256, 256, 256], BN=True)))).eval()
    load_cosine_sim(m, mlp, conv)
    if precision is not None:
        m.precision = precision
    return m.to(dev)


def _module_inputs(B, n1, n2):
    rs = np.random.RandomState(n1 + n2 + B)
    sf = torch.from_numpy(rs.standard_normal((B, MODULE_F, n2)).astype(np.float32))
    tf = torch.from_numpy(rs.standard_normal((B, MODULE_F, n1)).astype(np.float32))
    txyz = torch.from_numpy(rs.uniform(-2, 2, (B, n1, 3)).astype(np.float32))
    return sf, tf, txyz


def test_module(dev):
    mlp, conv = mlp_layers(MODULE_SEED, [4 + MODULE_F, 256, 256, 256]), cosine_sim_params(MODULE_SEED)[1]
    B, n1, n2 = 3, 64, 192
    assert B * n2 > ops.ONE_FRAME_MAX_POINTS                                       # the batched branch, just
    sf, tf, txyz = _module_inputs(B, n1, n2)
    ref64 = R.cosine_sim_aug(sf.double(), tf.double(), txyz.double(), FR.double_layers(mlp),
                             {k: v.double() for k, v in conv.items()})[0]
    batch = lambda: {'search_feats': sf.to(dev), 'template_feats': tf.to(dev), 'template_seeds': txyz.to(dev)}
    split, never = _module(dev, mlp, conv, 'bf16x2'), _module(dev, mlp, conv)
    ops.unfused_calls.clear()
    ops.precision_fallbacks.clear()
    with torch.no_grad():
        y = split(batch())['cosine_feats']
        y0 = never(batch())['cosine_feats']
        # the direct call on the module's own folded packs, as forward chains it
        P, S, b = split._params(), split._split_params(), batch()
        rows = torch.cat((b['template_seeds'], b['template_feats'].transpose(1, 2)), dim=2)
        pre = ops.linear(rows, P['w_rest'], P['c0'], P['scale0'], P['shift0'])
        cos_t = ops.cosine_map(b['search_feats'], b['template_feats'], eps=split.cosine.eps)
        fused = ops.xcorr_split(cos_t, pre, P['w_sim'], S['w1s'], S['shift1'], S['w2s'], S['shift2'], relu2=S['relu2'])
        direct = layer_utils.rows_forward(split.conv, fused.transpose(1, 2)).transpose(1, 2)
    torch.cuda.synchronize()
    assert not ops.unfused_calls and not ops.precision_fallbacks, (ops.unfused_calls, ops.precision_fallbacks)
    same_bits(y.cpu(), direct.cpu(), "'bf16x2' module against ops.xcorr_split on its own packs")
    assert not torch.equal(y, y0), "'bf16x2' gave the fp32 bits: the split kernel did not run"
    share = lambda t: float(((t.cpu().double() - ref64).abs() / (FR.TOL["atol"] + FR.TOL["rtol"] * ref64.abs())).max())
    print("MODULE (3,20,64,192): 'bf16x2' at %.2f of TOL from ref64, 'fp32' at %.3f" % (share(y), share(y0)))
    np.testing.assert_allclose(y0.cpu().numpy(), ref64.numpy(), **FR.TOL)
    np.testing.assert_allclose(y.cpu().numpy(), ref64.numpy(), **FR.TOL)
    with torch.no_grad():
        split.precision = 'fp32'
        y1 = split(batch())['cosine_feats']
    same_bits(y1.cpu(), y0.cpu(), "'fp32' after 'bf16x2' against a module whose attribute was never set")
    assert not split._split_cache.held() and not never._split_cache.held()      # fp32 mode packs nothing new


def test_module_one_frame_form_stays_fp32_and_says_so_once(dev):
    mlp, conv = mlp_layers(MODULE_SEED, [4 + MODULE_F, 256, 256, 256]), cosine_sim_params(MODULE_SEED)[1]
    sf, tf, txyz = _module_inputs(1, 64, 128)
    batch = lambda: {'search_feats': sf.to(dev), 'template_feats': tf.to(dev), 'template_seeds': txyz.to(dev)}
    split, plain = _module(dev, mlp, conv, 'bf16x2'), _module(dev, mlp, conv)
    ops.precision_fallbacks.clear()
    with torch.no_grad(), warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        y = split(batch())['cosine_feats']
        y0 = plain(batch())['cosine_feats']
    same_bits(y.cpu(), y0.cpu(), "a 'bf16x2' module on the one-frame form against fp32")
    assert list(ops.precision_fallbacks.values()) == [1], ops.precision_fallbacks
    assert "one-frame" in list(ops.precision_fallbacks)[0][1]
    assert len([w for w in seen if "bf16x2" in str(w.message)]) == 1
    assert not split._split_cache.held()
    ops.precision_fallbacks.clear()


# ================================================================================================================ graphs
def test_graph_is_captured_again_when_the_similarity_precision_changes(dev):
    from ptt_amd.config import StubDataset, ptt_model_cfg
    from ptt_amd.hot_path import GraphedHotPath, TrackerThroughput, randomize_
    from ptt_amd.models import build_network
    keys = ("cosine_feats", "pred_centroids_cls", "pred_centroids_votes", "votes_feats")
    B = 8
    s, t = (torch.from_numpy(a).to(dev) for a in synth.frames(77, B, 1024, 512))
    make = lambda: randomize_(build_network(ptt_model_cfg(), 1, StubDataset()), seed=11).to(dev).eval()
    tracker = make()
    grab = lambda out: {k: out[k].clone() for k in keys}
    scope = ('similarity',)
    ops.precision_fallbacks.clear()
    g = GraphedHotPath(TrackerThroughput(tracker), s, t)
    first = grab(g(s, t))
    assert g.captures == 1
    assert set_precision(tracker, 'bf16x2', scope=scope) == 1
    second = grab(g(s, t))
    assert g.captures == 2
    fresh_tracker = make()
    set_precision(fresh_tracker, 'bf16x2', scope=scope)
    fresh = grab(GraphedHotPath(TrackerThroughput(fresh_tracker), s, t)(s, t))
    set_precision(tracker, 'fp32', scope=scope)
    third = grab(g(s, t))
    assert g.captures == 3
    torch.cuda.synchronize()
    assert not ops.precision_fallbacks, ops.precision_fallbacks           # B * n2 = 1024: the split kernel is dispatched
    for k in keys:
        assert torch.equal(second[k], fresh[k]), "%s: replay after set_precision differs from a runner built in 'bf16x2'" % k
        assert torch.equal(third[k], first[k]), "%s: back in 'fp32' the first result does not come back" % k
    assert not torch.equal(second["cosine_feats"], first["cosine_feats"]), "'bf16x2' replayed the fp32 xcorr arithmetic"


def test_zz_ratio_report():
    RATIOS.report()
