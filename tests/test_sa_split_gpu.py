"""ptt_sa_stream_split_f32, ops.sa_stream_split and PointnetSAModuleVotes.precision = 'bf16x2' on the GPU, against the split
arithmetic in float64 (tests/sa_split_ref.py), behind guard bands (tests/guard.py) — launched as tests/fused_launch.run_sa_case
launches the fp32 kernel: outputs guarded(...), every input embed(...)-ded, check_guard / untouched_inputs afterwards.

  (a) generic cases stream_33 / stream_1027 / stream_1029: max|got - split64| / max|split64| <= R * Y, Y = max(e32, 4u) from the
      float32 run of the same emulation, R = R_RATIO = 4 (cap 8); output layouts A, B (point-major) and C (channel-major);
      normalize_xyz, l0_relu and relu2 each on and off. (The float32 run of the emulation sits at 0.45 - 0.75 of the split's own
      distance from exact on these cases — the chained splits amplify float32 rounding — so a share test like the pair kernel's
      cannot be applied to them; the planted cases carry it.)
  (b) the split is really there: on the planted cases max|got - split64| <= 0.3 * max|split64 - exact64| — between the
      reference's own 0.15 and the 0.9 of an fp32 kernel, both pinned by tests/test_sa_split_cpu.py.
  (c) a second run gives the same bits; a refused descriptor (NULL W2s, a misaligned term) leaves the guarded output untouched.
  (d) module: mlp [128, 128, 128, 256], 32 neighbours on stream_1027's inputs and centres: 'bf16x2' equals the direct
      ops.sa_stream_split call on the module's own folded packs bit for bit and differs from fp32; back in 'fp32' the bits of a
      module whose attribute was never set; an SA0 module (no features) under 'bf16x2' gives its fp32 bits and one fallback.
  (e) graphs: a GraphedHotPath at B = 8 in fp32, after set_precision(..., scope=('transformer', 'sa')), and back.

Measured on an MI355X, err / Y (worst over the output layouts; the layouts agree bit for bit):
  case          all on   normalize_xyz=0   l0_relu=0   relu2=0
  stream_33     0.92     0.92              0.86        0.92
  stream_1027   1.21     1.21              1.23        1.21
  stream_1029   0.94     0.94              1.23        0.94
  planted       stream_33 1.18, stream_1027 1.39
Worst err / Y 1.39 (planted stream_1027): no case came near the bar of 4, R stays 4. (b)'s ratio max|got - split64| /
max|split64 - exact64|: planted stream_33 0.089, planted stream_1027 0.146 (bar 0.3; the float32 emulation 0.075 / 0.105).
Module on stream_1027: 'bf16x2' at 0.67 of TOL from ref64, 'fp32' at 0.030 (printed, not asserted).
"""
import ctypes
import warnings

import numpy as np
import pytest
import torch

from oracle import index_ops as O
from ptt_amd import ops, synth
from ptt_amd.models.backbones_3d.pointnet2.pointnet2_modules import PointnetSAModuleVotes
from ptt_amd.precision import set_precision
from tests import fused_ref as FR
from tests import guard
from tests import sa_split_ref as SS
from tests.fused_launch import F32, I32, R_RATIO, Ratios, out_view, put, same_bits, untouched_inputs
from tests.guard import check_guard, embed

pytestmark = pytest.mark.gpu
SPLIT_SHARE = 0.3
RATIOS = Ratios()


def test_r_is_within_its_cap():
    assert R_RATIO <= 8


class Inputs(object):
    """The device operands of one parameter set (sa_split_ref.inputs / planted_case(...).p), every one embedded."""

    def __init__(self, p, dev):
        self.p, self.ins = p, []
        keep = lambda v: (self.ins.append(v), v)[1]
        self.xyz, self.new_xyz, self.idx = keep(put(p.xyz, dev)), keep(put(p.new_xyz, dev)), keep(put(p.idx, dev))
        if p.get("term") is not None:
            term = p.term.to(dev)
        else:       # as the module forms it: layer 0's feature half once per point on the linear kernel, scale folded, shift added
            term = ops.linear(p.feats.to(dev).transpose(1, 2).contiguous(), ops.pack_weight(p.wf.to(dev)), 128, None, p.sh0.to(dev), relu=False)
        self.term, self.wx = keep(embed(term.contiguous())), keep(put(p.wx, dev))
        self.W1s = keep(embed(ops.pack_weight_split(p.W1.to(dev)).view(I32)))
        self.W2s = keep(embed(ops.pack_weight_split(p.W2.to(dev)).view(I32)))
        self.sh1, self.sh2 = keep(put(p.sh1, dev)), keep(put(p.sh2, dev))

    def desc(self, out, strides, normalize_xyz, l0_relu, relu2):
        p, d = self.p, ops.SaSplitDesc()
        d.xyz, d.new_xyz, d.idx = self.xyz.data_ptr(), self.new_xyz.data_ptr(), self.idx.data_ptr()
        d.l0_point_term, d.l0_xyz_weight, d.l0_relu = self.term.data_ptr(), self.wx.data_ptr(), int(l0_relu)
        d.W1s, d.shift1, d.W2s, d.shift2, d.relu2 = self.W1s.data_ptr(), self.sh1.data_ptr(), self.W2s.data_ptr(), self.sh2.data_ptr(), int(relu2)
        d.out, (d.out_sb, d.out_sc, d.out_sm) = out.data_ptr(), strides
        d.B, d.N, d.M, d.radius, d.normalize_xyz = p.B, p.N, p.M, float(p.radius), int(normalize_xyz)
        return d

    def run(self, dev, lay, normalize_xyz=True, l0_relu=True, relu2=True):
        p = self.p
        out, strides, logical = out_view(dev, lay, p.B, p.M, 256)
        d = self.desc(out, strides, normalize_xyz, l0_relu, relu2)
        guard.launch("ptt_sa_stream_split_f32", dev, ctypes.byref(d))
        torch.cuda.synchronize()
        check_guard(out)
        untouched_inputs(self.ins)
        return logical(out).cpu().contiguous()


def bound(case, got, ref64, Y):
    r = RATIOS.note(case, FR.rel_err(got, ref64), Y)
    assert r <= R_RATIO, "%s: %.2f x the float32 emulation's own distance from float64 (R = %g)" % (case, r, R_RATIO)


FLAGS = [dict(), dict(normalize_xyz=False), dict(l0_relu=False), dict(relu2=False)]


# ================================================================================================================ kernel
@pytest.mark.parametrize("name", SS.GENERIC)
def test_generic(dev, name):
    s = Inputs(SS.inputs(name), dev)
    first = None
    for flags in FLAGS:
        g = SS.generic_case(name, **flags)
        tag = "%s %s" % (name, ",".join("%s=0" % k for k in flags) or "all on")
        for lay in ("ABC" if not flags else "AC"):
            got = s.run(dev, lay, **flags)
            bound("%s out=%s" % (tag, lay), got, g.split64, g.Y)                                        # (a)
            if not flags:
                if first is None:
                    first = got
                    same_bits(s.run(dev, lay), first, "%s: second run" % tag)                         # (c)
                same_bits(got, first, "%s: output layout %s against the first run" % (tag, lay))
        if flags:
            assert not torch.equal(got, first), "%s: the flag changed no bit" % tag


@pytest.mark.parametrize("name", SS.PLANTED)
def test_the_split_is_there(dev, name):
    c = SS.planted_case(name)
    s = Inputs(c.p, dev)
    own = float((c.split64 - c.exact64).abs().max())
    for lay in "AC":
        got = s.run(dev, lay)
        d = float((got.double() - c.split64).abs().max())
        print("SPLIT planted %-12s out=%s |got - split64| %.3e  |split64 - exact64| %.3e  ratio %.3f" % (name, lay, d, own, d / own))
        RATIOS["planted %s share" % name] = max(RATIOS.get("planted %s share" % name, 0.0), d / own)
        assert d <= SPLIT_SHARE * own, "%s: %.3e from the split arithmetic, which itself lies %.3e from exact" % (name, d, own)    # (b)
        bound("planted %s out=%s" % (name, lay), got, c.split64, c.Y)


@pytest.mark.parametrize("what", ["null_W2s", "misaligned_term"])
def test_refusals_write_nothing(dev, what):
    p = SS.inputs("stream_33")
    s = Inputs(p, dev)
    out, strides, _ = out_view(dev, "A", p.B, p.M, 256)
    d = s.desc(out, strides, True, True, True)
    if what == "null_W2s":
        d.W2s = None
    else:
        d.l0_point_term = s.term.data_ptr() + 4
    with pytest.raises(RuntimeError, match="PTT_EINVAL"):
        guard.launch("ptt_sa_stream_split_f32", dev, ctypes.byref(d))
    torch.cuda.synchronize()
    guard.assert_untouched(out)
    untouched_inputs(s.ins)


def test_empty_launches_write_nothing(dev):
    p = SS.inputs("stream_33")
    s = Inputs(p, dev)
    out, strides, _ = out_view(dev, "A", p.B, p.M, 256)
    for B, M in ((0, p.M), (p.B, 0)):
        d = s.desc(out, strides, True, True, True)
        d.B, d.M = B, M
        guard.launch("ptt_sa_stream_split_f32", dev, ctypes.byref(d))
    torch.cuda.synchronize()
    guard.assert_untouched(out)


def test_ops_wrapper_equals_the_raw_launch(dev):
    p = SS.inputs("stream_33")
    s = Inputs(p, dev)
    raw = s.run(dev, "A")
    args = (s.xyz, s.new_xyz, s.idx, (s.term, s.wx, True), ops.pack_weight_split(p.W1.to(dev)), s.sh1,
            ops.pack_weight_split(p.W2.to(dev)), s.sh2, p.radius, True)
    got = ops.sa_stream_split(*args)
    assert got.shape == (p.B, 256, p.M) and got.stride(1) == 1                   # point-major storage
    same_bits(got.cpu(), raw, "ops.sa_stream_split against the raw launch")
    same_bits(ops.sa_stream_split(*args, point_major_out=False).cpu(), raw, "channel-major output")
    with pytest.raises(ValueError):
        ops.sa_stream_split(s.xyz, s.new_xyz, s.idx, (s.term, s.wx, True), args[6], s.sh1, args[6], s.sh2, p.radius, True)


# ================================================================================================================ module
def _module(dev, layers, mlp, precision=None, radius=0.5):
    m = PointnetSAModuleVotes(mlp=list(mlp), radius=radius, nsample=32, use_xyz=True, normalize_xyz=True).eval()
    with torch.no_grad():
        for unit, L in zip(m.mlp_module, layers):
            bn = unit.normlayer.bn
            unit.conv.weight.copy_(L["conv_weight"])
            bn.weight.copy_(L["bn_weight"]); bn.bias.copy_(L["bn_bias"])
            bn.running_mean.copy_(L["bn_mean"]); bn.running_var.copy_(L["bn_var"])
            bn.eps = L["eps"]
    if precision is not None:
        m.precision = precision
    return m.to(dev)


def test_module(dev):
    c = FR.sa_case("stream_1027")
    xyz, feats = c.xyz.to(dev), c.feats.to(dev)
    inds = torch.from_numpy(O.fps(c.xyz.numpy(), c.M)).to(dev)
    split, never = _module(dev, c.layers, [128, 128, 128, 256], 'bf16x2'), _module(dev, c.layers, [128, 128, 128, 256])
    ops.unfused_calls.clear()
    ops.precision_fallbacks.clear()
    with torch.no_grad():
        new_xyz, y, _ = split(xyz, feats, c.M, inds=inds)
        _, y0, _ = never(xyz, feats, c.M, inds=inds)
        # the direct call on the module's own folded packs
        layers, hoist = split._fused_params(xyz.device)
        S = split._split_params(xyz.device)
        term = ops.linear(feats.transpose(1, 2).contiguous(), hoist[0], 128, None, layers[0].shift, relu=False)
        idx = ops.ball_query(new_xyz, xyz, 0.5, 32)
        assert torch.equal(idx.cpu(), c.idx) and torch.equal(new_xyz.cpu(), c.new_xyz)
        direct = ops.sa_stream_split(xyz, new_xyz, idx, (term, hoist[1], hoist[3]), S['w1s'], S['shift1'], S['w2s'], S['shift2'],
                                     0.5, True, relu2=S['relu2'])
    torch.cuda.synchronize()
    assert not ops.unfused_calls and not ops.precision_fallbacks, (ops.unfused_calls, ops.precision_fallbacks)
    same_bits(y.cpu(), direct.cpu(), "'bf16x2' module against ops.sa_stream_split on its own packs")
    assert not torch.equal(y, y0), "'bf16x2' gave the fp32 bits: the split kernel did not run"
    np.testing.assert_allclose(y0.cpu().numpy(), c.ref32.numpy(), **FR.TOL)
    share = lambda t: float(((t.cpu().double() - c.ref64).abs() / (FR.TOL["atol"] + FR.TOL["rtol"] * c.ref64.abs())).max())
    print("MODULE stream_1027: 'bf16x2' at %.2f of TOL from ref64, 'fp32' at %.3f" % (share(y), share(y0)))      # reported, not asserted
    with torch.no_grad():
        split.precision = 'fp32'
        _, y1, _ = split(xyz, feats, c.M, inds=inds)
    same_bits(y1.cpu(), y0.cpu(), "'fp32' after 'bf16x2' against a module whose attribute was never set")
    assert not split._split_cache.held() and not never._split_cache.held()      # fp32 mode packs nothing new


def test_module_sa0_stays_fp32_and_says_so_once(dev):
    c = FR.sa_case("lds12_1035")
    xyz = c.xyz.to(dev)
    inds = torch.from_numpy(O.fps(c.xyz.numpy(), c.M)).to(dev)
    mk = lambda precision=None: _module(dev, c.layers, [0, 64, 64, 128], precision, radius=c.radius)
    split, plain = mk('bf16x2'), mk()
    ops.precision_fallbacks.clear()
    with torch.no_grad(), warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        y = split(xyz, None, c.M, inds=inds)[1]
        y0 = plain(xyz, None, c.M, inds=inds)[1]
    same_bits(y.cpu(), y0.cpu(), "a 'bf16x2' SA0 module against fp32")
    assert list(ops.precision_fallbacks.values()) == [1], ops.precision_fallbacks
    assert "sa_lds_kernel" in list(ops.precision_fallbacks)[0][1]
    assert len([w for w in seen if "bf16x2" in str(w.message)]) == 1
    ops.precision_fallbacks.clear()


# ================================================================================================================ graphs
def test_graph_is_captured_again_when_the_sa_precision_changes(dev):
    from ptt_amd.hot_path import FrameHotPath, GraphedHotPath, kitti_model_cfg, randomize_
    keys = ("search_feats", "centroid_feats", "box_feats", "pred_box_center")
    B = 8
    s, t = (torch.from_numpy(a).to(dev) for a in synth.frames(77, B, 1024, 512))
    model = randomize_(FrameHotPath(kitti_model_cfg()), seed=11).to(dev).eval()
    grab = lambda out: {k: out[k].clone() for k in keys}
    scope = ('transformer', 'sa')
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")     # SA0 and the box transformer's 8 x 64 points stay fp32 and say so
        g = GraphedHotPath(model, s, t)
        first = grab(g(s, t))
        assert set_precision(model, 'bf16x2', scope=scope) == 2 + 3
        second = grab(g(s, t))
        assert g.captures == 2
        fresh_model = randomize_(FrameHotPath(kitti_model_cfg()), seed=11).to(dev).eval()
        set_precision(fresh_model, 'bf16x2', scope=scope)
        fresh = grab(GraphedHotPath(fresh_model, s, t)(s, t))
        set_precision(model, 'fp32', scope=scope)
        third = grab(g(s, t))
        assert g.captures == 3
    torch.cuda.synchronize()
    for k in keys:
        assert torch.equal(second[k], fresh[k]), "%s: replay after set_precision differs from a runner built in 'bf16x2'" % k
        assert torch.equal(third[k], first[k]), "%s: back in 'fp32' the first result does not come back" % k
    assert not torch.equal(second["search_feats"], first["search_feats"]), "'bf16x2' replayed the fp32 SA arithmetic"
    ops.precision_fallbacks.clear()


def test_zz_ratio_report():
    RATIOS.report()
