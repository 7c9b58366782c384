"""ptt_pack_weight_split_bf16, ptt_pt_attn_pair_split_f32 and TransformerBlock.precision = 'bf16x2' on the GPU, against the split
arithmetic in float64 (tests/pair_split_ref.py), behind guard bands (tests/guard.py) — launched as test_pair of
tests/test_fused_guard_gpu.py launches the fp32 kernel: outputs guarded(...), every input embed(...)-ded, untouched_inputs.

Pack: bit for bit the numpy restatement of the header's element order at (Cout, K) = (128,128), (256,256), (512,512); K = 24 and
Cout = 48 are refused (PTT_EINVAL) and leave the output untouched.

Kernel, all nine (D, k) on the clouds of pair_shapes_ref.CLOUDS for that k, rel and order on / off, attn on / off; per case
  (a) max|got - split64| / max|split64| <= R * Y for res (through fc2 + residual, as the fp32 files chain it), for the kernel's
      own res before fc2, and for attn; Y = max(e32, 4u) from the float32 run of the same emulation; R = R_RATIO = 4, R <= 8;
  (b) the split is really there: max|got - split64| <= 0.25 * max|split64 - exact64| on res (both forms). A kernel that ran
      fp32, or dropped a cross term, fails it; not applied to attn, whose split distance is of the size of exp2 / rcp's error;
  (c) check_guard on outputs and inputs;
  (d) attn off equals attn on bit for bit on res; rel and order change no bit; a second run gives the same bits;
  (e) N = 17 at k = 16 and D = 384 are refused and leave the outputs untouched.

Module: TransformerBlock(256, 512, 16) with precision 'bf16x2' on fixture G5's N = 128 inputs tiled past PER_LAYER_MAX_POINTS
meets TOL against the fixture tiled the same way; 'fp32' gives the bits of a block whose attribute was never set; below the
per-layer limit 'bf16x2' gives the fp32 bits and notes the fallback once.
Graphs: a GraphedHotPath at batch 8 in fp32, after set_precision(model, 'bf16x2'), and after switching back: the second result
equals a fresh runner's built in 'bf16x2' bit for bit, the third equals the first.

err / Y measured on an MI355X (res / res before fc2 / attn; worst over rel and order on / off — those runs agree bit for bit),
and (b)'s ratio max|got - split64| / max|split64 - exact64| on res / res before fc2:
  (D, k)      N = k                              3 clouds                           many tiles
  (128,  8)   0.90 / 0.99 / 1.30  0.226 / 0.117    0.36 / 1.16 / 0.74  0.075 / 0.081    0.23 / 1.09 / 1.00  0.112 / 0.092
  (128, 16)   0.38 / 1.18 / 1.03  0.086 / 0.091    0.39 / 0.89 / 0.96  0.089 / 0.051    0.26 / 1.01 / 1.02  0.116 / 0.067
  (128, 32)   0.57 / 0.63 / 1.03  0.127 / 0.047    0.39 / 0.85 / 1.13  0.114 / 0.074    0.25 / 0.66 / 0.88  0.087 / 0.057
  (256,  8)   0.41 / 0.79 / 0.86  0.106 / 0.061    0.28 / 1.10 / 0.95  0.089 / 0.091    0.46 / 1.03 / 0.98  0.217 / 0.199
  (256, 16)   0.35 / 0.96 / 0.91  0.120 / 0.106    0.42 / 0.84 / 0.96  0.138 / 0.095    0.23 / 0.53 / 0.98  0.094 / 0.082
  (256, 32)   0.32 / 0.69 / 0.75  0.088 / 0.069    0.34 / 0.80 / 0.84  0.104 / 0.089    0.18 / 0.73 / 0.73  0.090 / 0.085
  (512,  8)   0.57 / 0.86 / 0.87  0.127 / 0.090    0.30 / 1.71 / 1.01  0.098 / 0.148    0.20 / 1.05 / 0.91  0.107 / 0.089
  (512, 16)   0.39 / 1.15 / 0.94  0.092 / 0.091    0.33 / 0.84 / 0.99  0.112 / 0.065    0.30 / 0.74 / 0.90  0.099 / 0.062
  (512, 32)   0.41 / 0.89 / 0.80  0.105 / 0.078    0.34 / 0.91 / 0.74  0.092 / 0.074    0.23 / 0.78 / 0.70  0.105 / 0.078
Worst err / Y 1.71 ((512, 8), 3 clouds, res before fc2): no case came near the bar of 4, none needed investigation, R stays 4.
Worst share 0.226 (bar 0.25). The float32 CPU run of the emulation itself measures 0.08 - 0.24 on res at (128,8,1,8), (256,8,1,52),
(512,16,1,16), (512,8,3,12): at these shapes the kernel's distance from the split arithmetic is float32 rounding, a tenth to a
quarter of the split's own distance from exact float64 (an estimate of 0.008 - 0.018 made before the kernel existed was too low).
Module on G5 tiled x3: max |res - fixture| 2.03e-06, attn sample 2.2e-08.
"""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest
import torch

from ptt_amd import ops, synth
from ptt_amd.models.transformer_block.variants import PER_LAYER_MAX_POINTS, TransformerBlock
from ptt_amd.precision import set_precision
from tests import fused_ref as FR
from tests import guard
from tests import pair_shapes_ref as S
from tests import pair_split_ref as PS
from tests.fused_launch import F32, I32, R_RATIO, same_bits, untouched_inputs
from tests.guard import check_guard, embed, guarded
from tests.util import transformer_params

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SPLIT_SHARE = 0.25          # (b): the kernel lies at most this fraction of the split's own distance from exact away from split64
RATIOS = {}


def test_r_is_within_its_cap():
    assert R_RATIO <= 8


def note(case, err, Y):
    r = err / Y
    key = re.sub(r" rel=\d order=\d", "", case)
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)
    print("RATIO %-56s err %.3e  Y %.3e  err/Y %.2f" % (case, err, Y, r))
    return r


def bound(case, got, ref64, Y):
    r = note(case, FR.rel_err(got, ref64), Y)
    assert r <= R_RATIO, "%s: %.2f x the float32 emulation's own distance from float64 (R = %g)" % (case, r, R_RATIO)


def split_is_there(case, got, split64, exact64):
    d = float((got.double() - split64).abs().max())
    s = float((split64 - exact64).abs().max())
    key = re.sub(r" rel=\d order=\d", "", case)
    RATIOS[key] = max(RATIOS.get(key, 0.0), d / s)
    print("SPLIT %-56s |got - split64| %.3e  |split64 - exact64| %.3e  ratio %.3f" % (case, d, s, d / s))
    assert d <= SPLIT_SHARE * s, "%s: %.3e from the split arithmetic, which itself lies %.3e from exact" % (case, d, s)


def as_words(pack):
    """A split pack (int16 words) as the int32 tensor tests/guard.py embeds."""
    return pack.view(I32)


# ================================================================================================================== pack
@pytest.mark.parametrize("Cout,K", [(128, 128), (256, 256), (512, 512)])
def test_pack(dev, Cout, K):
    rs = np.random.RandomState(Cout + K)
    w = rs.uniform(-1.0, 1.0, (Cout, K)).astype(np.float32) / np.float32(np.sqrt(K))
    w[0, :8] = [0.0, 1.0, -1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 2.0 ** -20, -3.5, 255.0 / 256.0]       # ties and exact values
    n = int(ops._host("ptt_split_weight_elems", Cout, K))
    assert n == 2 * Cout * K
    w_e = embed(torch.from_numpy(w).to(dev))
    out = guarded((n // 2,), I32, device=dev)
    guard.launch("ptt_pack_weight_split_bf16", dev, guard.ptr(w_e), Cout, K, guard.ptr(out))
    torch.cuda.synchronize()
    check_guard(out)
    untouched_inputs([w_e])
    got = out.cpu().contiguous().numpy().view(np.uint16)
    want = PS.split_pack_np(w)
    assert got.shape == want.shape and np.array_equal(got, want), "%d of %d words differ" % (int((got != want).sum()), want.size)
    assert torch.equal(ops.pack_weight_split(torch.from_numpy(w).to(dev)).cpu(), torch.from_numpy(want.view(np.int16)))


@pytest.mark.parametrize("Cout,K", [(128, 24), (48, 128)])
def test_pack_refusal(dev, Cout, K):
    w = torch.zeros((Cout, K), dtype=F32, device=dev)
    out = guarded((Cout * K,), I32, device=dev)
    with pytest.raises(RuntimeError, match="PTT_EINVAL"):
        guard.launch("ptt_pack_weight_split_bf16", dev, guard.ptr(w), Cout, K, guard.ptr(out))
    torch.cuda.synchronize()
    guard.assert_untouched(out)
    with pytest.raises(ValueError):
        ops.pack_weight_split(w)


# ================================================================================================================ kernel
def _desc(xyz, knn, qkv, w, res, attn, B, N, k, D, rel=None, order=None):
    d = ops.AttnSplitDesc()
    d.xyz, d.knn, d.qkv = xyz.data_ptr(), knn.data_ptr(), qkv.data_ptr()
    d.rel = rel.data_ptr() if rel is not None else None
    d.order = order.data_ptr() if order is not None else None
    for f in ("Wd1p", "Wd2s", "bd2", "Wg1s", "bg1", "Wg2s", "bg2"):
        setattr(d, f, w[f].data_ptr())
    d.res, d.attn = res.data_ptr(), attn.data_ptr() if attn is not None else None
    d.B, d.N, d.k, d.D = B, N, k, D
    return d


def pair_run(dev, c, w, qkv_e, xyz_e, knn_e, ins, rel, order, want_attn):
    B, N, D, k = c.B, c.N, c.D, c.k
    res = guarded((B, N, D), F32, device=dev)
    attn = guarded((B, N * k, D), F32, device=dev) if want_attn else None
    d = _desc(xyz_e, knn_e, qkv_e, w, res, attn, B, N, k, D, rel, order)
    guard.launch("ptt_pt_attn_pair_split_f32", dev, ctypes.byref(d))
    torch.cuda.synchronize()
    check_guard(res)
    if attn is not None:
        check_guard(attn)
    untouched_inputs(ins + [v for v in (rel, order) if v is not None])
    return res, attn


@pytest.mark.parametrize("D,k,B,N", PS.CASES)
def test_pair_split(dev, D, k, B, N):
    c = PS.pair_case_split(B, N, D, k)
    P = c.P
    dv = lambda n: P[n].to(dev).contiguous()
    ins = []
    keep = lambda v: (ins.append(v), v)[1]
    xyz_d = c.xyz.to(dev)
    knn_d, rel_d = ops.knn(xyz_d, k, want_rel=True)
    assert torch.equal(knn_d.cpu(), c.knn), "the device kNN table is not the oracle's"
    order_d = ops.spatial_order(xyz_d)
    assert torch.equal(order_d.view(B, N).sort(dim=1)[0].cpu(), (torch.arange(B * N, dtype=I32).view(B, N)))
    x = ops.linear(c.feats.to(dev), ops.pack_weight(dv("fc1.weight")), D, None, dv("fc1.bias"))
    wqkv = torch.cat([P["w_qs.weight"], P["w_ks.weight"], P["w_vs.weight"]], 0).to(dev)
    qkv = ops.linear(x, ops.pack_weight(wqkv), 3 * D)
    sp = lambda n: as_words(ops.pack_weight_split(dv(n)))
    w = dict(Wd1p=ops.pack_delta0(dv("fc_delta.0.weight"), dv("fc_delta.0.bias")), Wd2s=sp("fc_delta.2.weight"),
             bd2=dv("fc_delta.2.bias"), Wg1s=sp("fc_gamma.0.weight"), bg1=dv("fc_gamma.0.bias"),
             Wg2s=sp("fc_gamma.2.weight"), bg2=dv("fc_gamma.2.bias"))
    w = {n: keep(embed(t)) for n, t in w.items()}
    qkv_e, xyz_e, knn_e = keep(embed(qkv.contiguous())), keep(embed(xyz_d)), keep(embed(knn_d))
    rel_e, order_e = embed(rel_d.view(B, N * k, 3).contiguous()), embed(order_d.view(B, N).contiguous())
    name = "split D=%d k=%d (%d,%d)" % (D, k, B, N)
    fc2 = ops.pack_weight(dv("fc2.weight"))

    def results(res, attn):      # the block's output: fc2 + residual on the linear kernel, as the fp32 files chain it
        out = ops.linear(res, fc2, S.D_POINTS, None, dv("fc2.bias"), False, c.feats.to(dev))
        return out.cpu(), (attn.view(B, N, k, D).cpu() if attn is not None else None)

    first = None
    for use_rel in (False, True):
        for use_order in (False, True):
            tag = "%s rel=%d order=%d" % (name, use_rel, use_order)
            rel, order = rel_e if use_rel else None, order_e if use_order else None
            res, attn = pair_run(dev, c, w, qkv_e, xyz_e, knn_e, ins, rel, order, True)
            out_h, attn_h = results(res, attn)
            res_bits = res.cpu().contiguous()
            bound(tag + " res", out_h, c.res64, c.Y_res)
            bound(tag + " pre", res_bits, c.pre64, c.Y_pre)
            bound(tag + " attn", attn_h, c.attn64, c.Y_attn)
            split_is_there(tag + " res  share", out_h, c.res64, c.exact_res64)
            split_is_there(tag + " pre  share", res_bits, c.pre64, c.exact_pre64)
            res_off, none = pair_run(dev, c, w, qkv_e, xyz_e, knn_e, ins, rel, order, False)
            assert none is None
            same_bits(res_off.cpu(), res_bits, tag + ": attn off against attn on")
            if first is None:
                first = (res_bits, attn_h)
                again, attn2 = pair_run(dev, c, w, qkv_e, xyz_e, knn_e, ins, None, None, True)
                same_bits(again.cpu(), res_bits, tag + ": second run")
                same_bits(results(again, attn2)[1], attn_h, tag + ": second run, attn")
            # rel = the kNN kernel's own xyz_i - xyz_j, the same float32 subtraction the kernel makes; order changes no arithmetic
            same_bits(res_bits, first[0], tag + ": res against rel = NULL, order = NULL")
            same_bits(attn_h, first[1], tag + ": attn against rel = NULL, order = NULL")


def _rand(dev, *shape):
    return torch.from_numpy(np.random.RandomState(sum(shape)).standard_normal(shape).astype(np.float32)).to(dev)


@pytest.mark.parametrize("what,N,k,D", [("k16_N17", 17, 16, 512), ("D384", 32, 16, 384)])
def test_pair_split_refusal(dev, what, N, k, D):
    """Every array has the size the refused shape would need: were the launch not refused, it would run inside its buffers."""
    B = 1
    xyz = _rand(dev, B, N, 3)
    knn = torch.arange(k, dtype=I32, device=dev).repeat(B, N, 1) % N
    res, attn = guarded((B, N, D), F32, device=dev), guarded((B, N * k, D), F32, device=dev)
    qkv, wd1, bias = _rand(dev, B, N, 3 * D), ops.pack_weight(_rand(dev, D, 4)), _rand(dev, D)
    wsq = torch.zeros((2 * D * D,), dtype=torch.int16, device=dev)
    w = dict(Wd1p=wd1, Wd2s=wsq, bd2=bias, Wg1s=wsq, bg1=bias, Wg2s=wsq, bg2=bias)
    d = _desc(xyz, knn, qkv, w, res, attn, B, N, k, D)
    with pytest.raises(RuntimeError, match="PTT_EUNSUPPORTED"):
        guard.launch("ptt_pt_attn_pair_split_f32", dev, ctypes.byref(d))
    torch.cuda.synchronize()
    guard.assert_untouched(res, attn)


# ================================================================================================================ module
def _g5_block(dev, precision=None):
    blk = TransformerBlock(256, 512, 16).eval()
    blk.load_state_dict(transformer_params(628))
    if precision is not None:
        blk.precision = precision
    return blk.to(dev)


def _g5_tiled(dev, times):
    g = np.load(os.path.join(GOLD, "G5_transformer.npz"))
    t = lambda a: torch.from_numpy(np.concatenate([a] * times, 0))
    return t(g["xyz128"]).to(dev), t(g["feat128"]).to(dev), t(g["res128"]), t(g["attn_sample128"])


def test_module_bf16x2_meets_the_contract_on_g5(dev):
    g = np.load(os.path.join(GOLD, "G5_transformer.npz"))
    times = PER_LAYER_MAX_POINTS // (g["xyz128"].shape[0] * 128) + 1
    xyz, feat, res_ref, attn_ref = _g5_tiled(dev, times)
    assert xyz.shape[0] * xyz.shape[1] > PER_LAYER_MAX_POINTS
    blk = _g5_block(dev, 'bf16x2')
    ops.unfused_calls.clear()
    ops.precision_fallbacks.clear()
    with torch.no_grad():
        res, attn = blk(xyz, feat)
        res_na, none = blk(xyz, feat, want_attn=False)
    torch.cuda.synchronize()
    assert not ops.unfused_calls and not ops.precision_fallbacks, (ops.unfused_calls, ops.precision_fallbacks)
    assert none is None and torch.equal(res, res_na)
    print("G5 tiled x%d bf16x2: max |res - fixture| %.3e, attn sample %.3e" % (
        times, float((res.cpu() - res_ref).abs().max()), float((attn[:, ::16, :, ::32].cpu() - attn_ref).abs().max())))
    np.testing.assert_allclose(res.cpu().numpy(), res_ref.numpy(), **FR.TOL)
    np.testing.assert_allclose(attn[:, ::16, :, ::32].cpu().numpy(), attn_ref.numpy(), **FR.TOL)
    # the same block in 'fp32': the bits of a block that never had the attribute set, and not the split kernel's
    never = _g5_block(dev)
    with torch.no_grad():
        r0, a0 = never(xyz, feat)
        blk.precision = 'fp32'
        r1, a1 = blk(xyz, feat)
    same_bits(r1.cpu(), r0.cpu(), "fp32 after bf16x2 against a block that never had the attribute set: res")
    same_bits(a1.cpu(), a0.cpu(), "fp32 after bf16x2 against a block that never had the attribute set: attn")
    assert not torch.equal(r0, res), "'bf16x2' gave the fp32 bits: the split kernel did not run"
    assert 'wd2s' not in blk._params() and 'wd2s' not in never._params()       # fp32 mode packs nothing new


def test_module_below_the_per_layer_limit_stays_fp32(dev):
    xyz, feat, _, _ = _g5_tiled(dev, 1)
    assert xyz.shape[0] * xyz.shape[1] <= PER_LAYER_MAX_POINTS
    split, plain = _g5_block(dev, 'bf16x2'), _g5_block(dev)
    ops.precision_fallbacks.clear()
    with torch.no_grad(), warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        for want_attn in (True, False, True):
            r, a = split(xyz, feat, want_attn=want_attn)
            r0, a0 = plain(xyz, feat, want_attn=want_attn)
            same_bits(r.cpu(), r0.cpu(), "bf16x2 below the per-layer limit, want_attn=%s" % want_attn)
            if want_attn:
                same_bits(a.cpu(), a0.cpu(), "attn below the per-layer limit")
    assert list(ops.precision_fallbacks.values()) == [3], ops.precision_fallbacks
    assert len([w for w in seen if "bf16x2" in str(w.message)]) == 1
    ops.precision_fallbacks.clear()


# ================================================================================================================ graphs
def test_graph_is_captured_again_when_the_precision_changes(dev):
    from ptt_amd.hot_path import FrameHotPath, GraphedHotPath, kitti_model_cfg, randomize_
    keys = ("search_feats", "centroid_feats", "box_feats", "pred_box_center")
    B = 8                                   # 8 x 128 seeds > PER_LAYER_MAX_POINTS: the centroid transformer runs the pair kernel
    s, t = (torch.from_numpy(a).to(dev) for a in synth.frames(77, B, 1024, 512))
    model = randomize_(FrameHotPath(kitti_model_cfg()), seed=11).to(dev).eval()
    grab = lambda out: {k: out[k].clone() for k in keys}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")     # the box transformer's 8 x 64 points stay on the fp32 per-layer form and say so
        g = GraphedHotPath(model, s, t)
        first = grab(g(s, t))
        assert set_precision(model, 'bf16x2') == 2
        second = grab(g(s, t))
        assert g.captures == 2
        fresh_model = randomize_(FrameHotPath(kitti_model_cfg()), seed=11).to(dev).eval()
        set_precision(fresh_model, 'bf16x2')
        fresh = grab(GraphedHotPath(fresh_model, s, t)(s, t))
        set_precision(model, 'fp32')
        third = grab(g(s, t))
        assert g.captures == 3
    torch.cuda.synchronize()
    for k in keys:
        assert torch.equal(second[k], fresh[k]), "%s: replay after set_precision differs from a runner built in 'bf16x2'" % k
        assert torch.equal(third[k], first[k]), "%s: back in 'fp32' the first result does not come back" % k
    assert not torch.equal(second["centroid_feats"], first["centroid_feats"]), "'bf16x2' replayed the fp32 arithmetic"
    ops.precision_fallbacks.clear()


def test_zz_ratio_report():
    for case in sorted(RATIOS):
        print("WORST %-60s %.3f" % (case, RATIOS[case]))
