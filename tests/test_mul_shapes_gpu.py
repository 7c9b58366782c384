"""ptt_pt_attn_pair_f32's multi-head form and MulTransformerBlock at DIM_MODEL 128 / 256 x KNN 8 / 16 / 32, heads with
hd = D / heads >= 32 (cases, seeds and references: tests/mul_shapes_ref.py) — the shapes beside the shipped (512, 16), which
tests/test_fused_guard_gpu.py and tests/test_multitransformer_gpu.py hold to the same bars.

Kernel level, per (D, heads > 1, k) — 5 x 3 = 15 instantiations of pt_attn_pair_heads_kernel<D, KNN, HEADS> — and per cloud of
pair_shapes_ref.CLOUDS (N = k; three clouds with an odd tile count; many tiles): q | k | v formed in float32 on the host; the device
kNN table equals oracle.index_ops.knn; with every operand embed()-ded between NaN / INDEX_FILL words and guarded outputs,
  (a) err / Y <= 4 for res and attn, Y = max(e32, 4u) the float32 oracle's (fused_ref.heads_attention) own distance from its float64
      run on the same table (fused_ref.yardstick);  (b) assert_allclose against the float32 oracle at FR.TOL;
  (c) the same bits with rel on / off, order = ops.spatial_order(xyz) / NULL, attn on / off (res), and on a second run;
  (d) guard words intact, inputs untouched.
Refusals (PTT_EUNSUPPORTED, outputs untouched): D 128 heads 8 (hd 16); D 256 heads 16; D 256 heads 3; D 256 heads 2 k 8 N 10; D 384.

Module level: MulTransformerBlock(256, D, k, heads, layers).eval() under no_grad on 48 x 40 and 1 x 40 points takes the fused path
(ops.unfused_calls stays empty — the test that fails without the instantiations), want_attn=False gives the same res bits, attn is
(B * heads, N, k, hd), and res / per-point sorted attn lie within 4 Y of a float64 copy of the module on its stock path, Y the
float32 stock path's distance from that run; the eval-mode module against fixture G24 (the reference's own block) at FR.TOL; the
tracker with DIM_MODEL 256, KNN 8 in both blocks against itself on the stock path. Training: mul_block_usable holds, a step runs
with F.softmax, F.layer_norm and Tensor.argsort forbidden, and every gradient lies within R_TRAIN x the stock float32 sequence's own
distance from a float64 run on the same kNN table.

err / Y measured on an MI355X (res / attn, worst over rel and order on / off — the runs agree bit for bit):
  (D, heads, k)   N = k          3 clouds       many tiles
  (128, 2,  8)   0.43 / 0.70    0.71 / 0.78    0.53 / 0.82
  (128, 2, 16)   0.54 / 0.77    0.69 / 0.93    0.53 / 0.90
  (128, 2, 32)   0.50 / 0.73    0.61 / 0.75    0.56 / 0.79
  (128, 4,  8)   0.51 / 0.71    0.60 / 0.77    0.55 / 0.80
  (128, 4, 16)   0.52 / 0.87    0.78 / 0.82    0.61 / 0.82
  (128, 4, 32)   0.66 / 0.82    0.68 / 0.86    0.70 / 0.76
  (256, 2,  8)   0.68 / 0.80    0.58 / 0.83    0.76 / 0.81
  (256, 2, 16)   0.63 / 0.86    0.85 / 0.95    0.63 / 0.92
  (256, 2, 32)   0.72 / 0.72    0.70 / 0.77    0.56 / 0.75
  (256, 4,  8)   0.65 / 0.75    0.74 / 0.81    0.71 / 0.82
  (256, 4, 16)   0.67 / 0.83    0.67 / 0.93    0.60 / 0.88
  (256, 4, 32)   0.57 / 0.80    0.65 / 0.75    0.53 / 0.82
  (256, 8,  8)   0.62 / 0.73    0.92 / 0.84    0.74 / 0.87
  (256, 8, 16)   0.57 / 0.86    0.56 / 0.92    0.59 / 0.90
  (256, 8, 32)   0.53 / 0.80    0.88 / 0.76    0.73 / 0.67
No case came near the bar of 4; none needed investigation.
Module level, (D, k, heads, layers): res / attn at B = 48, then at B = 1:
  (128,  8, 1, 1) 0.71 / 0.82, 0.68 / 1.05   (128, 16, 2, 1) 0.66 / 1.15, 0.73 / 0.65   (128, 32, 4, 1) 0.56 / 0.70, 0.73 / 1.04
  (256, 32, 1, 1) 0.63 / 0.75, 0.46 / 0.76   (256,  8, 2, 1) 0.56 / 0.91, 0.36 / 0.79   (256, 16, 4, 1) 0.50 / 0.89, 0.36 / 0.73
  (256, 32, 8, 1) 0.82 / 0.99, 0.45 / 0.98   (256,  8, 4, 2) 0.62 / 0.60, 0.36 / 0.75
Training, e_hip / e_ref per gradient (worst over res, parameters, features, xyz), B = 2, N = 40:
  (256,  8, heads 4, 1 layer):  2.65 (fc_gamma.0.bias: e_ref 5.4e-7, e_hip 1.4e-6), then 1.49 (fc_delta.0.bias), 1.06; every weight,
                                features and xyz 0.73 - 0.99; res 1.00; fc_gamma.2.bias |g - g64| 4.3e-7 (stock float32 4.2e-7)
  (256, 16, heads 2, 2 layers): 2.23 (layers.0.fc_gamma.0.bias), 1.79 (layers.1.fc_gamma.0.bias); fc_gamma.2.bias 3.6e-7 / 3.8e-7
                                — the first launches of ptt_rows_gemm_rsum16_heads_f32 at D = 256
  (128, 32, heads 2, 1 layer):  2.45 (fc_gamma.0.bias: e_ref 6.4e-7, e_hip 1.6e-6); fc_gamma.2.bias 6.8e-7
fc_gamma.0.bias is the parameter that led TransformerBlock's table too (2.94 at (256, 8), tests/test_pair_shapes_gpu.py).
R_TRAIN = twice the worst ratio (2.65), rounded up to one significant digit = 6, and R_TRAIN <= 8 is asserted.
Run once with the same measurement but not among the cases above (the head width 32 path, where fc_gamma runs on the linear
kernel instead of the row GEMM, and one head at 128): (256, 8, heads 8) 1.44, (128, 16, heads 4) 1.56, (256, 32, heads 8,
2 layers) 1.39, (128, 8, heads 1) 3.08 — all under the bar.
"""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from ptt_amd import ops, synth, train_ops
from ptt_amd.models.model_utils import index_points
from ptt_amd.models.transformer_block.multitransformer import MulTransformerBlock
from tests import fused_ref as FR
from tests import guard
from tests import multitransformer_ref as M
from tests import mul_shapes_ref as S
from tests.guard import check_guard, embed, guarded

pytestmark = pytest.mark.gpu
F32, I32 = torch.float32, torch.int32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

R_RATIO = 4.0               # the bar tests/test_fused_guard_gpu.py holds the shipped shape to
R_TRAIN = 6.0               # twice the worst measured e_hip / e_ref (2.65, table above), one significant digit
RATIOS = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def test_r_train_is_within_its_cap():
    assert R_TRAIN <= 8


def note(case, err, Y):
    r = err / Y
    key = re.sub(r" rel=\d order=\d", "", case)           # worst over rel and order on / off
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)
    print("RATIO %-60s err %.3e  Y %.3e  err/Y %.2f" % (case, err, Y, r))
    return r


def bound(case, got, ref64, ref32, Y):
    r = note(case, FR.rel_err(got, ref64), Y)
    assert r <= R_RATIO, "%s: %.2f x the float32 oracle's own distance from float64 (R = %g)" % (case, r, R_RATIO)
    np.testing.assert_allclose(got.numpy(), ref32.numpy(), **FR.TOL)


def bits(t):
    return t.contiguous().view(I32)


def same_bits(a, b, what):
    assert a.shape == b.shape and torch.equal(bits(a), bits(b)), "%s: not the same bits" % what


def _desc(xyz, knn, qkv, w, res, attn, B, N, k, D, heads, rel=None, order=None):
    d = ops.AttnDesc()
    d.xyz, d.knn, d.qkv = xyz.data_ptr(), knn.data_ptr(), qkv.data_ptr()
    d.rel = rel.data_ptr() if rel is not None else None
    d.order = order.data_ptr() if order is not None else None
    for f in ("Wd1p", "Wd2p", "bd2", "Wg1p", "bg1", "Wg2p", "bg2"):
        setattr(d, f, w[f].data_ptr())
    d.res, d.attn = res.data_ptr(), attn.data_ptr() if attn is not None else None
    d.B, d.N, d.k, d.D, d.heads = B, N, k, D, heads
    return d


def pair_run(dev, c, w, qkv_e, xyz_e, knn_e, ins, rel, order, want_attn):
    B, N, D, k, H = c.B, c.N, c.D, c.k, c.heads
    res = guarded((B, N, D), F32, device=dev)
    attn = guarded((B * H, N * k, D // H), F32, device=dev) if want_attn else None
    d = _desc(xyz_e, knn_e, qkv_e, w, res, attn, B, N, k, D, H, rel, order)
    guard.launch("ptt_pt_attn_pair_f32", dev, ctypes.byref(d))
    torch.cuda.synchronize()
    check_guard(res)
    if attn is not None:
        check_guard(attn)
    for v in ins + [v for v in (rel, order) if v is not None]:
        check_guard(v, all_written=False)
    return res, attn


@pytest.mark.parametrize("D,H,k,B,N", S.KERNEL_CASES)
def test_pair_heads(dev, D, H, k, B, N):
    c = S.kernel_case(D, H, k, B, N)
    P = c.P
    dv = lambda n: P[n].to(dev).contiguous()
    ins = []
    keep = lambda v: (ins.append(v), v)[1]
    xyz_d = c.xyz.to(dev)
    knn_d, rel_d = ops.knn(xyz_d, k, want_rel=True)
    assert torch.equal(knn_d.cpu(), c.knn), "the device kNN table is not the oracle's"
    order_d = ops.spatial_order(xyz_d)
    assert torch.equal(order_d.view(B, N).sort(dim=1)[0].cpu(), (torch.arange(B * N, dtype=I32).view(B, N)))    # a permutation inside clouds
    w = dict(Wd1p=ops.pack_delta0(dv("fc_delta.0.weight"), dv("fc_delta.0.bias")), Wd2p=ops.pack_weight(dv("fc_delta.2.weight")),
             bd2=dv("fc_delta.2.bias"), Wg1p=ops.pack_weight(dv("fc_gamma.0.weight")), bg1=dv("fc_gamma.0.bias").repeat(H).contiguous(),
             Wg2p=ops.pack_weight(dv("fc_gamma.2.weight")), bg2=dv("fc_gamma.2.bias").repeat(H).contiguous())
    w = {n: keep(embed(t)) for n, t in w.items()}
    qkv_e, xyz_e, knn_e = keep(embed(c.qkv.to(dev).contiguous())), keep(embed(xyz_d)), keep(embed(knn_d))
    rel_e, order_e = embed(rel_d.view(B, N * k, 3).contiguous()), embed(order_d.view(B, N).contiguous())
    name = "pair D=%d heads=%d k=%d (%d,%d)" % (D, H, k, B, N)

    def results(res, attn):
        return res.cpu().contiguous(), (attn.view(B * H, N, k, D // H).cpu() if attn is not None else None)

    first = None
    for use_rel in (False, True):
        for use_order in (False, True):
            tag = "%s rel=%d order=%d" % (name, use_rel, use_order)
            rel, order = rel_e if use_rel else None, order_e if use_order else None
            res, attn = pair_run(dev, c, w, qkv_e, xyz_e, knn_e, ins, rel, order, True)
            out_h, attn_h = results(res, attn)
            bound(tag + " res", out_h, c.res64, c.res32, c.Y_res)
            bound(tag + " attn", attn_h, c.attn64, c.attn32, c.Y_attn)
            res_off, none = pair_run(dev, c, w, qkv_e, xyz_e, knn_e, ins, rel, order, False)
            assert none is None
            same_bits(res_off.cpu(), out_h, tag + ": attn off against attn on")
            if first is None:
                first = (out_h, attn_h)
                again, attn2 = pair_run(dev, c, w, qkv_e, xyz_e, knn_e, ins, None, None, True)
                same_bits(again.cpu(), out_h, tag + ": second run")
                same_bits(results(again, attn2)[1], attn_h, tag + ": second run, attn")
            # rel = the kNN kernel's own xyz_i - xyz_j, the same float32 subtraction the kernel makes; order changes no arithmetic
            same_bits(out_h, first[0], tag + ": res against rel = NULL, order = NULL")
            same_bits(attn_h, first[1], tag + ": attn against rel = NULL, order = NULL")


# ============================================================================================================= refusals
def _rand(dev, *shape):
    return torch.from_numpy(np.random.RandomState(sum(shape)).standard_normal(shape).astype(np.float32)).to(dev)


@pytest.mark.parametrize("what", sorted(S.REFUSED))
def test_refusal(dev, what):
    """Every array has the size the refused shape would need (the weights D x D, more than any head count reads): were the launch
    not refused, it would run inside its buffers."""
    B, N, k, D, heads = S.REFUSED[what]
    xyz = _rand(dev, B, N, 3)
    knn = torch.arange(k, dtype=I32, device=dev).repeat(B, N, 1) % N
    res, attn = guarded((B, N, D), F32, device=dev), guarded((B, N * k, D), F32, device=dev)
    qkv, wsq, wd1, bias = _rand(dev, B, N, 3 * D), ops.pack_weight(_rand(dev, D, D)), ops.pack_weight(_rand(dev, D, 4)), _rand(dev, D)
    w = dict(Wd1p=wd1, Wd2p=wsq, bd2=bias, Wg1p=wsq, bg1=bias, Wg2p=wsq, bg2=bias)
    d = _desc(xyz, knn, qkv, w, res, attn, B, N, k, D, heads)
    with pytest.raises(RuntimeError, match="PTT_EUNSUPPORTED"):
        guard.launch("ptt_pt_attn_pair_f32", dev, ctypes.byref(d))
    torch.cuda.synchronize()
    guard.assert_untouched(res, attn)


# ========================================================================================================= module level
def _block(D, k, heads, layers, dev):
    return M.seeded_(MulTransformerBlock(S.D_POINTS, D, k, heads, layers), S.module_seed(D, k, heads, layers)).to(dev)


def _stock(blk, dtype=None):
    """A copy of the module pinned to its stock op sequence, in `dtype`."""
    ref = copy.deepcopy(blk)
    if dtype is not None:
        ref = ref.to(dtype)
    ref._fusable = lambda *a: False
    return ref


def _sorted(a):
    return a.sort(dim=2)[0]                     # a point's attention values as a set over its k neighbours (per channel)


@pytest.mark.parametrize("D,k,heads,layers", S.MODULE_CASES)
def test_module_eval_takes_the_fused_path(dev, D, k, heads, layers):
    blk = _block(D, k, heads, layers, dev).eval()
    ref64, ref32 = _stock(blk, torch.float64).eval(), _stock(blk).eval()
    for B in S.MODULE_BATCHES:
        xyz, f = S.module_inputs(D, k, heads, B)
        x, fe = torch.from_numpy(xyz).to(dev), torch.from_numpy(f).to(dev)
        ops.unfused_calls.clear()
        with torch.no_grad():
            got, attn = blk(x, fe)
            got_na, none = blk(x, fe, want_attn=False)
        torch.cuda.synchronize()
        assert not ops.unfused_calls, ops.unfused_calls
        assert none is None and torch.equal(got, got_na) and tuple(attn.shape) == (B * heads, S.MODULE_N, k, D // heads)
        with torch.no_grad():
            r64, a64 = ref64(x.double(), fe.double())
            r32, a32 = ref32(x, fe)
        ops.unfused_calls.clear()
        r64, a64 = r64.cpu(), a64.cpu()
        tag = "module D=%d k=%d heads=%d layers=%d B=%d" % (D, k, heads, layers, B)
        r = note(tag + " res", FR.rel_err(got.cpu(), r64), FR.yardstick(r32.cpu(), r64))
        assert r <= R_RATIO, tag
        r = note(tag + " attn", FR.rel_err(_sorted(attn).cpu(), _sorted(a64)), FR.yardstick(_sorted(a32).cpu(), _sorted(a64)))
        assert r <= R_RATIO, tag


@pytest.mark.parametrize("D,k,heads,layers", S.G24_CASES)
def test_module_against_g24(dev, D, k, heads, layers):
    g = np.load(os.path.join(GOLD, "g24_multransformer_shapes.npz"))
    blk = S.g24_seeded_(MulTransformerBlock(S.D_POINTS, D, k, heads, layers), D, k, heads, layers).to(dev).eval()
    xyz, f = S.g24_inputs(D, k, heads, layers)
    ops.unfused_calls.clear()
    with torch.no_grad():
        res, attn = blk(torch.from_numpy(xyz).to(dev), torch.from_numpy(f).to(dev))
    torch.cuda.synchronize()
    assert not ops.unfused_calls, ops.unfused_calls
    tag = S.g24_tag(D, k, heads, layers)
    np.testing.assert_allclose(res[..., ::4].cpu().numpy(), g["res_" + tag], **FR.TOL)
    np.testing.assert_allclose(np.sort(attn[:, ::16, :, ::8].cpu().numpy(), axis=2), np.sort(g["attn_" + tag], axis=2), **FR.TOL)


# ============================================================================================================== tracker
def test_tracker_with_small_blocks_runs_fused(dev):
    from ptt_amd.config import StubDataset, ptt_model_cfg
    from ptt_amd.models import build_network
    model = M.seeded_(build_network(S.tracker_cfg(ptt_model_cfg()), 1, StubDataset()), 2424).to(dev).eval()
    blocks = [m for m in model.modules() if isinstance(m, MulTransformerBlock)]
    assert len(blocks) == 2 and all((b.d_model, b.k, b.heads) == (S.TRACKER_D, S.TRACKER_K, M.TRACKER_HEADS) for b in blocks)
    s, t = synth.frames(2424, 2, 1024, 512)
    batch = lambda: {'search_points': torch.from_numpy(s).to(dev), 'template_points': torch.from_numpy(t).to(dev), 'batch_size': 2}
    ops.unfused_calls.clear()
    with torch.no_grad():
        out = {k: v.clone() for k, v in model(batch()).items() if torch.is_tensor(v)}
    torch.cuda.synchronize()
    assert not ops.unfused_calls, ops.unfused_calls
    for b in blocks:
        b._fusable = lambda *a: False
    with torch.no_grad():
        ref = model(batch())
    ops.unfused_calls.clear()
    for k in ('cosine_feats', 'pred_centroids_cls', 'pred_centroids_votes', 'votes_feats', 'pred_box_center', 'pred_box_data'):
        np.testing.assert_allclose(out[k].cpu().numpy(), ref[k].cpu().numpy(), err_msg=k, **FR.TOL)


# ============================================================================================================= training
class _Forbidden(RuntimeError):
    pass


def _forbid(monkeypatch):
    def boom(*a, **kw):
        raise _Forbidden("a stock torch op of the reference path ran")
    monkeypatch.setattr(torch.nn.functional, "softmax", boom)
    monkeypatch.setattr(torch.nn.functional, "layer_norm", boom)
    monkeypatch.setattr(torch.Tensor, "argsort", boom)


def _train_inputs(D, k, heads, dev, dtype=F32):
    xyz, f = S.module_inputs(D, k, heads, S.TRAIN_B, S.TRAIN_N)
    x = torch.from_numpy(xyz).to(dev).to(dtype).requires_grad_(True)
    fe = torch.from_numpy(f).to(dev).to(dtype).requires_grad_(True)
    w = torch.from_numpy(np.random.RandomState(D + k + heads).standard_normal((S.TRAIN_B, S.TRAIN_N, S.D_POINTS))).to(dev).to(dtype)
    return x, fe, w


def _grads(blk, x, fe):
    return [p.grad for p in blk.parameters()] + [fe.grad, x.grad]


def _stock_layer(layer, xyz, features, knn_idx):
    """MulHeadTransformerLayer.forward's stock op sequence (multitransformer.py:37-63) in the dtype of the layer's parameters, on a
    GIVEN kNN table (B,N,k) int64 instead of its own argsort -> res."""
    H = layer.heads
    knn_xyz = index_points(xyz, knn_idx)
    x = layer.fc1(features)
    B, N, C = x.shape
    query, key, value = layer.w_qs(x), index_points(layer.w_ks(x), knn_idx), index_points(layer.w_vs(x), knn_idx)
    query = query.view(B, N, H, -1).permute(0, 2, 1, 3).flatten(0, 1)
    pos_enc = layer.fc_delta(xyz[:, :, None] - knn_xyz)
    pos_enc, key, value = (t.view(B, N, t.shape[2], H, -1).permute(0, 3, 1, 2, 4).flatten(0, 1) for t in (pos_enc, key, value))
    attn = layer.fc_gamma(query[:, :, None] - key + pos_enc)
    attn = torch.softmax(attn / np.sqrt(key.size(-1)), dim=-2)
    res = (attn * (value + pos_enc)).sum(dim=2)
    if H > 1:
        res = res.permute(0, 2, 1).reshape(B, C, N).permute(0, 2, 1)
    res = layer.norm1(layer.proj(res))
    return layer.norm2(layer.fc2(res)) + features


@pytest.mark.parametrize("D,k,heads,layers", S.TRAIN_CASES)
def test_training_step_on_the_row_kernels(dev, monkeypatch, D, k, heads, layers):
    blk = _block(D, k, heads, layers, dev).train()
    x, fe, w = _train_inputs(D, k, heads, dev)
    assert train_ops.mul_block_usable(blk, x, fe)
    with monkeypatch.context() as mp:
        _forbid(mp)
        res, attn = blk(x, fe)
        (res * w).sum().backward()
        torch.cuda.synchronize()
    assert tuple(attn.shape) == (S.TRAIN_B * heads, S.TRAIN_N, k, D // heads) and not attn.requires_grad
    names = [n for n, _ in blk.named_parameters()] + ["features", "xyz"]
    g_hip = [g.detach().double().cpu() for g in _grads(blk, x, fe)]
    assert all(bool(torch.isfinite(g).all()) for g in g_hip)
    knn = ops.knn(x.detach(), k).long()

    def stock(dtype):
        ref = MulTransformerBlock(S.D_POINTS, D, k, heads, layers).to(dev).to(dtype).train()
        ref.load_state_dict(blk.state_dict())
        xr, fr, wr = _train_inputs(D, k, heads, dev, dtype)
        r = fr
        for layer in ref.layers:
            r = _stock_layer(layer, xr, r, knn)
        (r * wr).sum().backward()
        return r.detach().double().cpu(), [g.detach().double().cpu() for g in _grads(ref, xr, fr)]

    r64, g64 = stock(torch.float64)
    r32, g32 = stock(F32)
    tag = "TRAIN D=%d k=%d heads=%d layers=%d" % (D, k, heads, layers)
    e_ref = float((r32 - r64).norm() / r64.norm())
    e_hip = float((res.detach().double().cpu() - r64).norm() / r64.norm())
    print("\n%s %-28s e_ref %.3e  e_hip %.3e  ratio %.2f" % (tag, "res", e_ref, e_hip, e_hip / e_ref))
    bad = []
    if not e_hip <= R_TRAIN * e_ref:
        bad.append(("res", e_ref, e_hip))
    worst = e_hip / e_ref
    for n, gh, gr, gd in zip(names, g_hip, g32, g64):
        if n.endswith("fc_gamma.2.bias"):
            # a per-channel constant over the neighbours cancels in the softmax: the true gradient is 0, the float64 run gives
            # ~1e-17, both float32 runs rounding noise with no scale to hold a ratio against — absolute, as
            # tests/test_multitransformer_train_gpu.py holds it
            err = float((gh - gd).abs().max())
            print("%s %-28s max |g - g64| %.3e (stock float32 %.3e; atol 1e-4)" % (tag, n, err, float((gr - gd).abs().max())))
            if not err <= 1e-4:
                bad.append((n, err))
            continue
        d = float(gd.norm())
        e_ref, e_hip = float((gr - gd).norm()) / d, float((gh - gd).norm()) / d
        worst = max(worst, e_hip / e_ref)
        print("%s %-28s e_ref %.3e  e_hip %.3e  ratio %.2f" % (tag, n, e_ref, e_hip, e_hip / e_ref))
        if not e_hip <= R_TRAIN * e_ref:
            bad.append((n, e_ref, e_hip))
    print("%s worst ratio %.2f" % (tag, worst))
    RATIOS[tag] = worst
    assert not bad, bad


def test_zz_ratio_report():
    for case in sorted(RATIOS):
        print("WORST %-64s %.2f" % (case, RATIOS[case]))
