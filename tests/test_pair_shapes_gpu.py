"""ptt_pt_attn_pair_f32 and TransformerBlock at DIM_MODEL 128 / 256 / 512 x KNN 8 / 16 / 32 — the eight pairs beside the shipped
(512, 16), which tests/test_fused_guard_gpu.py holds to the same bars (cases, seeds and references: tests/pair_shapes_ref.py).

Kernel level, per (D, k) and cloud — k = 8: (1,8), (3,12), (1,52); k = 16: (1,16), (3,18), (1,50); k = 32: (1,32), (3,33), (1,70):
the device kNN table equals oracle.index_ops.knn; with every operand embed()-ded between NaN / INDEX_FILL words and guarded outputs,
  (a) err / Y <= 4 for res (through fc2 + residual) and attn, Y = max(e32, 4u) the float32 oracle's own distance from its float64
      run on the same table (fused_ref.yardstick);  (b) assert_allclose against the float32 oracle at FR.TOL;
  (c) the same bits with rel on / off, order = ops.spatial_order(xyz) / NULL, attn on / off (res), and on a second run;
  (d) guard words intact, inputs untouched.
Refusals (PTT_EUNSUPPORTED, outputs untouched): k = 8 with N = 10; k = 32 with N = 31; D = 384; k = 4; heads = 2 with k = 8.

Module level: TransformerBlock(256, D, k).eval() under no_grad on 48 x 40 and 1 x 40 points takes the fused path
(ops.unfused_calls stays empty — the test that fails without the instantiations) and lies within 4 Y of the float64 stock path of
the same module, attn compared as per-point sorted sets; the eval-mode module against fixture G23 (the reference's own block at
(256, 8), (128, 32), (512, 32)) at FR.TOL. Training: pt_block_usable holds for k = 8 / 32, a step runs with the stock op sequence
forbidden, and every gradient lies within R_TRAIN x the stock float32 sequence's own distance from a float64 run on the same table.

err / Y measured on an MI355X (res / attn, worst over rel and order on / off — the runs agree bit for bit):
  (D, k)      N = k          3 clouds       many tiles
  (128,  8)   0.32 / 0.69    0.29 / 0.79    0.19 / 0.84
  (128, 16)   0.42 / 0.94    0.34 / 0.87    0.23 / 0.93
  (128, 32)   0.41 / 0.75    0.36 / 0.75    0.26 / 0.74
  (256,  8)   0.26 / 0.84    0.23 / 0.89    0.25 / 0.87
  (256, 16)   0.25 / 0.94    0.23 / 0.91    0.18 / 0.92
  (256, 32)   0.26 / 0.81    0.27 / 0.76    0.25 / 0.72
  (512,  8)   0.34 / 0.97    0.31 / 0.90    0.18 / 0.90
  (512, 32)   0.33 / 0.85    0.30 / 0.71    0.24 / 0.79
No case came near the bar of 4; none needed investigation.
Module level, worst over the 48-frame and the 1-frame batch (res / attn):
  (128, 8) 0.22 / 0.89   (128, 16) 0.30 / 0.88   (128, 32) 0.29 / 0.78
  (256, 8) 0.19 / 0.95   (256, 16) 0.15 / 0.93   (256, 32) 0.24 / 0.78
  (512, 8) 0.22 / 0.97   (512, 32) 0.35 / 0.73
Training, e_hip / e_ref per gradient (worst over parameters, features, xyz), B = 2, N = 40:
  (256, 8):  2.94 (fc_gamma.0.bias: e_ref 7.4e-7, e_hip 2.2e-6), then 1.92 (fc_delta.0.bias), 1.27 (fc2.bias); every weight,
             features and xyz 0.63 - 1.00; res 1.01
  (512, 32): 1.13 (fc2.bias); every other gradient below 1 — at this size the stock float32 GEMMs themselves lie 5e-4 - 1e-3 from
             float64 for fc_gamma.0 / w_qs / w_ks (e_hip 7e-7 - 2e-6 there); res 1.01
R_TRAIN = twice the worst ratio (2.94), rounded up to one significant digit = 6, and R_TRAIN <= 8 is asserted.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from ptt_amd import ops, train_ops
from ptt_amd.models.transformer_block.variants import TransformerBlock
from tests import fused_ref as FR
from tests import guard
from tests import pair_shapes_ref as S
from tests.guard import check_guard, embed, guarded

pytestmark = pytest.mark.gpu
F32, I32 = torch.float32, torch.int32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

R_RATIO = 4.0               # the bar tests/test_fused_guard_gpu.py holds the shipped shape to
R_TRAIN = 6.0               # twice the worst measured e_hip / e_ref (2.94, table above), one significant digit
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
    print("RATIO %-52s err %.3e  Y %.3e  err/Y %.2f" % (case, err, Y, r))
    return r


def bound(case, got, ref64, ref32, Y):
    r = note(case, FR.rel_err(got, ref64), Y)
    assert r <= R_RATIO, "%s: %.2f x the float32 oracle's own distance from float64 (R = %g)" % (case, r, R_RATIO)
    np.testing.assert_allclose(got.numpy(), ref32.numpy(), **FR.TOL)


def bits(t):
    return t.contiguous().view(I32)


def same_bits(a, b, what):
    assert a.shape == b.shape and torch.equal(bits(a), bits(b)), "%s: not the same bits" % what


def _desc(xyz, knn, qkv, w, res, attn, B, N, k, D, heads=1, rel=None, order=None):
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
    B, N, D, k = c.B, c.N, c.D, c.k
    res = guarded((B, N, D), F32, device=dev)
    attn = guarded((B, N * k, D), F32, device=dev) if want_attn else None
    d = _desc(xyz_e, knn_e, qkv_e, w, res, attn, B, N, k, D, 1, rel, order)
    guard.launch("ptt_pt_attn_pair_f32", dev, ctypes.byref(d))
    torch.cuda.synchronize()
    check_guard(res)
    if attn is not None:
        check_guard(attn)
    for v in ins + [v for v in (rel, order) if v is not None]:
        check_guard(v, all_written=False)
    return res, attn


@pytest.mark.parametrize("D,k,B,N", S.CASES)
def test_pair(dev, D, k, B, N):
    c = S.pair_case(D, k, B, N)
    P = c.P
    dv = lambda n: P[n].to(dev).contiguous()
    ins = []
    keep = lambda v: (ins.append(v), v)[1]
    xyz_d = c.xyz.to(dev)
    knn_d, rel_d = ops.knn(xyz_d, k, want_rel=True)
    assert torch.equal(knn_d.cpu(), c.knn), "the device kNN table is not the oracle's"
    order_d = ops.spatial_order(xyz_d)
    assert torch.equal(order_d.view(B, N).sort(dim=1)[0].cpu(), (torch.arange(B * N, dtype=I32).view(B, N)))    # a permutation inside clouds
    x = ops.linear(c.feats.to(dev), ops.pack_weight(dv("fc1.weight")), D, None, dv("fc1.bias"))
    wqkv = torch.cat([P["w_qs.weight"], P["w_ks.weight"], P["w_vs.weight"]], 0).to(dev)
    qkv = ops.linear(x, ops.pack_weight(wqkv), 3 * D)
    w = dict(Wd1p=ops.pack_delta0(dv("fc_delta.0.weight"), dv("fc_delta.0.bias")), Wd2p=ops.pack_weight(dv("fc_delta.2.weight")),
             bd2=dv("fc_delta.2.bias"), Wg1p=ops.pack_weight(dv("fc_gamma.0.weight")), bg1=dv("fc_gamma.0.bias"),
             Wg2p=ops.pack_weight(dv("fc_gamma.2.weight")), bg2=dv("fc_gamma.2.bias"))
    w = {n: keep(embed(t)) for n, t in w.items()}
    qkv_e, xyz_e, knn_e = keep(embed(qkv.contiguous())), keep(embed(xyz_d)), keep(embed(knn_d))
    rel_e, order_e = embed(rel_d.view(B, N * k, 3).contiguous()), embed(order_d.view(B, N).contiguous())
    name = "pair D=%d k=%d (%d,%d)" % (D, k, B, N)
    fc2 = ops.pack_weight(dv("fc2.weight"))

    def results(res, attn):      # the block's output: fc2 + residual on the linear kernel, as tests/test_dense_gpu.py chains it
        out = ops.linear(res, fc2, S.D_POINTS, None, dv("fc2.bias"), False, c.feats.to(dev))
        return out.cpu(), (attn.view(B, N, k, D).cpu() if attn is not None else None)

    first = None
    for use_rel in (False, True):
        for use_order in (False, True):
            tag = "%s rel=%d order=%d" % (name, use_rel, use_order)
            rel, order = rel_e if use_rel else None, order_e if use_order else None
            res, attn = pair_run(dev, c, w, qkv_e, xyz_e, knn_e, ins, rel, order, True)
            out_h, attn_h = results(res, attn)
            bound(tag + " res", out_h, c.res64, c.res32, c.Y_res)
            bound(tag + " attn", attn_h, c.attn64, c.attn32, c.Y_attn)
            res_bits = res.cpu().contiguous()
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


# ============================================================================================================= refusals
def _rand(dev, *shape):
    return torch.from_numpy(np.random.RandomState(sum(shape)).standard_normal(shape).astype(np.float32)).to(dev)


REFUSED = {"k8_N10": (1, 10, 8, 256, 1), "k32_N31": (1, 31, 32, 256, 1), "D384": (1, 32, 16, 384, 1), "k4": (1, 32, 4, 256, 1),
           "heads2_k8": (1, 32, 8, 512, 2)}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_refusal(dev, what):
    """Every array has the size the refused shape would need: were the launch not refused, it would run inside its buffers."""
    B, N, k, D, heads = REFUSED[what]
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
def _module(D, k, dev, seed):
    torch.manual_seed(seed)
    return TransformerBlock(S.D_POINTS, D, k).to(dev)


def _copy64(blk, D, k, dev):
    ref = TransformerBlock(S.D_POINTS, D, k).to(dev).double()
    ref.load_state_dict(blk.state_dict())
    return ref


@pytest.mark.parametrize("D,k", S.PAIRS)
def test_module_eval_takes_the_fused_path(dev, D, k):
    blk = _module(D, k, dev, 10 * D + k).eval()
    ref64 = _copy64(blk, D, k, dev).eval()
    for B in S.MODULE_BATCHES:
        xyz, f = S.module_inputs(D, k, B)
        x, fe = torch.from_numpy(xyz).to(dev), torch.from_numpy(f).to(dev)
        ops.unfused_calls.clear()
        with torch.no_grad():
            got, attn = blk(x, fe)
            got_na, none = blk(x, fe, want_attn=False)
        torch.cuda.synchronize()
        assert not ops.unfused_calls, ops.unfused_calls
        assert none is None and torch.equal(got, got_na) and tuple(attn.shape) == (B, S.MODULE_N, k, D)
        knn = ops.knn(x, k).long()
        with torch.no_grad():
            # the stock op sequence of the same module in float64 and in float32 — the latter's distance is the yardstick
            r64, a64 = S.block_forward(ref64, x.double(), fe.double(), knn)
            r32, a32 = S.block_forward(blk, x, fe, knn)
            # and the module's own stock path in float64 (its own argsort): the same neighbour sets, so the same result
            ref64._fusable = lambda *a: False
            r64_own, a64_own = ref64(x.double(), fe.double())
        r64, a64, r64_own, a64_own = r64.cpu(), a64.cpu(), r64_own.cpu(), a64_own.cpu()
        assert float((r64 - r64_own).abs().max()) <= 1e-12 * float(r64.abs().max())
        srt = lambda a: a.sort(dim=2)[0]            # a point's attention values as a set over its k neighbours (per channel)
        assert float((srt(a64) - srt(a64_own)).abs().max()) <= 1e-12
        tag = "module D=%d k=%d B=%d" % (D, k, B)
        r = note(tag + " res", FR.rel_err(got, r64), FR.yardstick(r32.cpu(), r64))
        assert r <= R_RATIO, tag
        r = note(tag + " attn", FR.rel_err(srt(attn), srt(a64)), FR.yardstick(srt(a32).cpu(), srt(a64)))
        assert r <= R_RATIO, tag
    ops.unfused_calls.clear()


@pytest.mark.parametrize("D,k", S.G23_PAIRS)
def test_module_against_g23(dev, D, k):
    g = np.load(os.path.join(GOLD, "g23_transformer_shapes.npz"))
    blk = S.g23_seeded_(TransformerBlock(S.D_POINTS, D, k), D, k).to(dev).eval()
    xyz, f = S.g23_inputs(D, k)
    ops.unfused_calls.clear()
    with torch.no_grad():
        res, attn = blk(torch.from_numpy(xyz).to(dev), torch.from_numpy(f).to(dev))
    torch.cuda.synchronize()
    assert not ops.unfused_calls, ops.unfused_calls
    tag = "d%d_k%d" % (D, k)
    np.testing.assert_allclose(res[..., ::4].cpu().numpy(), g["res_" + tag], **FR.TOL)
    np.testing.assert_allclose(np.sort(attn[:, ::16, :, ::8].cpu().numpy(), axis=2), np.sort(g["attn_" + tag], axis=2), **FR.TOL)


# ============================================================================================================= training
class _Forbidden(RuntimeError):
    pass


def _forbid(monkeypatch):
    def boom(*a, **kw):
        raise _Forbidden("a stock torch op of the reference path ran")
    monkeypatch.setattr(torch.nn.functional, "softmax", boom)
    monkeypatch.setattr(torch.Tensor, "argsort", boom)


def _train_inputs(D, k, dev, dtype=F32):
    xyz, f = S.module_inputs(D, k, S.TRAIN_B, S.TRAIN_N)
    x = torch.from_numpy(xyz).to(dev).to(dtype).requires_grad_(True)
    fe = torch.from_numpy(f).to(dev).to(dtype).requires_grad_(True)
    w = torch.from_numpy(np.random.RandomState(D + k).standard_normal((S.TRAIN_B, S.TRAIN_N, S.D_POINTS))).to(dev).to(dtype)
    return x, fe, w


def _grads(blk, x, fe):
    return [p.grad for p in blk.parameters()] + [fe.grad, x.grad]


@pytest.mark.parametrize("D,k", S.TRAIN_PAIRS)
def test_training_step_on_the_row_kernels(dev, monkeypatch, D, k):
    blk = _module(D, k, dev, 20 * D + k).train()
    x, fe, w = _train_inputs(D, k, dev)
    assert train_ops.pt_block_usable(blk, x, fe)
    with monkeypatch.context() as mp:
        _forbid(mp)
        res, attn = blk(x, fe)
        (res * w).sum().backward()
        torch.cuda.synchronize()
    assert tuple(attn.shape) == (S.TRAIN_B, S.TRAIN_N, k, D) and not attn.requires_grad
    names = [n for n, _ in blk.named_parameters()] + ["features", "xyz"]
    g_hip = [g.detach().double().cpu() for g in _grads(blk, x, fe)]
    assert all(bool(torch.isfinite(g).all()) for g in g_hip)
    knn = ops.knn(x.detach(), k).long()

    def stock(dtype):
        ref = TransformerBlock(S.D_POINTS, D, k).to(dev).to(dtype).train()
        ref.load_state_dict(blk.state_dict())
        xr, fr, wr = _train_inputs(D, k, dev, dtype)
        r, _ = S.block_forward(ref, xr, fr, knn)
        (r * wr).sum().backward()
        return r.detach().double().cpu(), [g.detach().double().cpu() for g in _grads(ref, xr, fr)]

    r64, g64 = stock(torch.float64)
    r32, g32 = stock(F32)
    e_ref = float((r32 - r64).norm() / r64.norm())
    e_hip = float((res.detach().double().cpu() - r64).norm() / r64.norm())
    print("\nTRAIN D=%d k=%d %-20s e_ref %.3e  e_hip %.3e  ratio %.2f" % (D, k, "res", e_ref, e_hip, e_hip / e_ref))
    bad = []
    if not e_hip <= R_TRAIN * e_ref:
        bad.append(("res", e_ref, e_hip))
    worst = 0.0
    for n, gh, gr, gd in zip(names, g_hip, g32, g64):
        if n == "fc_gamma.2.bias":
            # a per-channel constant over the neighbours cancels in the softmax: the true gradient is 0, the float64 run gives
            # ~1e-17, both float32 runs rounding noise with no scale to hold a ratio against — absolute, as
            # tests/test_multitransformer_train_gpu.py holds it
            err = float((gh - gd).abs().max())
            print("TRAIN D=%d k=%d %-20s max |g - g64| %.3e (stock float32 %.3e; atol 1e-4)" % (D, k, n, err, float((gr - gd).abs().max())))
            if not err <= 1e-4:
                bad.append((n, err))
            continue
        d = float(gd.norm())
        e_ref, e_hip = float((gr - gd).norm()) / d, float((gh - gd).norm()) / d
        worst = max(worst, e_hip / e_ref)
        print("TRAIN D=%d k=%d %-20s e_ref %.3e  e_hip %.3e  ratio %.2f" % (D, k, n, e_ref, e_hip, e_hip / e_ref))
        if not e_hip <= R_TRAIN * e_ref:
            bad.append((n, e_ref, e_hip))
    print("TRAIN D=%d k=%d worst gradient ratio %.2f" % (D, k, worst))
    RATIOS["train D=%d k=%d" % (D, k)] = worst
    assert not bad, bad


def test_zz_ratio_report():
    for case in sorted(RATIOS):
        print("WORST %-56s %.2f" % (case, RATIOS[case]))
