"""The split-bf16 arithmetic of ptt_pt_attn_pair_split_f32 in plain torch on the CPU (tests/test_pair_split_cpu.py,
tests/test_pair_split_gpu.py). A plain module: no fixtures, no pytest settings.

Every fp32 operand x of the block's three in-kernel GEMMs (fc_delta[2], fc_gamma[0], fc_gamma[2]) is two bf16 pieces,
hi = bf16(x) rounded to nearest even and lo = bf16(x - float(hi)); a product is hi.hi + hi.lo + lo.hi. Every other step is
oracle.dense_ref.transformer_block's, on the kNN table of the cases tests/fused_ref.pair_case and tests/pair_shapes_ref build.
"split64": the three products and everything else in float64 (the pieces are exact in it); "split32" the same in float32 — its
distance from split64 is the yardstick Y of the GPU test, as tests/fused_ref.yardstick is for the fp32 kernels."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import dense_ref as R
from tests import fused_ref as FR
from tests import pair_shapes_ref as S

ALL_PAIRS = [(D, k) for D in (128, 256, 512) for k in (8, 16, 32)]
CASES = [(D, k, B, N) for D, k in ALL_PAIRS for B, N in S.CLOUDS[k]]


def split2(x):
    """-> (hi, lo) of the float32 value of x, as float64 tensors: hi = bf16(x) (round to nearest even), lo = bf16(x - hi)."""
    x32 = x.float()
    hi = x32.bfloat16().float()
    lo = (x32 - hi).bfloat16().float()
    return hi.double(), lo.double()


def linear_split(layer, x):
    """layer = (weight, bias | None); x of any float dtype. The three products and the bias in the dtype of x: float64 is the
    arithmetic itself, float32 the "float32 run"."""
    w, b = layer
    hx, lx = (t.to(x.dtype) for t in split2(x))
    hw, lw = (t.to(x.dtype) for t in split2(w))
    y = hx @ hw.t() + hx @ lw.t() + lx @ hw.t()
    return y if b is None else y + b.to(x.dtype)


def block(xyz, features, P, k, knn_idx, split):
    """dense_ref.transformer_block in the dtype of its inputs on a given kNN table; split: the three in-kernel GEMMs in two-piece
    arithmetic -> (res through fc2 + residual, attn, res before fc2)."""
    lin = (lambda wb, x: linear_split(wb, x)) if split else (lambda wb, x: F.linear(x, wb[0], wb[1]))
    knn_xyz = R.index_points(xyz, knn_idx)
    x = F.linear(features, P["fc1.weight"], P["fc1.bias"])
    q = F.linear(x, P["w_qs.weight"])
    kk = R.index_points(F.linear(x, P["w_ks.weight"]), knn_idx)
    v = R.index_points(F.linear(x, P["w_vs.weight"]), knn_idx)
    d = xyz[:, :, None] - knn_xyz
    h = F.relu(F.linear(d, P["fc_delta.0.weight"], P["fc_delta.0.bias"]))
    pos_enc = lin((P["fc_delta.2.weight"], P["fc_delta.2.bias"]), h)
    a = q[:, :, None] - kk + pos_enc
    g = F.relu(lin((P["fc_gamma.0.weight"], P["fc_gamma.0.bias"]), a))
    a = lin((P["fc_gamma.2.weight"], P["fc_gamma.2.bias"]), g)
    attn = F.softmax(a / np.sqrt(kk.size(-1)), dim=-2)
    pre = (attn * (v + pos_enc)).sum(dim=2)
    res = F.linear(pre, P["fc2.weight"], P["fc2.bias"]) + features
    return res, attn, pre


def _double(P):
    return {n: v.double() for n, v in P.items()}


@functools.lru_cache(maxsize=None)
def pair_case_split(B, N, D, k):
    """The case tests/fused_ref.pair_case (at (512, 16)) or tests/pair_shapes_ref.pair_case (elsewhere) builds, with the three
    in-kernel GEMMs replaced. res64 / attn64 / pre64: the split arithmetic in float64; res32 / attn32: its float32 run;
    exact_res64 / exact_pre64: the block without the split in float64; Y_*: max(e32, 4u) of the float32 run."""
    base = FR.pair_case(B, N, 1) if (D, k) == (FR.D_MODEL, FR.KNN) else S.pair_case(D, k, B, N)
    P, xyz, feats, knn = base.P, base.xyz, base.feats, base.knn.long()
    res32, attn32, pre32 = block(xyz, feats, P, k, knn, True)
    res64, attn64, pre64 = block(xyz.double(), feats.double(), _double(P), k, knn, True)
    ex_res, _, ex_pre = block(xyz.double(), feats.double(), _double(P), k, knn, False)
    return FR.Case(D=D, k=k, B=B, N=N, P=P, xyz=xyz, feats=feats, knn=base.knn, res32=res32, attn32=attn32, pre32=pre32,
                   res64=res64, attn64=attn64, pre64=pre64, exact_res64=ex_res, exact_pre64=ex_pre,
                   Y_res=FR.yardstick(res32, res64), Y_attn=FR.yardstick(attn32, attn64), Y_pre=FR.yardstick(pre32, pre64))


# ------------------------------------------------------------------------------------------------- the split pack's order
def bf16_rne_np(x):
    """bf16 bits (uint16) of a float32 array, round to nearest even, on the bits."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def split_pack_np(w):
    """include/ptt_hip.h, "Split pack of a (Cout, K) fp32 weight", restated: element
        e = (((kb * NT + ct) * 2 + piece) * 64 + lane) * 8 + j,   NT = Cout / 32
    holds piece `piece` (0 = hi, 1 = lo) of W[32 * ct + (lane & 31)][16 * kb + 8 * (lane >> 5) + j] -> uint16 (2 * Cout * K,)."""
    w = np.ascontiguousarray(w, dtype=np.float32)
    Cout, K = w.shape
    assert Cout % 32 == 0 and K % 16 == 0
    NT = Cout // 32
    hi = bf16_rne_np(w)
    hif = (hi.astype(np.uint32) << 16).view(np.float32)
    lo = bf16_rne_np(w - hif)
    e = np.arange(2 * Cout * K, dtype=np.int64)
    j, lane, piece, tile = e & 7, (e >> 3) & 63, (e >> 9) & 1, e >> 10
    ct, kb = tile % NT, tile // NT
    col, kk = 32 * ct + (lane & 31), 16 * kb + 8 * (lane >> 5) + j
    return np.where(piece == 0, hi[col, kk], lo[col, kk]).astype(np.uint16)
