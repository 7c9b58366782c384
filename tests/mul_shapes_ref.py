"""Cases for MulTransformerBlock at DIM_MODEL 128 / 256 x KNN 8 / 16 / 32 (tests/test_mul_shapes_cpu.py,
tests/test_mul_shapes_gpu.py, fixture G24). A plain module: no fixtures, no pytest settings, importable on the CPU.

The envelope: heads 1 / 2 / 4 / 8 with hd = d_model / heads >= 32 (one 32-column MFMA tile), i.e. heads 1, 2, 4 at 128 and
1, 2, 4, 8 at 256. Kernel-level cases are built as tests/fused_ref.pair_case builds the shipped multi-head shape: the clouds of
tests/pair_shapes_ref.CLOUDS (distinct points, the k-th neighbour never tied), nn.Linear's init range for the case's own D and hd,
q | k | v rows formed in float32 on the host, the kNN table of the float32 oracle, fused_ref.heads_attention in float32 and
float64 on that table."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import index_ops as O
from ptt_amd import synth
from tests import fused_ref as FR
from tests import multitransformer_ref as M
from tests import pair_shapes_ref as S
from tests.util import transformer_params

D_POINTS = S.D_POINTS
# every new (D, heads): hd >= 32
D_HEADS = [(128, 1), (128, 2), (128, 4), (256, 1), (256, 2), (256, 4), (256, 8)]
KNNS = (8, 16, 32)
# kernel level: the multi-head kernel's 15 new instantiations (heads = 1 is pt_attn_pair_kernel<D, k>: tests/test_pair_shapes_gpu.py)
KERNEL_SHAPES = [(D, H, k) for D, H in D_HEADS if H > 1 for k in KNNS]
KERNEL_CASES = [(D, H, k, B, N) for D, H, k in KERNEL_SHAPES for B, N in S.CLOUDS[k]]
# (B, N, k, D, heads) the C entry point refuses: hd 16; a head count that is not instantiated (16; 3); the tile rule at k = 8; D 384
REFUSED = {"D128_heads8": (1, 32, 16, 128, 8), "D256_heads16": (1, 32, 16, 256, 16), "D256_heads3": (1, 32, 16, 256, 3),
           "D256_heads2_k8_N10": (1, 10, 8, 256, 2), "D384_heads2": (1, 32, 16, 384, 2)}


@functools.lru_cache(maxsize=None)
def kernel_case(D, heads, k, B, N):
    rs = np.random.RandomState(11 * D + 5 * heads + k + N)
    P = dict(transformer_params(D + heads + k + N, D_POINTS, D))
    P.update(FR.gamma_params(D + k + N + heads, D // heads))
    s = S.cloud(k, B, N)
    xyz = torch.from_numpy(s)
    feats = torch.from_numpy(rs.standard_normal((B, N, D_POINTS)).astype(np.float32))
    knn = torch.from_numpy(O.knn(s, k))
    x = F.linear(feats, P["fc1.weight"], P["fc1.bias"])
    qkv = F.linear(x, torch.cat([P["w_qs.weight"], P["w_ks.weight"], P["w_vs.weight"]], 0))          # float32
    res32, attn32 = FR.heads_attention(xyz, qkv, knn, P, heads)
    res64, attn64 = FR.heads_attention(xyz.double(), qkv.double(), knn, {n: v.double() for n, v in P.items()}, heads)
    return FR.Case(D=D, heads=heads, k=k, B=B, N=N, P=P, xyz=xyz, qkv=qkv, knn=knn, res32=res32, attn32=attn32, res64=res64,
                   attn64=attn64, Y_res=FR.yardstick(res32, res64), Y_attn=FR.yardstick(attn32, attn64))


# ------------------------------------------------------------------------------------------------------------- module level
# every new (D, heads) at one k each, all three k; one 2-layer block
MODULE_CASES = [(128, 8, 1, 1), (128, 16, 2, 1), (128, 32, 4, 1), (256, 32, 1, 1), (256, 8, 2, 1), (256, 16, 4, 1), (256, 32, 8, 1),
                (256, 8, 4, 2)]                 # (D, k, heads, layers)
MODULE_N, MODULE_BATCHES = S.MODULE_N, S.MODULE_BATCHES           # 48 x 40 and 1 x 40 points
TRAIN_CASES = [(256, 8, 4, 1), (256, 16, 2, 2), (128, 32, 2, 1)]
TRAIN_B, TRAIN_N = S.TRAIN_B, S.TRAIN_N
TRACKER_D, TRACKER_K = 256, 8


def module_seed(D, k, heads, layers):
    return 2400 + D + k + 10 * heads + layers


def module_inputs(D, k, heads, B, N=MODULE_N):
    """(xyz (B,N,3), features (B,N,256)) float32 arrays: distinct points, no tie at any rank. The seed base is one at which every
    k-th-neighbour gap of the module and training cases is >= 1.5e-5 relative (tests/test_mul_shapes_cpu.py holds 2e-6; the bases
    5000 and 5100 gave a case with 1.7e-6 and 2.0e-6)."""
    seed = 5200 + D + k + 7 * heads + B
    xyz, _ = synth.frames(seed, B, N, 64, K_s=N)
    f = np.random.RandomState(seed + 1).standard_normal((B, N, D_POINTS)).astype(np.float32)
    return xyz, f


def tracker_cfg(cfg):
    """multitransformer_ref.tracker_cfg with DIM_MODEL 256 and KNN 8 in both blocks."""
    cfg = M.tracker_cfg(cfg)
    for head in ("CENTROID_HEAD", "BOX_HEAD"):
        tb = cfg[head]["TRANSFORMER_BLOCK"]
        tb["DIM_MODEL"], tb["KNN"] = TRACKER_D, TRACKER_K
    return cfg


# ------------------------------------------------------------------------------------------------------------- fixture G24
G24_CASES = [(256, 8, 4, 2), (128, 32, 2, 1), (256, 16, 8, 1)]       # (D, k, heads, layers)
G24_B, G24_N = 2, 64


def g24_tag(D, k, heads, layers):
    return "d%d_k%d_h%d_l%d" % (D, k, heads, layers)


def g24_seed(D, k, heads, layers):
    return 24000 + D + k + 10 * heads + layers


def g24_inputs(D, k, heads, layers):
    """The one (xyz (2,64,3), features (2,64,256)) batch of fixture G24: a function of nothing but the fixture."""
    xyz, _ = synth.frames(2424, G24_B, G24_N, 64, K_s=G24_N)
    f = np.random.RandomState(2425).standard_normal((G24_B, G24_N, D_POINTS)).astype(np.float32)
    return xyz, f


def g24_seeded_(block, D, k, heads, layers):
    """Seeded weights, LayerNorm affine included (multitransformer_ref.seeded_)."""
    return M.seeded_(block, g24_seed(D, k, heads, layers))
