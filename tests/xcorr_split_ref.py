"""The split-bf16 arithmetic of ptt_xcorr_split_f32 in plain torch on the CPU (tests/test_xcorr_split_cpu.py,
tests/test_xcorr_split_gpu.py). A plain module: no fixtures, no pytest settings.

The level is CosineSimAug's batched pair MLP at C0 = 256: h0 = relu(P_i + w_sim * cos_ij) with layer 0's BatchNorm folded into P and
w_sim in float32 (what CosineSimAug hands to the kernel; cos and P are float32 operands of the level, formed on the host), then
256 -> 256 (ReLU) -> 256 with the BatchNorm scale folded into the weights in float32 — the values the kernel's pack sees — in
tests/sa_split_ref._lin's two-piece arithmetic (hi.hi + hi.lo + lo.hi), then shift, the max over the template points and the ReLU.

    split64   the arithmetic itself: everything in float64 (the bf16 pieces are exact in it)
    split32   its float32 run; Y = max(e32, 4u) of split32 against split64 is the yardstick of the GPU test
    exact64   no split: the same level with plain float64 products
    drop64    split64 without the a_lo . w_hi term (what a kernel that forgot a cross term computes)
    plain32   float32 without the split (what an fp32 kernel computes)

Generic cases: tests/fused_ref.xcorr_case(B, Ns, Nt, XCORR_F, (256, 256, 256)) at GENERIC — one chunk, three chunks with an all-zero
template row, two chunks: the smallest launches that still cross a chunk boundary and a cloud boundary. Planted cases: PLANTED's
shapes with operands that split exactly (planted_case)."""
import functools

import numpy as np
import torch

from tests import fused_ref as FR
from tests.pair_split_ref import split2                                   # noqa: F401  (re-exported for the tests)
from tests.sa_split_ref import _folded, _lin, _planted_values

GENERIC = ((1, 1, 64), (3, 5, 192), (2, 3, 128))
PLANTED = ((1, 1, 64), (3, 5, 192))
PLANTED_SEED = 7
WIDTHS = (256, 256, 256)


def level(p, dtype, mode="split", relu2=True, shifts=True):
    """The level of parameter set `p` in `dtype` -> (B, 256, Ns). shifts=False: both shifts absent (NULL for the kernel)."""
    c = lambda t: t.to(dtype)
    h0 = torch.relu(c(p.P)[:, None, :, :] + c(p.cos)[..., None] * c(p.w_sim))                 # (B,Ns,Nt,256)
    y1 = _lin(h0, p.W1, mode)
    h1 = torch.relu(y1 + c(p.sh1) if shifts else y1)
    y2 = _lin(h1, p.W2, mode)
    y2 = (y2 + c(p.sh2) if shifts else y2).max(dim=2)[0]                                       # (B,Ns,256)
    if relu2:
        y2 = torch.relu(y2)
    return y2.transpose(1, 2).contiguous()


@functools.lru_cache(maxsize=None)
def inputs(B, Ns, Nt):
    """The operands of a generic case, float32: what the module would hand to the kernel (packs aside)."""
    c = FR.xcorr_case(B, Ns, Nt, FR.XCORR_F, WIDTHS)
    L0 = c.layers[0]
    w0 = L0["conv_weight"].reshape(256, -1)                                          # (256, 1 + 3 + f)
    s0 = L0["bn_weight"] / torch.sqrt(L0["bn_var"] + L0["eps"])
    t0 = L0["bn_bias"] - L0["bn_mean"] * s0
    rows = torch.cat((c.txyz, c.tf.transpose(1, 2)), dim=2)                         # (B,Nt,3+f)
    P = (torch.nn.functional.linear(rows, w0[:, 1:]) * s0 + t0).contiguous()
    W1, sh1 = _folded(c.layers[1])
    W2, sh2 = _folded(c.layers[2])
    return FR.Case(name="(%d,%d,%d)" % (B, Ns, Nt), B=B, Ns=Ns, Nt=Nt, cos=c.sim32.transpose(1, 2).contiguous(), P=P,
                   w_sim=(w0[:, 0] * s0).contiguous(), W1=W1, sh1=sh1, W2=W2, sh2=sh2)


@functools.lru_cache(maxsize=None)
def generic_case(B, Ns, Nt, relu2=True, shifts=True):
    p = inputs(B, Ns, Nt)
    kw = dict(relu2=relu2, shifts=shifts)
    s64, s32 = level(p, torch.float64, **kw), level(p, torch.float32, **kw)
    return FR.Case(p=p, split64=s64, split32=s32, exact64=level(p, torch.float64, "exact", **kw),
                   plain32=level(p, torch.float32, "exact", **kw), Y=FR.yardstick(s32, s64), **kw)


@functools.lru_cache(maxsize=None)
def planted_case(B, Ns, Nt, seed=PLANTED_SEED):
    """Operands that split exactly, all positive: w_sim = 0 (the cosines drop out), both shifts zero, all ReLUs on. Layer 1's
    dropped lo . lo terms then all have one sign, so exact64 >= split64."""
    rs = np.random.RandomState(seed)
    P = _planted_values(rs, (B, Nt, 256), -2, 1)
    W1 = _planted_values(rs, (256, 256), -7, -5)
    W2 = _planted_values(rs, (256, 256), -7, -5)
    p = FR.Case(name="planted (%d,%d,%d)" % (B, Ns, Nt), B=B, Ns=Ns, Nt=Nt, cos=torch.zeros(B, Ns, Nt), P=P, w_sim=torch.zeros(256),
                W1=W1, sh1=torch.zeros(256), W2=W2, sh2=torch.zeros(256))
    s64, s32 = level(p, torch.float64), level(p, torch.float32)
    return FR.Case(p=p, split64=s64, split32=s32, exact64=level(p, torch.float64, "exact"), plain32=level(p, torch.float32, "exact"),
                   drop64=level(p, torch.float64, "drop"), Y=FR.yardstick(s32, s64))
