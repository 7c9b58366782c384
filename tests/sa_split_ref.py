"""The split-bf16 arithmetic of ptt_sa_stream_split_f32 in plain torch on the CPU (tests/test_sa_split_cpu.py,
tests/test_sa_split_gpu.py). A plain module: no fixtures, no pytest settings.

The level is the dense SA1 / SA2 stream shape on a fixed index table: a hoisted 128-channel layer 0, h0 = act(term[idx] + Wx . rel)
formed as PointnetSAModuleVotes forms it (the BatchNorm scale folded into both halves of layer 0 in float32, the shift inside the
per-point term), then 128 -> 128 (ReLU) -> 256 with the BatchNorm scale folded into the weights in float32 — the values the
kernel's pack sees — and tests/pair_split_ref.linear_split's two-piece arithmetic (hi.hi + hi.lo + lo.hi), then shift, ReLU and
the max over the 32 neighbours.

    split64   the arithmetic itself: everything in float64 (the bf16 pieces are exact in it)
    split32   its float32 run; Y = max(e32, 4u) of split32 against split64 is the yardstick of the GPU test
    exact64   no split: the same level with plain float64 products
    drop64    split64 without the a_lo . w_hi term (what a kernel that forgot a cross term computes)
    plain32   float32 without the split (what an fp32 kernel computes)

Generic cases: tests/fused_ref.sa_case("stream_33" / "stream_1027" / "stream_1029"), imported, not edited. Planted cases: the
index tables of stream_33 and stream_1027 with operands that split exactly (planted_case)."""
import functools

import numpy as np
import torch

from tests import fused_ref as FR
from tests.pair_split_ref import split2

GENERIC = ("stream_33", "stream_1027", "stream_1029")
PLANTED = ("stream_33", "stream_1027")
PLANTED_SEED = 7


def _lin(x, w, mode):
    """x (..., K) . w (Cout, K)^T in the dtype of x. mode: 'split' hi.hi + hi.lo + lo.hi, 'drop' without lo.hi, 'exact' plain."""
    if mode == "exact":
        return x @ w.to(x.dtype).t()
    hx, lx = (t.to(x.dtype) for t in split2(x))
    hw, lw = (t.to(x.dtype) for t in split2(w))
    y = hx @ hw.t() + hx @ lw.t()
    return y if mode == "drop" else y + lx @ hw.t()


def level(p, dtype, mode="split", normalize_xyz=None, l0_relu=None, relu2=None):
    """The level of parameter set `p` (inputs()) in `dtype` -> (B, 256, M). The three flags default to the set's own."""
    normalize_xyz = p.normalize_xyz if normalize_xyz is None else normalize_xyz
    l0_relu = p.l0_relu if l0_relu is None else l0_relu
    relu2 = p.relu2 if relu2 is None else relu2
    c = lambda t: t.to(dtype)
    g = FR._sa_gather64(c(p.xyz).transpose(1, 2).contiguous(), p.idx) - c(p.new_xyz).transpose(1, 2).unsqueeze(-1)     # (B,3,M,ns)
    if normalize_xyz:
        g = g / (float(np.float32(p.radius)) if dtype == torch.float64 else p.radius)
    t = FR._sa_gather64(p.term_of(dtype).transpose(1, 2).contiguous(), p.idx)                                          # (B,128,M,ns)
    h0 = t + torch.einsum("kc,bkmn->bcmn", c(p.wx), g)
    if l0_relu:
        h0 = torch.relu(h0)
    rows = h0.permute(0, 2, 3, 1)                                                                                       # (B,M,ns,128)
    h1 = torch.relu(_lin(rows, p.W1, mode) + c(p.sh1))
    h2 = _lin(h1, p.W2, mode) + c(p.sh2)
    if relu2:
        h2 = torch.relu(h2)
    return h2.max(dim=2)[0].transpose(1, 2).contiguous()


class Params(FR.Case):
    def term_of(self, dtype):
        """(B,N,128) per-point term in `dtype`: given (planted) or feats . (W0f * scale0)^T + shift0 (generic)."""
        if self.get("term") is not None:
            return self.term.to(dtype)
        return self.feats.to(dtype).transpose(1, 2) @ self.wf.to(dtype).t() + self.sh0.to(dtype)


def _folded(L):
    """(weight with the BatchNorm scale folded in float32 (Cout, Cin), shift float32 (Cout))."""
    w = L["conv_weight"].reshape(L["conv_weight"].shape[0], -1).float()
    scale, shift = FR.layer_affine(L)
    w = w if scale is None else w * scale.view(-1, 1)
    return w.contiguous(), (shift if shift is not None else torch.zeros(w.shape[0])).float().contiguous()


@functools.lru_cache(maxsize=None)
def inputs(name):
    """The operands of a generic case, float32: what the module would hand to the kernel (packs aside)."""
    c = FR.sa_case(name)
    assert c.hoist and c.spec == FR.SPEC1 and c.ns == 32
    w0, sh0 = _folded(c.layers[0])
    W1, sh1 = _folded(c.layers[1])
    W2, sh2 = _folded(c.layers[2])
    return Params(name=name, B=c.B, N=c.N, M=c.M, xyz=c.xyz, new_xyz=c.new_xyz, idx=c.idx, radius=c.radius, feats=c.feats, term=None,
                  wf=w0[:, 3:].contiguous(), wx=w0[:, 0:3].t().contiguous(), sh0=sh0, W1=W1, sh1=sh1, W2=W2, sh2=sh2,
                  normalize_xyz=True, l0_relu=True, relu2=True)


@functools.lru_cache(maxsize=None)
def generic_case(name, normalize_xyz=True, l0_relu=True, relu2=True):
    p = inputs(name)
    kw = dict(normalize_xyz=normalize_xyz, l0_relu=l0_relu, relu2=relu2)
    s64, s32 = level(p, torch.float64, **kw), level(p, torch.float32, **kw)
    return FR.Case(p=p, split64=s64, split32=s32, exact64=level(p, torch.float64, "exact", **kw), Y=FR.yardstick(s32, s64), **kw)


def _planted_values(rs, shape, e_lo, e_hi):
    """u * (1 + 2^-9), u = (1 + i / 128) * 2^e with i in [0, 128) and e in [e_lo, e_hi]: hi = u and lo = u * 2^-9 exactly."""
    i = rs.randint(0, 128, size=shape)
    e = rs.randint(e_lo, e_hi + 1, size=shape)
    u = (1.0 + i / 128.0) * np.exp2(e.astype(np.float64))
    v = (u * (1.0 + 2.0 ** -9)).astype(np.float32)
    assert np.array_equal(v.astype(np.float64), u * (1.0 + 2.0 ** -9))          # 17 significant bits: exact in float32
    return torch.from_numpy(v)


@functools.lru_cache(maxsize=None)
def planted_case(name, seed=PLANTED_SEED):
    """The index table (and clouds) of a generic case with operands that split exactly, all positive: wx = 0, both shifts zero,
    all ReLUs on. Layer 1's dropped lo . lo terms then all have one sign, so exact64 >= split64."""
    c = FR.sa_case(name)
    rs = np.random.RandomState(seed)
    term = _planted_values(rs, (c.B, 128, c.N), -2, 1).transpose(1, 2).contiguous()       # drawn as (B,128,N), used as (B,N,128)
    W1 = _planted_values(rs, (128, 128), -6, -4)
    W2 = _planted_values(rs, (256, 128), -6, -4)
    p = Params(name="planted_" + name, B=c.B, N=c.N, M=c.M, xyz=c.xyz, new_xyz=c.new_xyz, idx=c.idx, radius=c.radius, feats=None,
               term=term, wx=torch.zeros(3, 128), W1=W1, sh1=torch.zeros(128), W2=W2, sh2=torch.zeros(256),
               normalize_xyz=True, l0_relu=True, relu2=True)
    s64, s32 = level(p, torch.float64), level(p, torch.float32)
    return FR.Case(p=p, split64=s64, split32=s32, exact64=level(p, torch.float64, "exact"), plain32=level(p, torch.float32, "exact"),
                   Y=FR.yardstick(s32, s64))
