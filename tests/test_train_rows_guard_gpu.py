"""The kernels only a training step reaches — xcorr_z0 and its two backward forms, sa_z0_rows and sa_z0_bnbwd, the partial-sum
finishers, pt_attn_train_bwd, unit_rows / cos_bwd_rows — at the smallest shapes where each loop edge exists, against float64
(tests/train_rows_ref.py, anchored to autograd by tests/test_train_rows_ref_cpu.py), behind guard bands (tests/guard.py).

The method of tests/test_fused_guard_gpu.py and tests/test_index_guard_gpu.py: every launch goes through guard.launch on the C
ABI, every output in a guarded(...) buffer of exactly its size, every workspace in guard.workspace(...) of exactly the bytes its
query returns, every statistics / sums buffer of exactly chunks * 2 * C doubles (2C, 2C + 1 for the two sums finishers), every
input embed(...)-ded between NaN / INDEX_FILL words. Asserted per launch: check_guard on the outputs (all written), on inputs and
workspaces (nothing written outside); a second run gives the same bits; the guarded result equals, bit for bit, what the ops.*
wrapper returns.

The bound. For each result err = max|got - ref64| / max|ref64|; Y = max(e32, 4u), u = 2^-24, e32 the same distance for the
reference function run in float32 on the host (never the kernel's own output); err <= R * Y. Results with a derivable bound do
not use R: rel_rows and the sign of nrm are bit-equal to the float32 reference; xcorr's z0 is one fma, within one float32 ulp of
the float64 value (half an ulp for the fma, the rest covers the reference's own rounding); the `da` row of a one-hot softmax is
exactly 0; the float64 partial sums equal the column sums of the z0 the same launch wrote to 1e-12 of sum|z0| and sum z0^2; a
refused launch leaves every output word untouched.

ReLU masks. No argument z * a + b lies within 1e-4 of 0 (train_rows_ref.bn_relu_bwd asserts it on the reference side). xcorr's
z0 is derived from P, cos and w, so there `b` is chosen: the threshold sits in the widest gap of every column
(train_rows_ref.clear_shift). sa_z0_bnbwd's Z0 is an input, so there the offenders are nudged by 5e-4 / a.

Refusals: REFUSALS names the status the host code returns and the words of include/ptt_hip.h the refusal follows from.

The ratio R. err / Y measured on an MI355X, worst over the forms and layouts of a case; R = twice the worst ratio (1.02),
rounded up to one significant digit = 3, and R <= 8 is asserted. One case needed investigation, and it was not a ratio: the `da`
row of the one-hot point came out as 3e-8 .. 9e-8 instead of 0 at every shape with more than one point. attn_bwd_kernel used
dat = dres * vp twice, rounded inside the sum s and — contracted into an fma — unrounded inside `dat - s`; the product is now
rounded once for both uses.

  xcorr_z0 (B,n2,n1,C)    finished mean / var / invstd   _bwd dP / dcos / dw     _bnbwd dP / dcos / dw / dgamma / dbeta
  (1,1,1,4)               0.00 / 0.00 / 0.23             0.00 / 0.13 / 0.08      0.31 / 0.29 / 0.37 / 0.05 / 0.10
  (2,7,5,12)              0.10 / 0.14 / 0.13             0.27 / 0.25 / 0.35      0.27 / 0.19 / 0.66 / 0.07 / 0.10
  (3,9,3,256)             0.13 / 0.13 / 0.18             0.44 / 0.37 / 0.34      0.39 / 0.40 / 0.51 / 0.11 / 0.15
  (1,4,6,132)             0.09 / 0.19 / 0.19             0.33 / 0.30 / 0.26      0.37 / 0.24 / 0.46 / 0.19 / 0.10
  (2,33,10,64)            0.17 / 0.11 / 0.19             0.56 / 0.33 / 0.39      0.53 / 0.43 / 0.68 / 0.13 / 0.13
  sa_z0_rows (B,N,M,ns,C) z0, finished mean / var / invstd
  (1,5,1,1,4) 0.03, 0.00 / 0.00 / 0.23      (3,65,7,16,132) 0.26, 0.18 / 0.14 / 0.16      (2,200,33,32,64) 0.32, 0.15 / 0.09 / 0.11
  (2,40,3,64,1024) 0.30, 0.19 / 0.12 / 0.12      (64,64,40,32,256) 0.37, 0.16 / 0.12 / 0.12      (1,32,513,32,1024) 0.47
  (1,9,2,3,1028) 0.35
  sa_z0_bnbwd (R,C)       dz0 / d_wx / d_wx from the workspace partials / dgamma / dbeta
  (1,4) 0.29 / 0.29 / 0.29 / 0.17 / 0.20       (65,4) 0.36 / 0.86 / 0.80 / 0.15 / 0.08       (555,64) 0.33 / 0.28 / 0.24 / 0.16 / 0.18
  (70001,132) 0.35 / 0.03 / 0.01 / 0.17 / 0.15   (300,1024) 0.30 / 0.33 / 0.33 / 0.16 / 0.11   (131073,8) 0.31 / 0.02 / 0.02 / 0.17 / 0.08
  finishers, worst over chunks in {1, 255, 256, 257, 700} and C in {1, 5, 260}
  bn_bwd_consts dgamma 0.21  dbeta 0.23  k1 0.18  c0 0.26  c1 0.29
  bn_finish_partials_train mean 0.22  var 0.22  invstd 0.24  act_a 0.40  act_b 0.77  running_mean 0.39  running_var 0.35
  bn_update_running running_mean 0.49  running_var 0.29
  pt_attn_train_bwd (B,N,k,D) da / dvp
  (1,1,8,4) 0.52 / 0.13     (2,17,16,132) 0.45 / 0.22     (3,33,32,64) 0.54 / 0.08     (1,40,8,512) 0.58 / 0.13
  unit_rows unit / |nrm|, worst over C in {1, 63, 64, 65, 260}: n = 1: 0.35 / 0.18     n = 5: 0.24 / 0.27
  cos_bwd_rows dx, worst over C, n, m in {1, 63, 65, 130}, both sides and both layouts: 1.02; the rows under the clamp 0.24

The whole file takes about six seconds on an MI355X; no case more than one.
"""
import ctypes
import os
import re

import pytest
import torch

from ptt_amd import _lib, ops
from tests import guard
from tests import train_rows_ref as T
from tests.guard import check_guard, embed, guarded

pytestmark = pytest.mark.gpu
L, P = guard.launch, guard.ptr
F32, F64, I32, I64 = torch.float32, torch.float64, torch.int32, torch.int64
U = 2.0 ** -24
EPS = 1e-5

R_RATIO = 3.0               # twice the worst measured err / Y (1.02, table above), rounded up to one significant digit
RATIOS = {}                 # result -> worst err / Y of its runs: printed by test_zz_ratio_report


def test_r_is_within_its_cap():
    assert R_RATIO <= 8


def bound(case, got, ref64, ref32):
    """err <= R * Y for one result; the references live on the host."""
    Y = max(T.rel_err(ref32, ref64), 4 * U)
    err = T.rel_err(got.detach().cpu(), ref64)
    r = err / Y
    RATIOS[case] = max(RATIOS.get(case, 0.0), r)
    print("RATIO %-52s err %.3e  Y %.3e  err/Y %.2f" % (case, err, Y, r))
    assert r <= R_RATIO, "%s: %.2f x the float32 formulation's own distance from float64 (R = %g)" % (case, r, R_RATIO)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rnd(g, *shape):
    return torch.randn(*shape, generator=g, dtype=F32)


def away(g, *shape):
    """Random signs, magnitudes in [0.5, 1.5)."""
    return (torch.rand(*shape, generator=g, dtype=F32) + 0.5) * (torch.randint(0, 2, shape, generator=g) * 2 - 1).to(F32)


def E(t, dev, **kw):
    return embed(t.to(dev).contiguous(), **kw)


def G(shape, dtype, dev, **kw):
    return guarded(shape, dtype, device=dev, **kw)


def done(outs, ins=(), ws=()):
    torch.cuda.synchronize()
    for v in outs:
        check_guard(v)
    for v in tuple(ins) + tuple(ws):
        check_guard(v, all_written=False)


def bits(t):
    return t.contiguous().view(I32)


def same_bits(a, b, what):
    assert a.numel() == b.numel() and torch.equal(bits(a).reshape(-1), bits(b.to(a.device)).reshape(-1)), "%s: not the same bits" % what


def twice(run, what):
    """run() -> tuple of guarded outputs, each checked; the second run's bits equal the first's. -> the first run's outputs."""
    first, second = run(), run()
    for k, (a, b) in enumerate(zip(first, second)):
        same_bits(a, b, "%s: output %d of a second run" % (what, k))
    return first


def within_one_ulp(got, ref64, what):
    """|got - ref64| <= the spacing of float32 at |ref64| (2^-149 at least)."""
    ref64 = ref64.to(got.device)
    _, e = torch.frexp(ref64.abs())
    ulp = torch.ldexp(torch.ones_like(ref64), (e - 24).clamp_min(-149))
    bad = (got.double().reshape(ref64.shape) - ref64).abs() > ulp
    assert not bool(bad.any()), "%s: %d values farther than one float32 ulp from the float64 value" % (what, int(bad.sum()))


def check_partials(part, chunks, C, z0, what):
    """The summed float64 partials are the column sums of the z0 the launch wrote; -> the partials as (chunks, 2, C)."""
    part3 = part.reshape(chunks, 2, C)
    s = part3.sum(0)
    z = z0.double()
    assert bool(((s[0] - z.sum(0)).abs() <= 1e-12 * z.abs().sum(0)).all()), "%s: column sums" % what
    assert bool(((s[1] - (z * z).sum(0)).abs() <= 1e-12 * (z * z).sum(0)).all()), "%s: column sums of squares" % what
    return part3


def check_finish(case, part3, z0, rows):
    """ops.bn_finish_partials on the launch's partials against the float64 mean / variance / invstd of the z0 it wrote."""
    got = ops.bn_finish_partials(part3.contiguous(), rows, EPS)
    z32 = z0.detach().cpu().contiguous()
    z64 = z32.double()
    for name, g, r64, r32 in zip(("mean", "var", "invstd"), got,
                                 (z64.mean(0), z64.var(0, unbiased=False), 1 / torch.sqrt(z64.var(0, unbiased=False) + EPS)),
                                 (z32.mean(0), z32.var(0, unbiased=False), 1 / torch.sqrt(z32.var(0, unbiased=False) + EPS))):
        bound("%s %s" % (case, name), g, r64, r32)


# ================================================================================================================ refusals
def _header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "ptt_hip.h")) as fh:
        return " ".join(re.sub(r"^\s*\*", " ", fh.read(), flags=re.M).split())


# refusal -> (status, the words of include/ptt_hip.h it follows from)
REFUSALS = {
    "xcorr_stats_C_1028":   ("PTT_EUNSUPPORTED", "at most 1024 channels (PTT_EUNSUPPORTED otherwise, and the chunk query returns 0)"),
    "xcorr_bwd_C_260":      ("PTT_EINVAL", "C % 4 == 0; the backward needs C <= 256 (PTT_EINVAL otherwise)"),
    "xcorr_C_6":            ("PTT_EINVAL", "C % 4 == 0; the backward needs C <= 256 (PTT_EINVAL otherwise)"),
    "xcorr_ws_short":       ("PTT_EWORKSPACE", "a workspace of at least ptt_xcorr_z0_bwd_workspace(B, n1, C) bytes (PTT_EWORKSPACE otherwise)"),
    "xcorr_partials_short": ("PTT_EWORKSPACE", "fewer than chunks * 2 * C partial_elems: PTT_EWORKSPACE"),
    "sa_stats_C_1028":      ("PTT_EUNSUPPORTED", "C <= 1024 (PTT_EUNSUPPORTED otherwise, and the chunk query returns 0)"),
    "sa_radius_0":          ("PTT_EINVAL", "C % 4 == 0, radius > 0 (PTT_EINVAL otherwise)"),
    "sa_ldw_2":             ("PTT_EINVAL", "row stride ldw >= 3"),
    "sa_C_6":               ("PTT_EINVAL", "C % 4 == 0, radius > 0 (PTT_EINVAL otherwise)"),
    "sa_rows_per_cloud":    ("PTT_EUNSUPPORTED", "at most (2^31 - 1) / 4 rows per cloud (PTT_EUNSUPPORTED otherwise)"),
}


def refused(what, fn, *outputs):
    status, words = REFUSALS[what]
    assert words in _header(), "%s: include/ptt_hip.h does not document this refusal" % what
    with pytest.raises(RuntimeError, match=status):
        fn()
    torch.cuda.synchronize()
    guard.assert_untouched(*outputs)


# ============================================================================================================ xcorr_z0 family
XCORR = [(1, 1, 1, 4), (2, 7, 5, 12), (3, 9, 3, 256), (1, 4, 6, 132), (2, 33, 10, 64)]


def xcorr_inputs(B, n2, n1, C):
    g = gen(B * 100000 + n2 * 100 + n1 + C)
    P_, cos, w = rnd(g, B, n1, C), torch.rand(B, n2, n1, generator=g, dtype=F32) * 2 - 1, rnd(g, C)
    flat = cos.view(-1)
    flat[3::7], flat[4::11], flat[5::13] = 0.0, 1.0, -1.0          # some cosines exactly 0, 1 and -1
    return g, P_, cos, w


def xcorr_forward(dev, Pe, ce, we, B, n2, n1, C, stats):
    rows = B * n2 * n1
    z0 = G((rows, C), F32, dev)
    if not stats:
        L("ptt_xcorr_z0_f32", dev, P(Pe), P(ce), P(we), B, n2, n1, C, P(z0))
        done([z0], [Pe, ce, we])
        return z0, None
    chunks = int(ops._host("ptt_xcorr_z0_stat_chunks", B, n2, n1, C))
    part = G((chunks * 2 * C,), F64, dev)
    L("ptt_xcorr_z0_stats_f32", dev, P(Pe), P(ce), P(we), B, n2, n1, C, P(z0), P(part), chunks * 2 * C)
    done([z0, part], [Pe, ce, we])
    return z0, part


@pytest.mark.parametrize("B,n2,n1,C", XCORR)
def test_xcorr_z0_forward(dev, B, n2, n1, C):
    _, P_, cos, w = xcorr_inputs(B, n2, n1, C)
    Pe, ce, we = E(P_, dev), E(cos, dev), E(w, dev)
    rows, tag = B * n2 * n1, "xcorr_z0 %s" % ((B, n2, n1, C),)
    ref64 = T.xcorr_z0(P_, cos, w)[0]
    z0 = twice(lambda: xcorr_forward(dev, Pe, ce, we, B, n2, n1, C, False)[:1], tag)[0]
    within_one_ulp(z0, ref64, tag)
    same_bits(z0, ops.xcorr_z0(Pe.contiguous(), ce.contiguous(), we.contiguous()), tag + " against ops.xcorr_z0")
    z0s, part = twice(lambda: xcorr_forward(dev, Pe, ce, we, B, n2, n1, C, True), tag + " with stats")
    chunks = part.numel() // (2 * C)
    same_bits(z0s, z0, tag + ": z0 with and without statistics")
    part3 = check_partials(part, chunks, C, z0s, tag)
    p_z0, p_part = ops.xcorr_z0(Pe.contiguous(), ce.contiguous(), we.contiguous(), want_stats=True)
    same_bits(z0s, p_z0, tag + " against ops.xcorr_z0(want_stats)")
    assert tuple(p_part.shape) == (chunks, 2, C) and torch.equal(p_part, part3), tag + ": partials against ops.xcorr_z0(want_stats)"
    check_finish(tag, part3, z0s, rows)


def test_xcorr_z0_stats_past_the_grid_cap(dev):
    """33153 rows at 8 per workgroup = 4145 workgroups, capped at 4096: the stride loop runs with statistics on."""
    B, n2, n1, C = 1, 257, 129, 1024
    _, P_, cos, w = xcorr_inputs(B, n2, n1, C)
    Pe, ce, we = E(P_, dev), E(cos, dev), E(w, dev)
    assert int(ops._host("ptt_xcorr_z0_stat_chunks", B, n2, n1, C)) == 4096
    z0, part = xcorr_forward(dev, Pe, ce, we, B, n2, n1, C, True)
    within_one_ulp(z0, T.xcorr_z0(P_.to(dev), cos.to(dev), w.to(dev))[0], "xcorr_z0 past the stats cap")
    check_partials(part, 4096, C, z0, "xcorr_z0 past the stats cap")


def test_xcorr_z0_past_the_plain_grid_cap(dev):
    """131200 rows at 8 per workgroup = 16400 workgroups, capped at 16384; the reference is formed on the device in slices of n2."""
    B, n2, n1, C = 1, 1025, 128, 1024
    _, P_, cos, w = xcorr_inputs(B, n2, n1, C)
    Pe, ce, we = E(P_, dev), E(cos, dev), E(w, dev)
    z0, _ = xcorr_forward(dev, Pe, ce, we, B, n2, n1, C, False)
    Pd, cd, wd = P_.to(dev), cos.to(dev), w.to(dev)
    for j0 in range(0, n2, 205):
        j1 = min(n2, j0 + 205)
        within_one_ulp(z0[j0 * n1:j1 * n1], T.xcorr_z0(Pd, cd[:, j0:j1], wd)[0], "xcorr_z0 past the grid cap, search points %d..%d" % (j0, j1))


def test_xcorr_z0_two_quads_per_thread(dev):
    """C = 1028: 257 channel quads on 256 threads, the `q += span` loop; accepted without statistics only."""
    B, n2, n1, C = 2, 7, 5, 1028
    _, P_, cos, w = xcorr_inputs(B, n2, n1, C)
    Pe, ce, we = E(P_, dev), E(cos, dev), E(w, dev)
    z0, _ = xcorr_forward(dev, Pe, ce, we, B, n2, n1, C, False)
    within_one_ulp(z0, T.xcorr_z0(P_, cos, w)[0], "xcorr_z0 C = 1028")
    same_bits(z0, ops.xcorr_z0(Pe.contiguous(), ce.contiguous(), we.contiguous()), "C = 1028 against ops.xcorr_z0")
    assert int(ops._host("ptt_xcorr_z0_stat_chunks", B, n2, n1, C)) == 0
    z0, part = G((B * n2 * n1, C), F32, dev), G((64 * 2 * C,), F64, dev)
    refused("xcorr_stats_C_1028", lambda: L("ptt_xcorr_z0_stats_f32", dev, P(Pe), P(ce), P(we), B, n2, n1, C, P(z0), P(part), part.numel()),
            z0, part)


def xcorr_bwd_outputs(dev, B, n2, n1, C, extra=0):
    nbytes = int(ops._host("ptt_xcorr_z0_bwd_workspace", B, n1, C))
    return ([G((B, n1, C), F32, dev), G((B, n2, n1), F32, dev)] + [G((C,), F32, dev) for _ in range(1 + extra)],
            guard.workspace(nbytes, device=dev), nbytes)


@pytest.mark.parametrize("B,n2,n1,C", XCORR)
def test_xcorr_z0_backward(dev, B, n2, n1, C):
    g, P_, cos, w = xcorr_inputs(B, n2, n1, C)
    dz0 = rnd(g, B * n2 * n1, C)
    de, ce, we = E(dz0, dev), E(cos, dev), E(w, dev)
    tag = "xcorr_z0_bwd %s" % ((B, n2, n1, C),)

    def run():
        outs, ws, nbytes = xcorr_bwd_outputs(dev, B, n2, n1, C)
        L("ptt_xcorr_z0_bwd_f32", dev, P(de), P(ce), P(we), B, n2, n1, C, *[P(o) for o in outs], P(ws), nbytes)
        done(outs, [de, ce, we], [ws])
        return outs
    outs = twice(run, tag)
    plain = ops.xcorr_z0_bwd(de.contiguous(), ce.contiguous(), we.contiguous(), B, n2, n1)
    for name, got, r64, r32, p in zip(("dP", "dcos", "dw"), outs, T.xcorr_z0_bwd(dz0, cos, w, B, n2, n1),
                                      T.xcorr_z0_bwd(dz0, cos, w, B, n2, n1, F32), plain):
        bound("%s %s" % (tag, name), got, r64, r32)
        same_bits(got, p, "%s %s against ops.xcorr_z0_bwd" % (tag, name))


def bn_inputs(g, C, chunks):
    """mean, invstd, gamma, act_a of a BatchNorm nobody ran (they are inputs of the ABI) and arbitrary float64 chunk partials."""
    return (rnd(g, C), rnd(g, C).abs() + 0.5, rnd(g, C), away(g, C), torch.randn(chunks, 2, C, generator=g, dtype=F64))


@pytest.mark.parametrize("B,n2,n1,C", XCORR)
def test_xcorr_z0_bn_backward(dev, B, n2, n1, C):
    g, P_, cos, w = xcorr_inputs(B, n2, n1, C)
    up = rnd(g, B * n2 * n1, C)
    mean, invstd, gamma, a, part = bn_inputs(g, C, 9)
    b = T.clear_shift(T.xcorr_z0_f32(P_, cos, w).double() * a.double())           # the threshold in the widest gap of every column
    ins = [E(t, dev) for t in (part, up, P_, cos, w, mean, invstd, gamma, a, b)]
    tag = "xcorr_z0_bnbwd %s" % ((B, n2, n1, C),)

    def run():
        outs, ws, nbytes = xcorr_bwd_outputs(dev, B, n2, n1, C, extra=2)
        L("ptt_xcorr_z0_bnbwd_f32", dev, P(ins[0]), 9, *[P(v) for v in ins[1:]], B, n2, n1, C, *[P(o) for o in outs], P(ws), nbytes)
        done(outs, ins, [ws])
        return outs
    outs = twice(run, tag)
    plain = ops.xcorr_z0_bnbwd(*[v.contiguous() for v in ins])
    args = (part, up, P_, cos, w, mean, invstd, gamma, a, b)
    for name, got, r64, r32, p in zip(("dP", "dcos", "dw", "dgamma", "dbeta"), outs, T.xcorr_z0_bnbwd(*args), T.xcorr_z0_bnbwd(*args, dtype=F32), plain):
        bound("%s %s" % (tag, name), got, r64, r32)
        same_bits(got, p, "%s %s against ops.xcorr_z0_bnbwd" % (tag, name))


def test_xcorr_z0_refusals(dev):
    """Every array has the size the refused shape would need: were the launch not refused, it would run inside its buffers."""
    for what, C in (("xcorr_bwd_C_260", 260), ("xcorr_C_6", 6)):
        B, n2, n1 = 2, 7, 5
        g, P_, cos, w = xcorr_inputs(B, n2, n1, C)
        up = rnd(g, B * n2 * n1, C)
        mean, invstd, gamma, a, part = bn_inputs(g, C, 9)
        ins = [E(t, dev) for t in (part, up, P_, cos, w, mean, invstd, gamma, a, rnd(g, C))]
        if C == 6:
            z0 = G((B * n2 * n1, C), F32, dev)
            refused(what, lambda: L("ptt_xcorr_z0_f32", dev, P(ins[2]), P(ins[3]), P(ins[4]), B, n2, n1, C, P(z0)), z0)
        outs, ws, nbytes = xcorr_bwd_outputs(dev, B, n2, n1, C, extra=2)
        refused(what, lambda: L("ptt_xcorr_z0_bwd_f32", dev, P(ins[1]), P(ins[3]), P(ins[4]), B, n2, n1, C, *[P(o) for o in outs[:3]], P(ws), nbytes),
                *outs, ws)
        refused(what, lambda: L("ptt_xcorr_z0_bnbwd_f32", dev, P(ins[0]), 9, *[P(v) for v in ins[1:]], B, n2, n1, C, *[P(o) for o in outs], P(ws),
                                nbytes), *outs, ws)
    B, n2, n1, C = 2, 7, 5, 12
    g, P_, cos, w = xcorr_inputs(B, n2, n1, C)
    up = rnd(g, B * n2 * n1, C)
    mean, invstd, gamma, a, part = bn_inputs(g, C, 9)
    ins = [E(t, dev) for t in (part, up, P_, cos, w, mean, invstd, gamma, a, rnd(g, C))]
    outs, ws, nbytes = xcorr_bwd_outputs(dev, B, n2, n1, C, extra=2)           # a workspace 4 bytes short
    refused("xcorr_ws_short", lambda: L("ptt_xcorr_z0_bwd_f32", dev, P(ins[1]), P(ins[3]), P(ins[4]), B, n2, n1, C, *[P(o) for o in outs[:3]], P(ws),
                                        nbytes - 4), *outs, ws)
    refused("xcorr_ws_short", lambda: L("ptt_xcorr_z0_bnbwd_f32", dev, P(ins[0]), 9, *[P(v) for v in ins[1:]], B, n2, n1, C, *[P(o) for o in outs],
                                        P(ws), nbytes - 4), *outs, ws)
    chunks = int(ops._host("ptt_xcorr_z0_stat_chunks", B, n2, n1, C))            # partials one double short
    z0, part = G((B * n2 * n1, C), F32, dev), G((chunks * 2 * C,), F64, dev)
    refused("xcorr_partials_short", lambda: L("ptt_xcorr_z0_stats_f32", dev, P(ins[2]), P(ins[3]), P(ins[4]), B, n2, n1, C, P(z0), P(part),
                                              chunks * 2 * C - 1), z0, part)


# ====================================================================================================== sa_z0_rows / stats
def sa_inputs(B, N, M, ns, C, with_term):
    """idx built by hand: groups padded with their first index, as the ball query pads them; (B > 1) one cloud whose every entry
    is the same point; (more than one row) one centre that coincides with its neighbour (rel exactly 0)."""
    g = gen(N * 1000 + M * 10 + C)
    xyz, new_xyz = rnd(g, B, N, 3) * 0.3, rnd(g, B, M, 3) * 0.3
    idx = torch.randint(0, N, (B, M, ns), generator=g)
    count = torch.randint(1, ns + 1, (B, M, 1), generator=g)
    idx = torch.where(torch.arange(ns).view(1, 1, ns) >= count, idx[..., :1], idx)
    if B > 1:
        idx[B - 1] = N // 2
    if B * M * ns > 1:
        new_xyz[0, 0] = xyz[0, idx[0, 0, 0]]
    return xyz, new_xyz, idx.to(I32), (rnd(g, B, N, C) if with_term else None), rnd(g, C, 3)


def sa_embed(dev, xyz, new_xyz, idx, term, wx, ldw):
    """-> (the embedded inputs, wx as the (C,3) view the launch reads). ldw > 3: the first three columns of a (C, ldw) weight
    whose other columns are NaN."""
    xe, ne, ie = E(xyz, dev), E(new_xyz, dev), E(idx, dev)
    te = E(term, dev) if term is not None else None
    if ldw == 3:
        we = E(wx, dev)
        wv = we
    else:
        full = torch.full((wx.shape[0], ldw), float("nan"), dtype=F32)
        full[:, :3] = wx
        we = E(full, dev)
        wv = we[:, :3]
    return xe, ne, ie, te, we, wv


def sa_forward(dev, emb, ldw, B, N, M, ns, C, radius, normalize, stats):
    xe, ne, ie, te, we, _ = emb
    rows = B * M * ns
    z0, rel = G((rows, C), F32, dev), G((rows, 3), F32, dev)
    ins = [v for v in (xe, ne, ie, te, we) if v is not None]
    if not stats:
        L("ptt_sa_z0_rows_f32", dev, P(xe), P(ne), P(ie), P(te), P(we), ldw, B, N, M, ns, C, radius, int(normalize), P(z0), P(rel))
        done([z0, rel], ins)
        return z0, rel
    chunks = int(ops._host("ptt_sa_z0_rows_stat_chunks", B, M, ns, C))
    part = G((chunks * 2 * C,), F64, dev)
    L("ptt_sa_z0_rows_stats_f32", dev, P(xe), P(ne), P(ie), P(te), P(we), ldw, B, N, M, ns, C, radius, int(normalize), P(z0), P(rel), P(part),
      chunks * 2 * C)
    done([z0, rel, part], ins)
    return z0, rel, part


def sa_case(dev, B, N, M, ns, C, with_term, normalize, radius, ldw, plain=True, stats=True, stat_chunks=None):
    xyz, new_xyz, idx, term, wx = sa_inputs(B, N, M, ns, C, with_term)
    emb = sa_embed(dev, xyz, new_xyz, idx, term, wx, ldw)
    rows, tag = B * M * ns, "sa_z0_rows %s" % ((B, N, M, ns, C),)
    ref64, rel_ref = T.sa_z0_rows(xyz, new_xyz, idx, term, wx, radius, normalize)
    ref32 = T.sa_z0_rows(xyz, new_xyz, idx, term, wx, radius, normalize, F32)[0]
    assert rows == 1 or float(rel_ref.view(B, M, ns, 3)[0, 0, 0].abs().max()) == 0.0           # the coinciding centre
    z0 = None
    if plain:
        z0, rel = twice(lambda: sa_forward(dev, emb, ldw, B, N, M, ns, C, radius, normalize, False), tag)
        same_bits(rel, rel_ref, tag + ": rel_rows against the float32 reference")
        bound(tag + " z0", z0, ref64, ref32)
        p = ops.sa_z0_rows(*[v.contiguous() if v is not None else None for v in emb[:4]], emb[5], radius, normalize)
        same_bits(z0, p[0], tag + " against ops.sa_z0_rows")
        same_bits(rel, p[1], tag + " against ops.sa_z0_rows (rel)")
    if stats:
        chunks = int(ops._host("ptt_sa_z0_rows_stat_chunks", B, M, ns, C))
        if stat_chunks is not None:
            assert chunks == stat_chunks
        z0s, rels, part = twice(lambda: sa_forward(dev, emb, ldw, B, N, M, ns, C, radius, normalize, True), tag + " with stats")
        same_bits(rels, rel_ref, tag + ": rel_rows of the stats form")
        if z0 is not None:
            same_bits(z0s, z0, tag + ": z0 with and without statistics")
        else:
            bound(tag + " z0 (stats form)", z0s, ref64, ref32)
        part3 = check_partials(part, chunks, C, z0s, tag)
        p = ops.sa_z0_rows(*[v.contiguous() if v is not None else None for v in emb[:4]], emb[5], radius, normalize, want_stats=True)
        same_bits(z0s, p[0], tag + " against ops.sa_z0_rows(want_stats)")
        assert torch.equal(p[2], part3), tag + ": partials against ops.sa_z0_rows(want_stats)"
        check_finish(tag, part3, z0s, rows)


@pytest.mark.parametrize("B,N,M,ns,C,with_term,normalize,ldw", [(1, 5, 1, 1, 4, False, False, 3), (3, 65, 7, 16, 132, True, True, 135),
                                                               (2, 200, 33, 32, 64, False, True, 3), (2, 40, 3, 64, 1024, True, False, 3)])
def test_sa_z0_rows(dev, B, N, M, ns, C, with_term, normalize, ldw):
    sa_case(dev, B, N, M, ns, C, with_term, normalize, 0.3, ldw)


def test_sa_z0_rows_stats_past_the_grid_cap(dev):
    """E = 1280 rows per cloud, four row groups, four rows each: 80 workgroups per cloud before the cap of ceil(4096 / 64) = 64."""
    sa_case(dev, 64, 64, 40, 32, 256, True, True, 0.3, 3, plain=False, stat_chunks=64 * 64)


def test_sa_z0_rows_past_the_plain_grid_cap(dev):
    """E = 16416 rows of one row group, four rows per workgroup: 4104 workgroups, capped at 4096."""
    sa_case(dev, 1, 32, 513, 32, 1024, False, True, 0.3, 3, stats=False)


def test_sa_z0_rows_two_quads_per_thread(dev):
    """C = 1028 is accepted without statistics and refused with them."""
    B, N, M, ns, C = 1, 9, 2, 3, 1028
    sa_case(dev, B, N, M, ns, C, True, True, 0.3, 3, stats=False)
    assert int(ops._host("ptt_sa_z0_rows_stat_chunks", B, M, ns, C)) == 0
    xe, ne, ie, te, we, _ = sa_embed(dev, *sa_inputs(B, N, M, ns, C, True), 3)
    z0, rel, part = G((B * M * ns, C), F32, dev), G((B * M * ns, 3), F32, dev), G((2 * C,), F64, dev)
    refused("sa_stats_C_1028", lambda: L("ptt_sa_z0_rows_stats_f32", dev, P(xe), P(ne), P(ie), P(te), P(we), 3, B, N, M, ns, C, 0.3, 1, P(z0), P(rel),
                                         P(part), part.numel()), z0, rel, part)


def test_sa_z0_rows_refusals(dev):
    B, N, M, ns = 2, 40, 3, 16
    for what, C, radius, ldw in (("sa_radius_0", 8, 0.0, 3), ("sa_ldw_2", 8, 0.3, 2), ("sa_C_6", 6, 0.3, 3)):
        xe, ne, ie, te, we, _ = sa_embed(dev, *sa_inputs(B, N, M, ns, C, True), 3)
        chunks = max(1, int(ops._host("ptt_sa_z0_rows_stat_chunks", B, M, ns, C)))
        z0, rel, part = G((B * M * ns, C), F32, dev), G((B * M * ns, 3), F32, dev), G((chunks * 2 * C,), F64, dev)
        refused(what, lambda: L("ptt_sa_z0_rows_f32", dev, P(xe), P(ne), P(ie), P(te), P(we), ldw, B, N, M, ns, C, radius, 1, P(z0), P(rel)), z0, rel)
        refused(what, lambda: L("ptt_sa_z0_rows_stats_f32", dev, P(xe), P(ne), P(ie), P(te), P(we), ldw, B, N, M, ns, C, radius, 1, P(z0), P(rel),
                                P(part), part.numel()), z0, rel, part)
    # more rows per cloud than an int holds four times over: dimensions only, the host refuses before it reads a pointer
    d = [G((4,), F32, dev) for _ in range(6)]
    refused("sa_rows_per_cloud", lambda: L("ptt_sa_z0_rows_f32", dev, P(d[0]), P(d[1]), P(d[2]), None, P(d[3]), 3, 1, 8, 1 << 29, 1, 4, 0.3, 1,
                                           P(d[4]), P(d[5])), *d)


# ============================================================================================================== sa_z0_bnbwd
@pytest.mark.parametrize("R,C", [(1, 4), (65, 4), (555, 64), (70001, 132), (300, 1024), (131073, 8)])
def test_sa_z0_bn_backward(dev, R, C):
    g = gen(R + C)
    up, z, rel = rnd(g, R, C), rnd(g, R, C), rnd(g, R, 3)
    mean, invstd, gamma, a, part = bn_inputs(g, C, 17)
    b = rnd(g, C)
    arg = z.double() * a.double() + b.double()                     # offenders nudged: z * a + b moves by +5e-4, out of the band
    z = torch.where(arg.abs() < 2e-4, (z.double() + 5e-4 / a.double()).float(), z)
    assert T.near_flips(z, a, b) == 0
    ins = [E(t, dev) for t in (part, up, z, rel, mean, invstd, gamma, a, b)]
    nbytes = int(ops._host("ptt_sa_z0_bnbwd_workspace", R, C))
    tag = "sa_z0_bnbwd %s" % ((R, C),)
    r64 = T.sa_z0_bnbwd(part, up, z, rel, mean, invstd, gamma, a, b)
    r32 = T.sa_z0_bnbwd(part, up, z, rel, mean, invstd, gamma, a, b, dtype=F32)

    def launch(Ge, dz_out, dwx):
        dgamma, dbeta, ws = G((C,), F32, dev), G((C,), F32, dev), guard.workspace(nbytes, device=dev)
        L("ptt_sa_z0_bnbwd_f32", dev, P(ins[0]), 17, P(Ge), *[P(v) for v in ins[2:]], R, C, P(dz_out), P(dwx), P(dgamma), P(dbeta), P(ws), nbytes)
        outs = [dgamma, dbeta] + ([dwx] if dwx is not None else []) + ([dz_out] if dz_out is not None and dz_out is not Ge else [])
        done(outs, [Ge] + ins, [ws])
        return dgamma, dbeta, ws

    def check(dz, dwx, dgamma, dbeta):
        for name, got, k in (("dz0", dz, 0), ("d_wx", dwx, 1), ("dgamma", dgamma, 2), ("dbeta", dbeta, 3)):
            if got is not None:
                bound("%s %s" % (tag, name), got, r64[k], r32[k])
        return [t for t in (dz, dwx, dgamma, dbeta) if t is not None]

    # dz_out NULL: G is untouched
    dwx = G((C, 3), F32, dev)
    dgamma, dbeta, _ = launch(ins[1], None, dwx)
    same_bits(ins[1], up, tag + ": G after a launch without dz_out")
    first = check(None, dwx, dgamma, dbeta)
    p = ops.sa_z0_bnbwd(ins[0].contiguous(), ins[1].contiguous(), *[v.contiguous() for v in ins[2:]], False)
    for got, want in zip(first, p[1:]):
        same_bits(got, want, tag + " against ops.sa_z0_bnbwd(want_dz=False)")
    # dz_out a buffer of its own: G is untouched; d_wx left as partial sums in the workspace
    dz = G((R, C), F32, dev)
    dgamma, dbeta, ws = launch(ins[1], dz, None)
    same_bits(ins[1], up, tag + ": G after a launch with a separate dz_out")
    nchunks = nbytes // (12 * C)
    dwx_sum = ws.view(F32).reshape(nchunks, C, 3).double().sum(0)
    bound(tag + " d_wx from the workspace partials", dwx_sum, r64[1], r32[1])
    second = check(dz, None, dgamma, dbeta)
    same_bits(second[1], first[1], tag + ": dgamma of the two forms")
    same_bits(second[2], first[2], tag + ": dbeta of the two forms")
    # dz_out aliasing G
    Ge, dwx2 = E(up, dev), G((C, 3), F32, dev)
    dgamma, dbeta, _ = launch(Ge, Ge, dwx2)
    same_bits(Ge, dz, tag + ": dz0 written over G against dz0 in a buffer of its own")
    same_bits(dwx2, dwx, tag + ": d_wx of a second run")
    p = ops.sa_z0_bnbwd(ins[0].contiguous(), up.to(dev), *[v.contiguous() for v in ins[2:]], True)
    for got, want, name in zip((Ge, dwx2, dgamma, dbeta), p, ("dz0", "d_wx", "dgamma", "dbeta")):
        same_bits(got, want, "%s %s against ops.sa_z0_bnbwd(want_dz=True)" % (tag, name))


# ================================================================================================== partial-sum finishers
def chunked_partials(g, chunks, C):
    """Real data cut into `chunks` pieces -> (x (rows, C) float32, its per-chunk float64 sums and sums of squares (chunks, 2, C))."""
    rows = 3 * chunks + 1
    x = rnd(g, rows, C) * 2 + 0.5
    pieces = torch.tensor_split(x.double(), chunks, 0)
    return x, torch.stack([torch.stack([p.sum(0), (p * p).sum(0)]) for p in pieces])


@pytest.mark.parametrize("chunks", [1, 255, 256, 257, 700])
@pytest.mark.parametrize("C", [1, 5, 260])
def test_partial_sum_finishers(dev, chunks, C):
    g = gen(chunks * 1000 + C)
    x, part = chunked_partials(g, chunks, C)
    rows, tag = x.shape[0], "finishers (chunks %d, C %d)" % (chunks, C)
    pe = E(part, dev)
    s0, s1 = T.partial_sums(part)
    scale = part.abs().sum(0)

    # the two sums finishers: 2C + 1 doubles with the row count, 2C without (the guard word behind them is the point)
    sums = G((2 * C + 1,), F64, dev)
    L("ptt_bn_sums_partials_f64", dev, P(pe), chunks, C, rows, P(sums))
    done([sums], [pe])
    bw = G((2 * C,), F64, dev)
    L("ptt_bn_bwd_sums_partials_f64", dev, P(pe), chunks, C, P(bw))
    done([bw], [pe])
    got = sums.cpu()
    assert float(got[2 * C]) == float(rows), tag + ": the count slot"
    assert bool(((got[:C] - s0).abs() <= 1e-12 * scale[0]).all()) and bool(((got[C:2 * C] - s1).abs() <= 1e-12 * scale[1]).all()), tag
    same_bits(sums[:2 * C], bw, tag + ": the two sums finishers")
    same_bits(sums, ops.bn_sums_partials(pe.contiguous(), rows), tag + " against ops.bn_sums_partials")
    same_bits(bw, ops.bn_bwd_sums_from_partials(pe.contiguous()), tag + " against ops.bn_bwd_sums_from_partials")

    # the constants of a BatchNorm backward applied by its consumer
    mean, invstd, gamma = rnd(g, C), rnd(g, C).abs() + 0.5, rnd(g, C)
    me, ie, ge = E(mean, dev), E(invstd, dev), E(gamma, dev)
    outs = [G((C,), F32, dev) for _ in range(5)]
    L("ptt_bn_bwd_consts_f32", dev, P(pe), chunks, P(me), P(ie), P(ge), rows, C, *[P(o) for o in outs])
    done(outs, [pe, me, ie, ge])
    p = ops.bn_bwd_consts(pe.contiguous(), me.contiguous(), ie.contiguous(), ge.contiguous(), rows)
    for name, got, r64, r32, want in zip(("dgamma", "dbeta", "k1", "c0", "c1"), outs, T.bn_bwd_consts(part, mean, invstd, gamma, rows),
                                         T.bn_bwd_consts(part, mean, invstd, gamma, rows, F32), (p[0], p[1]) + tuple(p[2])):
        bound("bn_bwd_consts %s" % name, got, r64, r32)
        same_bits(got, want, "%s %s against ops.bn_bwd_consts" % (tag, name))

    # the statistics with the training tail: all members, the activation constants only, the running statistics only, none
    x64 = x.double()
    m64, v64 = x64.mean(0), x64.var(0, unbiased=False)
    i64 = 1 / torch.sqrt(v64 + EPS)
    m32, v32 = x.mean(0), x.var(0, unbiased=False)
    i32 = 1 / torch.sqrt(v32 + EPS)
    beta, rm, rv, momentum = rnd(g, C), rnd(g, C), rnd(g, C).abs() + 0.1, 0.1
    t64 = T.bn_train_tail(m64, v64, i64, gamma, beta, rm, rv, momentum, rows)
    t32 = T.bn_train_tail(m32, v32, i32, gamma, beta, rm, rv, momentum, rows, F32)
    be = E(beta, dev)
    results = []
    for form in ("all", "act", "running", "none"):
        stats = [G((C,), F32, dev) for _ in range(3)]
        act = [G((C,), F32, dev) for _ in range(2)] if form in ("all", "act") else [None, None]
        run = [E(rm, dev), E(rv, dev)] if form in ("all", "running") else [None, None]
        tracked = E(torch.tensor([5], dtype=I64), dev) if form in ("all", "running") else None
        tail = None
        if form != "none":
            adr = lambda t: t.data_ptr() if t is not None else None
            tail = ctypes.byref(_lib.BnTrainTail(gamma=adr(ge), beta=adr(be), act_a=adr(act[0]), act_b=adr(act[1]), running_mean=adr(run[0]),
                                                 running_var=adr(run[1]), num_batches_tracked=adr(tracked), momentum=momentum))
        L("ptt_bn_finish_partials_train_f32", dev, P(pe), chunks, C, rows, EPS, *[P(o) for o in stats], tail)
        done(stats + [o for o in act if o is not None], [pe, ge, be] + [t for t in run + [tracked] if t is not None])
        for name, got, r64, r32 in zip(("mean", "var", "invstd"), stats, (m64, v64, i64), (m32, v32, i32)):
            bound("bn_finish_partials_train %s" % name, got, r64, r32)
        for k, (name, got) in enumerate(zip(("act_a", "act_b", "running_mean", "running_var"), act + run)):
            if got is not None:
                bound("bn_finish_partials_train %s" % name, got, t64[k], t32[k])
        if tracked is not None:
            assert int(tracked[0]) == 6, tag + ": num_batches_tracked"
        results.append(stats)
    for other in results[1:]:
        for a_, b_ in zip(results[0], other):
            same_bits(a_, b_, tag + ": the statistics do not depend on the tail")
    p = ops.bn_finish_partials(pe.contiguous(), rows, EPS)
    for a_, b_ in zip(results[3], p):
        same_bits(a_, b_, tag + " against ops.bn_finish_partials")


def test_bn_update_running(dev):
    """C = 257: two workgroups; count = 1: the n > 1 guard gives the factor 1; num_batches_tracked NULL."""
    C, momentum = 257, 0.1
    g = gen(C)
    mean, var, rm, rv = rnd(g, C), rnd(g, C).abs(), rnd(g, C), rnd(g, C).abs() + 0.1
    me, ve, ce = E(mean, dev), E(var, dev), E(torch.tensor([1.0], dtype=F64), dev)
    re_, rve = E(rm, dev), E(rv, dev)
    L("ptt_bn_update_running_f32", dev, P(me), P(ve), P(ce), momentum, C, P(re_), P(rve), None)
    done([], [me, ve, ce, re_, rve])
    t64 = T.bn_train_tail(mean, var, var, var, var, rm, rv, momentum, 1)
    t32 = T.bn_train_tail(mean, var, var, var, var, rm, rv, momentum, 1, F32)
    bound("bn_update_running running_mean", re_, t64[2], t32[2])
    bound("bn_update_running running_var", rve, t64[3], t32[3])
    tracked = E(torch.tensor([41], dtype=I64), dev)                        # and with the counter, as the module wrapper passes it
    L("ptt_bn_update_running_f32", dev, P(me), P(ve), P(ce), momentum, C, P(re_), P(rve), P(tracked))
    done([], [me, ve, ce, re_, rve, tracked])
    assert int(tracked[0]) == 42


# ======================================================================================================= pt_attn_train_bwd
@pytest.mark.parametrize("B,N,k,D", [(1, 1, 8, 4), (2, 17, 16, 132), (3, 33, 32, 64), (1, 40, 8, 512)])
def test_pt_attn_train_backward(dev, B, N, k, D):
    g = gen(N * 100 + k + D)
    scale = 0.37
    a, vf, pos, dres = rnd(g, B, N, k, D) * 3, rnd(g, B, N, D), rnd(g, B, N, k, D), rnd(g, B, N, D)
    knn = torch.randint(0, N, (B, N, k), generator=g).to(I32)
    knn[..., 1] = knn[..., 0]                                               # duplicates within a point
    hot = B * N > 1
    if hot:                                                                 # one point whose softmax is exactly one-hot in float32
        a[B - 1, N - 1] = -1000.0
        a[B - 1, N - 1, 3] = 0.0
    attn = ops.pt_attn_train_fwd(a.to(dev), vf.to(dev), knn.to(dev), pos.to(dev), scale)[0].cpu()
    if hot:
        assert bool((attn[B - 1, N - 1, 3] == 1).all()) and float(attn[B - 1, N - 1].sum()) == D
    ins = [E(t.view(B, N * k, D) if t.dim() == 4 else t, dev) for t in (attn, vf, knn, pos, dres)]
    tag = "pt_attn_train_bwd %s" % ((B, N, k, D),)

    def run():
        da, dvp = G((B, N * k, D), F32, dev), G((B, N * k, D), F32, dev)
        L("ptt_pt_attn_train_bwd_f32", dev, *[P(v) for v in ins], B, N, k, D, scale, P(da), P(dvp))
        done([da, dvp], ins)
        return da, dvp
    da, dvp = twice(run, tag)
    r64, r32 = T.attn_bwd(attn, vf, knn, pos, dres, scale), T.attn_bwd(attn, vf, knn, pos, dres, scale, F32)
    bound(tag + " da", da, r64[0].view(B, N * k, D), r32[0].view(B, N * k, D))
    bound(tag + " dvp", dvp, r64[1].view(B, N * k, D), r32[1].view(B, N * k, D))
    if hot:
        assert float(da.view(B, N, k, D)[B - 1, N - 1].abs().max()) == 0.0, tag + ": da of the one-hot point"
    p = ops.pt_attn_train_bwd(ins[0].contiguous().view(B, N, k, D), ins[1].contiguous(), ins[2].contiguous(), ins[3].contiguous().view(B, N, k, D),
                              ins[4].contiguous(), scale)
    same_bits(da, p[0], tag + " against ops.pt_attn_train_bwd (da)")
    same_bits(dvp, p[1], tag + " against ops.pt_attn_train_bwd (dvp)")


# ================================================================================================= unit_rows / cos_bwd_rows
COS_EPS = 1e-8


def cos_input(g, B, C, n):
    """(B,C,n): ordinary rows, (n > 1) one all-zero row, one non-zero row of norm 1e-10 < eps. With n = 1 there are two rows in
    all: one ordinary, one under the clamp."""
    x = rnd(g, B, C, n)
    if n > 1:
        x[0, :, 0] = 0.0
    x[1, :, n - 1] *= 1e-10 / float(x[1, :, n - 1].double().norm())
    return x


def both_layouts(x, dev):
    """x (B,C,n) -> (name, the (B,C,n) view the launch reads, the embedded tensor that owns it) in both layouts: channel-major, and a
    view of point-major rows."""
    cm, pm = E(x, dev), E(x.transpose(1, 2), dev)
    return (("channel-major", cm, cm), ("point-major", pm.transpose(1, 2), pm))


def strides_bnc(v):
    return v.stride(0), v.stride(2), v.stride(1)                   # (sb, sn, sc) of a (B,C,n) view


@pytest.mark.parametrize("C", [1, 63, 64, 65, 260])
@pytest.mark.parametrize("n", [1, 5])
def test_unit_rows(dev, C, n):
    B = 2
    x = cos_input(gen(C * 10 + n), B, C, n)
    eps32 = torch.tensor(COS_EPS, dtype=F32)
    u64, n64 = T.unit_rows(x, COS_EPS)
    u32, n32 = T.unit_rows(x, COS_EPS, F32)
    tag = "unit_rows (C %d, n %d)" % (C, n)
    first = None
    for name, view, owner in both_layouts(x, dev):
        def run():
            unit, nrm = G((B, n, C), F32, dev), G((B, n), F32, dev)
            L("ptt_unit_rows_f32", dev, P(view), *strides_bnc(view), B, n, C, COS_EPS, P(unit), P(nrm))
            done([unit, nrm], [owner])
            return unit, nrm
        unit, nrm = twice(run, "%s %s" % (tag, name))
        bound(tag + " unit", unit, u64, u32)
        bound(tag + " |nrm|", nrm.abs(), n64.abs(), n32.abs())
        assert torch.equal(torch.signbit(nrm.cpu()), torch.signbit(n64)), tag + ": the sign of nrm marks the clamp"
        got_n, got_u = nrm.cpu(), unit.cpu()
        assert float(got_n[1, n - 1]) == -float(eps32), tag + ": nrm of the row under the clamp is -eps"
        same_bits(got_u[1, n - 1], x[1, :, n - 1] / eps32, tag + ": unit of the row under the clamp is x / eps")
        if n > 1:
            assert float(got_n[0, 0]) == -float(eps32) and float(got_u[0, 0].abs().max()) == 0.0, tag + ": the all-zero row"
        p = ops.unit_rows_eps(view, COS_EPS)
        same_bits(unit, p[0], "%s %s against ops.unit_rows_eps" % (tag, name))
        same_bits(nrm, p[1], "%s %s against ops.unit_rows_eps (nrm)" % (tag, name))
        if first is None:
            first = (unit, nrm)
        else:
            same_bits(unit, first[0], tag + ": the two input layouts")
            same_bits(nrm, first[1], tag + ": the two input layouts (nrm)")


@pytest.mark.parametrize("C", [1, 63, 64, 65, 260])
@pytest.mark.parametrize("n", [1, 5])
def test_cos_bwd_rows(dev, C, n):
    B = 2
    g = gen(C * 10 + n + 7)
    x = cos_input(g, B, C, n)
    unit, nrm = (t.float() for t in T.unit_rows(x, COS_EPS))
    clamped = nrm < 0
    A = rnd(g, B, n, C)
    ue, ne, Ae = E(unit, dev), E(nrm, dev), E(A, dev)
    for m in (1, 63, 65, 130):
        for own_is_row in (True, False):
            n2, n1 = (n, m) if own_is_row else (m, n)
            Gm, cosm = rnd(g, B, n2, n1), torch.rand(B, n2, n1, generator=g, dtype=F32) * 2 - 1
            Ge, ce = E(Gm, dev), E(cosm, dev)
            own, other = (n1, 1) if own_is_row else (1, n1)
            r64 = T.cos_bwd_rows(A, unit, nrm, Gm, cosm, own_is_row)
            r32 = T.cos_bwd_rows(A, unit, nrm, Gm, cosm, own_is_row, F32)
            tag = "cos_bwd_rows (C %d, n %d, m %d, %s)" % (C, n, m, "rows" if own_is_row else "columns")
            first = None
            for name in ("channel-major", "point-major"):
                dx = G((B, C, n), F32, dev) if name == "channel-major" else G((B, n, C), F32, dev)
                view = dx if name == "channel-major" else dx.transpose(1, 2)
                L("ptt_cos_bwd_rows_f32", dev, P(Ae), P(ue), P(ne), P(Ge), P(ce), n2 * n1, own, other, m, B, n, C, P(view), *strides_bnc(view))
                done([dx], [Ae, ue, ne, Ge, ce])
                got = view.transpose(1, 2).cpu()                   # (B,n,C)
                # the rows under the clamp are 1e8 times larger than the others: each kind against its own largest value
                bound("cos_bwd_rows dx", got[~clamped], r64[~clamped], r32[~clamped])
                bound("cos_bwd_rows dx under the clamp", got[clamped], r64[clamped], r32[clamped])
                p = ops.cos_bwd_rows(Ae.contiguous(), ue.contiguous(), ne.contiguous(), Ge.contiguous(), ce.contiguous(), own_is_row,
                                     (tuple(view.shape), tuple(view.stride())))
                same_bits(view, p, "%s %s against ops.cos_bwd_rows" % (tag, name))
                if first is None:
                    first = got
                else:
                    same_bits(got, first, tag + ": the two output layouts")


def test_zz_ratio_report():
    """Not a check of its own: the err / Y table of the run (pytest -s), the source of R and of the table above."""
    worst = max(RATIOS.values()) if RATIOS else 0.0
    for k in sorted(RATIOS):
        print("REPORT %-60s %.2f" % (k, RATIOS[k]))
    print("REPORT worst err/Y %.2f over %d results; R = %g" % (worst, len(RATIOS), R_RATIO))
    assert worst <= R_RATIO
