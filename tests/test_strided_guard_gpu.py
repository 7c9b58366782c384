"""The row kernels on strided, offset and misaligned views, behind guard bands (tests/guard.py).

Every case runs an entry point of the C ABI twice, against one float64 reference computed with plain torch on the host:
  run A  dense operands (ld == C); outputs, statistics partials and workspaces in guarded buffers of exactly their size;
  run B  every operand that has a leading dimension embedded with ld > C, a column offset and NaN surroundings, every output
         guarded with a leading dimension of its own (operands get DIFFERENT lds: swapping two of them cannot cancel out).
and asserts, for both: (1) the values meet exactly the bound the op's existing contiguous test asserts (restated here with its
source line; no bound is new), (2) check_guard passes on every output, workspace and input, (3) where A and B take the same
code path — both float4-addressable or both not — B is bit-identical to A (the fixed summation order is a documented property
of these kernels, and a row stride must not change it).

Misaligned layouts (col_off = 1, or an odd ld) must either compute the right values through the scalar form or be refused with
the status the table REFUSALS names; a refusal that is not in the table fails the test, so a refusal can never hide a case that
should run. A refused launch must leave every output word untouched.

What this does not prove: a read past an input that does not influence the result goes unseen. NaN surroundings catch leaks
(a staged row too many times a zero weight is NaN), not every stray load. Nothing here measures speed.

Out of scope here: the index ops (no leading dimensions) are behind guard bands in tests/test_index_guard_gpu.py, the fused
SA / xcorr / pair kernels (their descriptors take whole tensors and output strides) in tests/test_fused_guard_gpu.py."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import guard
from tests.guard import check_guard, embed, guarded

pytestmark = pytest.mark.gpu
L, P = guard.launch, guard.ptr
F32, F64, I32 = torch.float32, torch.float64, torch.int32
EPS = 1e-5

# ------------------------------------------------------------------------------------------------------------------ layouts
# name -> (ld of operand number k with C channels, column offset). "strided" keeps float32 rows 16-byte aligned when C % 4 == 0,
# "off1" and "odd" never do.
LAYOUTS = {
    "dense": (lambda C, k: C, 0),
    "strided": (lambda C, k: C + 4 * (k + 1), 4),
    "off1": (lambda C, k: C + 4 * (k + 1), 1),
    "odd": (lambda C, k: C + 1 + 2 * k + (C % 2), 0),           # always odd
}


def put(t, dev, lay, k):
    """Input operand number k of a case in layout `lay`."""
    ld, off = LAYOUTS[lay]
    t = t.to(dev)
    return embed(t, ld=ld(t.shape[-1], k), col_off=off) if t.dim() >= 2 else embed(t)


def out(shape, dtype, dev, lay, k):
    ld, off = LAYOUTS[lay]
    return guarded(shape, dtype, ld=ld(shape[-1], k), col_off=off, device=dev) if len(shape) >= 2 else guarded(shape, dtype, device=dev)


def vec4(*views):
    """What vec4_ok (train_ops.hip) and its kin decide from: C % 4 == 0, ld % 4 == 0, a 16-byte aligned base."""
    return all(v.shape[-1] % 4 == 0 and v.stride(-2) % 4 == 0 and v.data_ptr() % 16 == 0 for v in views)


def host(*views):
    return tuple(v.detach().cpu().clone() for v in views)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def same_bits(a, b, what):
    for x, y, n in zip(a, b, what):
        assert x.dtype == y.dtype and torch.equal(x.view(I32) if x.dtype == F32 else x, y.view(I32) if y.dtype == F32 else y), \
            "%s: the strided run is not bit-identical to the dense one" % n


def checked(*views, inputs=()):
    for v in views:
        check_guard(v)
    for v in inputs:
        check_guard(v, all_written=False)


def ws_of(query, dev, *dims):
    from ptt_amd import ops
    n = int(ops._host(query, *dims))
    w = guard.workspace(n, device=dev)
    return w, n


# ------------------------------------------------------------------------------------------- the refusal table (misaligned views)
# (entry point, form) -> the status a view that is not float4-addressable (C % 4 != 0, ld % 4 != 0 or a base off 16 bytes) gets,
# or None: it runs through the scalar form. From include/ptt_hip.h and the argument checks of train_ops.hip:
REFUSALS = {
    "ptt_bn_stats_f32": None,                       # scalar form: col_stats_kernel<0> (train_ops.hip, ptt_bn_stats_train_f32)
    "ptt_bn_stats_train_f32": None,
    "ptt_bn_apply_f32": None,                       # bn_apply_kernel
    "ptt_bn_bwd_f32[Act]": None,                    # col_stats_kernel<1> + bn_bwd_apply_kernel
    "ptt_bn_bwd_f32[act_scale]": "PTT_EUNSUPPORTED",    # "the mask-from-z form needs C % 4 == 0 and 16-byte aligned rows"
    "ptt_bn_sums_f64": "PTT_EUNSUPPORTED",          # ptt_hip.h, SyncBatchNorm: "C % 4 == 0, 16-byte aligned rows" (vector form only)
    "ptt_bn_bwd_sums_f64": "PTT_EUNSUPPORTED",      # same paragraph
    "ptt_bn_bwd_apply_f32": "PTT_EUNSUPPORTED",     # same paragraph
    "ptt_bn_bwd_from_partials_f32": "PTT_EUNSUPPORTED",     # vec4_ok of every operand, "needs C % 4 == 0 and 16-byte aligned rows"
    "ptt_bn_bwd_pooled_f32": "PTT_EUNSUPPORTED",    # pooled_args_ok
    "ptt_bn_bwd_pooled_sums_f64": "PTT_EUNSUPPORTED",
    "ptt_bn_bwd_pooled_apply_f32": "PTT_EUNSUPPORTED",
    "ptt_pool_rows_f32": None,                      # one scalar kernel for every layout
    "ptt_pool_rows_bwd_f32": None,
    "ptt_colsum_f32": None,                         # colsum_partial_scalar_kernel (ptt_hip.h: float4 loads where the rows allow them)
}
PATHS = {}      # (entry, R, C, layout) -> "vector" | "scalar" | "refused": printed by test_zz_coverage_report


def attempt(entry, aligned, fn, outputs, key):
    """Run fn(); a view that is not float4-addressable must get exactly what REFUSALS says. -> True when the launch ran."""
    want = None if aligned else REFUSALS[entry]
    if want is None:
        fn()
        PATHS[(entry,) + key] = "vector" if aligned else "scalar"
        return True
    with pytest.raises(RuntimeError, match=want):
        fn()
    guard.assert_untouched(*outputs)                # refused before anything was launched
    PATHS[(entry,) + key] = "refused"
    return False


def classes(runs):
    """{layout: (aligned, results)} -> within each alignment class every run is bit-identical to the first one."""
    first = {}
    for lay, (aligned, res, names) in runs.items():
        if res is None:
            continue
        if aligned in first:
            same_bits(first[aligned][0], res, ["%s (%s vs %s)" % (n, lay, first[aligned][1]) for n in names])
        else:
            first[aligned] = (res, lay)


# ------------------------------------------------------------------------------------------------ BatchNorm training kernels
BN_SHAPES = [(1, 4), (255, 64), (257, 132), (2049, 4), (257, 1028), (255, 7), (2049, 7), (1, 132), (2049, 64)]


def bn_layouts(C):
    return ["dense", "strided"] + (["off1", "odd"] if C in (4, 64, 132) else [])


def bn_data(R, C):
    g = gen(1000 * R + C)
    z = torch.randn(R, C, generator=g) * 2 + torch.randn(C, generator=g) * 3
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.2
    up = torch.randn(R, C, generator=g)
    v64, m64 = torch.var_mean(z.double(), 0, unbiased=False)
    mean, invstd = m64.float(), (1.0 / torch.sqrt(v64 + EPS)).float()
    a = gamma * invstd
    b = beta - mean * a
    return dict(z=z, gamma=gamma, beta=beta, up=up, m64=m64, v64=v64, mean=mean, invstd=invstd, a=a, b=b)


@pytest.mark.parametrize("R,C", BN_SHAPES)
def test_bn_stats_and_sums(dev, R, C):
    """ptt_bn_stats_f32, ptt_bn_stats_train_f32 (with its tail), ptt_bn_sums_f64 + ptt_bn_finish_f64."""
    from ptt_amd import _lib
    d = bn_data(R, C)
    runs, runs_sums = {}, {}
    for lay in bn_layouts(C):
        x = put(d["z"], dev, lay, 0)
        key = (R, C, lay)
        mean, var, invstd = (guarded((C,), F32, device=dev) for _ in range(3))
        w, n = ws_of("ptt_bn_stats_workspace", dev, R, C)
        ran = attempt("ptt_bn_stats_f32", vec4(x), lambda: L("ptt_bn_stats_f32", dev, P(x), R, C, x.stride(0), EPS, P(mean), P(var), P(invstd), P(w), n),
                      (mean, var, invstd, w), key)
        assert ran
        checked(mean, var, invstd, inputs=(x, w))
        # bounds: tests/test_train_gpu.py:32-33
        torch.testing.assert_close(mean.cpu().double(), d["m64"], rtol=1e-6, atol=1e-6)
        torch.testing.assert_close(var.cpu().double(), d["v64"], rtol=1e-5, atol=1e-7)
        # the training form: the same statistics, the activation constants bit-equal to the element-wise expressions
        # (tests/test_gemm_gpu.py:101-102), the running statistics as torch's BatchNorm keeps them (:108-109)
        gam, bet = embed(d["gamma"].to(dev)), embed(d["beta"].to(dev))
        rm0, rv0 = torch.linspace(-1, 1, C), torch.linspace(0.5, 2, C)
        m2, v2, i2, aa, ab = (guarded((C,), F32, device=dev) for _ in range(5))
        rm, rv = embed(rm0.to(dev)), embed(rv0.to(dev))
        nbt = embed(torch.zeros(1, dtype=torch.int64).to(dev))
        w2, _ = ws_of("ptt_bn_stats_workspace", dev, R, C)
        tail = _lib.BnTrainTail(gamma=gam.data_ptr(), beta=bet.data_ptr(), act_a=aa.data_ptr(), act_b=ab.data_ptr(), running_mean=rm.data_ptr(),
                                running_var=rv.data_ptr(), num_batches_tracked=nbt.data_ptr(), momentum=0.1)
        if R > 1:                                   # the unbiased running variance divides by R - 1
            attempt("ptt_bn_stats_train_f32", vec4(x), lambda: L("ptt_bn_stats_train_f32", dev, P(x), R, C, x.stride(0), EPS, P(m2), P(v2), P(i2),
                                                                P(w2), n, ctypes.byref(tail)), (), key)
            checked(m2, v2, i2, aa, ab, inputs=(x, w2, gam, bet, rm, rv, nbt))
            same_bits(host(m2, v2, i2), host(mean, var, invstd), ("mean", "var", "invstd"))
            assert torch.equal(aa, gam * invstd) and torch.equal(ab, bet - mean * aa)
            assert int(nbt) == 1
            torch.testing.assert_close(rm.cpu(), 0.9 * rm0 + 0.1 * d["m64"].float(), rtol=1e-5, atol=1e-6)
            torch.testing.assert_close(rv.cpu(), 0.9 * rv0 + 0.1 * (d["v64"] * R / (R - 1)).float(), rtol=1e-5, atol=1e-6)
        runs[lay] = (vec4(x), host(mean, var, invstd, w), ("mean", "var", "invstd", "partials"))
        # SyncBatchNorm forward: 2C + 1 doubles, then the finish — the same bounds as the one-rank statistics
        sums = guarded((2 * C + 1,), F64, device=dev)
        w3, _ = ws_of("ptt_bn_stats_workspace", dev, R, C)
        if attempt("ptt_bn_sums_f64", vec4(x), lambda: L("ptt_bn_sums_f64", dev, P(x), R, C, x.stride(0), P(sums), P(w3), n), (sums, w3), key):
            checked(sums, inputs=(x, w3))
            assert float(sums[-1]) == float(R)
            m3, v3, i3 = (guarded((C,), F32, device=dev) for _ in range(3))
            L("ptt_bn_finish_f64", dev, P(sums), C, EPS, P(m3), P(v3), P(i3))
            checked(m3, v3, i3, inputs=(sums,))
            torch.testing.assert_close(m3.cpu().double(), d["m64"], rtol=1e-6, atol=1e-6)
            torch.testing.assert_close(v3.cpu().double(), d["v64"], rtol=1e-5, atol=1e-7)
            runs_sums[lay] = (True, host(sums, w3), ("sums", "partials"))
    classes(runs)
    classes(runs_sums)


@pytest.mark.parametrize("R,C", BN_SHAPES)
def test_bn_apply(dev, R, C):
    d = bn_data(R, C)
    ref = torch.relu((d["z"].double() - d["m64"]) / torch.sqrt(d["v64"] + EPS) * d["gamma"].double() + d["beta"].double())
    runs = {}
    vecs = [embed(d[k].to(dev)) for k in ("mean", "invstd", "gamma", "beta")]
    for lay in bn_layouts(C):
        z, x = put(d["z"], dev, lay, 0), out((R, C), F32, dev, lay, 1)
        attempt("ptt_bn_apply_f32", vec4(z, x), lambda: L("ptt_bn_apply_f32", dev, P(z), z.stride(0), *[P(v) for v in vecs], R, C, 1, P(x), x.stride(0)),
                (x,), (R, C, lay))
        checked(x, inputs=[z] + vecs)
        torch.testing.assert_close(x.cpu().double(), ref, rtol=1e-5, atol=1e-5)         # tests/test_train_gpu.py:36
        runs[lay] = (vec4(z, x), host(x), ("x",))
    classes(runs)


def bn_bwd_reference(d, masked_by_z):
    zz = d["z"].double().requires_grad_(True)
    gg, bb = d["gamma"].double().requires_grad_(True), d["beta"].double().requires_grad_(True)
    v, m = torch.var_mean(zz, 0, unbiased=False)
    pre = (zz - m) / torch.sqrt(v + EPS) * gg + bb
    if masked_by_z:         # the kernel's mask is fmaf(z, a, b) > 0 in float32: the sign of the exactly evaluated z * a + b
        mask = (d["z"].double() * d["a"].double() + d["b"].double()) > 0
        y = torch.where(mask, pre, torch.zeros_like(pre))
    else:
        y = torch.relu(pre)
    y.backward(d["up"].double())
    return zz.grad, gg.grad, bb.grad, torch.relu(pre).detach().float()


def bn_bwd_bounds(dz, dgamma, dbeta, ref):
    """tests/test_train_gpu.py:45-48"""
    rz, rg, rb = ref[:3]
    scale = float(rz.abs().max())
    assert float((dz.cpu().double() - rz).abs().max()) <= 2e-5 * scale + 1e-7
    torch.testing.assert_close(dgamma.cpu().double(), rg, rtol=1e-4, atol=1e-3 * float(rg.abs().max()) * 1e-1)
    torch.testing.assert_close(dbeta.cpu().double(), rb, rtol=1e-4, atol=1e-3 * float(rb.abs().max()) * 1e-1)


@pytest.mark.parametrize("form", ["Act", "act_scale"])
@pytest.mark.parametrize("R,C", BN_SHAPES)
def test_bn_bwd(dev, R, C, form):
    """ptt_bn_bwd_f32 with the stored activation and with the mask from z; out of place and with dZ aliasing G."""
    d = bn_data(R, C)
    by_z = form == "act_scale"
    if by_z and C % 4:
        # no layout of a C % 4 != 0 tensor is float4-addressable: the refusal is the whole case
        z, g = put(d["z"], dev, "dense", 0), put(d["up"], dev, "dense", 1)
        dz, dg, db = out((R, C), F32, dev, "dense", 3), guarded((C,), F32, device=dev), guarded((C,), F32, device=dev)
        w, n = ws_of("ptt_bn_stats_workspace", dev, R, C)
        vecs = [embed(d[k].to(dev)) for k in ("mean", "invstd", "gamma", "a", "b")]
        ran = attempt("ptt_bn_bwd_f32[act_scale]", False,
                      lambda: L("ptt_bn_bwd_f32", dev, P(g), g.stride(0), None, 0, P(z), z.stride(0), P(vecs[0]), P(vecs[1]), P(vecs[2]), R, C, 1, P(dz),
                                dz.stride(0), P(dg), P(db), P(w), n, P(vecs[3]), P(vecs[4])), (dz, dg, db, w), (R, C, "dense"))
        assert not ran
        return
    ref = bn_bwd_reference(d, by_z)
    act_host = ref[3]
    runs = {}
    for lay in bn_layouts(C):
        z, g = put(d["z"], dev, lay, 0), put(d["up"], dev, lay, 1)
        act = None if by_z else put(act_host, dev, lay, 2)
        mean, invstd, gamma, a, b = (embed(d[k].to(dev)) for k in ("mean", "invstd", "gamma", "a", "b"))
        res = []
        for inplace in (False, True):
            g_in = put(d["up"], dev, lay, 1)
            dz = g_in if inplace else out((R, C), F32, dev, lay, 3)
            dg, db = guarded((C,), F32, device=dev), guarded((C,), F32, device=dev)
            w, n = ws_of("ptt_bn_stats_workspace", dev, R, C)
            aligned = vec4(z, g_in, dz) and (act is None or vec4(act))
            ran = attempt("ptt_bn_bwd_f32[%s]" % form, aligned,
                          lambda: L("ptt_bn_bwd_f32", dev, P(g_in), g_in.stride(0), P(act), act.stride(0) if act is not None else 0, P(z), z.stride(0),
                                    P(mean), P(invstd), P(gamma), R, C, 1, P(dz), dz.stride(0), P(dg), P(db), P(w), n,
                                    P(a) if by_z else None, P(b) if by_z else None),
                          (dg, db, w) + (() if inplace else (dz,)), (R, C, lay + ("/in place" if inplace else "")))
            if not ran:
                break
            checked(dg, db, inputs=[z, w, mean, invstd, gamma] + ([act] if act is not None else []) + ([a, b] if by_z else []))
            check_guard(dz, all_written=not inplace)
            if not inplace:
                check_guard(g_in, all_written=False)
            bn_bwd_bounds(dz, dg, db, ref)
            res.append(host(dz, dg, db, w))
        if res:
            same_bits(res[0], res[1], ("dz in place", "dgamma in place", "dbeta in place", "partials in place"))
            runs[lay] = (aligned, res[0], ("dz", "dgamma", "dbeta", "partials"))
    assert "dense" in runs and "strided" in runs
    classes(runs)


@pytest.mark.parametrize("form", ["Act", "act_scale"])
@pytest.mark.parametrize("R,C", [s for s in BN_SHAPES if s[1] % 4 == 0])
def test_syncbn_backward_pieces(dev, R, C, form):
    """ptt_bn_bwd_sums_f64 -> (all-reduce) -> ptt_bn_bwd_apply_f32, out of place and with dZ aliasing G; and the same dz from the
    partials of a GEMM epilogue, ptt_bn_bwd_from_partials_f32 (fed here with the partials ptt_bn_bwd_sums_f64's first kernel left
    in the workspace: the same [chunk][2][C] layout)."""
    d = bn_data(R, C)
    by_z = form == "act_scale"
    ref = bn_bwd_reference(d, by_z)
    runs = {}
    for lay in bn_layouts(C):
        z, g = put(d["z"], dev, lay, 0), put(d["up"], dev, lay, 1)
        act = None if by_z else put(ref[3], dev, lay, 2)
        mean, invstd, gamma, a, b = (embed(d[k].to(dev)) for k in ("mean", "invstd", "gamma", "a", "b"))
        lda = act.stride(0) if act is not None else 0
        aligned = vec4(z, g) and (act is None or vec4(act))
        sums = guarded((2, C), F64, device=dev)
        w, n = ws_of("ptt_bn_stats_workspace", dev, R, C)
        key = (R, C, lay)
        ran = attempt("ptt_bn_bwd_sums_f64", aligned,
                      lambda: L("ptt_bn_bwd_sums_f64", dev, P(g), g.stride(0), P(act), lda, P(z), z.stride(0), P(mean), P(invstd), R, C, P(sums), P(w), n,
                                P(a) if by_z else None, P(b) if by_z else None), (sums, w), key)
        dz_dummy = out((R, C), F32, dev, lay, 3)
        s32 = embed(torch.zeros(2, C).to(dev)) if not ran else embed(sums.float().contiguous())
        count = embed(torch.full((1,), float(R), dtype=F64).to(dev))
        if not ran:
            assert not attempt("ptt_bn_bwd_apply_f32", False,
                               lambda: L("ptt_bn_bwd_apply_f32", dev, P(g), g.stride(0), P(act), lda, P(z), z.stride(0), P(mean), P(invstd), P(gamma),
                                         s32[0].data_ptr(), s32[1].data_ptr(), P(count), R, C, P(dz_dummy), dz_dummy.stride(0),
                                         P(a) if by_z else None, P(b) if by_z else None), (dz_dummy,), key)
            if by_z:
                part = embed(torch.zeros(1, 2, C, dtype=F64).to(dev))
                dg, db = guarded((C,), F32, device=dev), guarded((C,), F32, device=dev)
                assert not attempt("ptt_bn_bwd_from_partials_f32", False,
                                   lambda: L("ptt_bn_bwd_from_partials_f32", dev, P(part), 1, P(g), g.stride(0), P(z), z.stride(0), P(mean), P(invstd),
                                             P(gamma), R, C, P(dz_dummy), dz_dummy.stride(0), P(dg), P(db), P(a), P(b)), (dz_dummy, dg, db), key)
            continue
        checked(sums, inputs=[z, g, w, mean, invstd] + ([act] if act is not None else []))
        # the sums are dbeta / dgamma: tests/test_train_gpu.py:47-48
        for got, want in ((sums[1], ref[1]), (sums[0], ref[2])):
            torch.testing.assert_close(got.cpu(), want, rtol=1e-4, atol=1e-3 * float(want.abs().max()) * 1e-1)
        res = []
        for inplace in (False, True):
            g_in = put(d["up"], dev, lay, 1)
            dz = g_in if inplace else out((R, C), F32, dev, lay, 3)
            attempt("ptt_bn_bwd_apply_f32", True,
                    lambda: L("ptt_bn_bwd_apply_f32", dev, P(g_in), g_in.stride(0), P(act), lda, P(z), z.stride(0), P(mean), P(invstd), P(gamma),
                              s32[0].data_ptr(), s32[1].data_ptr(), P(count), R, C, P(dz), dz.stride(0), P(a) if by_z else None, P(b) if by_z else None),
                    (), (R, C, lay + ("/in place" if inplace else "")))
            check_guard(dz, all_written=not inplace)
            checked(inputs=[z, s32, count, gamma, g_in])
            scale = float(ref[0].abs().max())
            assert float((dz.cpu().double() - ref[0]).abs().max()) <= 2e-5 * scale + 1e-7           # tests/test_train_gpu.py:46
            res.append(host(dz))
        same_bits(res[0], res[1], ("dz in place",))
        got = [res[0][0], sums.cpu().clone(), w.cpu().clone()]
        names = ["dz", "sums", "partials"]
        if by_z:
            chunks = (R + 255) // 256               # ST4_ROWS: the chunks col_stats4_kernel<1> wrote into the workspace
            dz2, dg, db = out((R, C), F32, dev, lay, 4), guarded((C,), F32, device=dev), guarded((C,), F32, device=dev)
            attempt("ptt_bn_bwd_from_partials_f32", True,
                    lambda: L("ptt_bn_bwd_from_partials_f32", dev, P(w), chunks, P(g), g.stride(0), P(z), z.stride(0), P(mean), P(invstd), P(gamma), R, C,
                              P(dz2), dz2.stride(0), P(dg), P(db), P(a), P(b)), (), key)
            checked(dz2, dg, db, inputs=[w, g, z])
            bn_bwd_bounds(dz2, dg, db, ref)
            got += list(host(dz2, dg, db))
            names += ["dz from partials", "dgamma", "dbeta"]
        runs[lay] = (True, tuple(got), names)
    classes(runs)


# ------------------------------------------------------------------------------------------------------------- max-pooling
POOL_CASES = [(3, ns, C) for ns in (1, 16, 64) for C in (4, 33)]


def pool_data(G, ns, C):
    g = gen(G * 100 + ns * 7 + C)
    x = torch.randn(G * ns, C, generator=g)
    x[0:ns, 0] = 1.5                                    # ties inside a group: the first row wins (tests/test_train_gpu.py:85)
    up = torch.randn(G, C, generator=g)
    return x, up


@pytest.mark.parametrize("G,ns,C", POOL_CASES)
def test_pool_rows_forward_and_backward(dev, G, ns, C):
    x, up = pool_data(G, ns, C)
    a, b = torch.linspace(-1.0, 1.5, C), torch.linspace(0.3, -0.3, C)
    runs = {}
    for lay in ["dense", "strided", "off1", "odd"]:
        res = []
        for deferred in (False, True):
            # the kernel's fmaf(x, a, b) is the exactly evaluated x * a + b rounded once: float64 holds that sum
            src = (x.double() * a.double() + b.double()).float().clamp_min(0) if deferred else x
            ref, ridx = src.view(G, ns, C).max(dim=1)
            xv, o, arg = put(x, dev, lay, 0), out((G, C), F32, dev, lay, 1), guarded((G, C), I32, device=dev)
            av, bv = embed(a.to(dev)), embed(b.to(dev))
            attempt("ptt_pool_rows_f32", False, lambda: L("ptt_pool_rows_f32", dev, P(xv), xv.stride(0), G, ns, C, P(o), o.stride(0), P(arg),
                                                                P(av) if deferred else None, P(bv) if deferred else None), (o, arg), (G * ns, C, lay))
            checked(o, arg, inputs=(xv, av, bv))
            assert torch.equal(o.cpu(), ref)                                           # tests/test_train_gpu.py:88
            if not deferred:
                assert int(arg[0, 0]) == 0                                             # :89
            assert torch.equal(arg.cpu().long(), (src.view(G, ns, C) == ref[:, None, :]).float().argmax(dim=1))         # the FIRST arg-max
            assert bool(((arg >= 0) & (arg < ns)).all())
            res += list(host(o, arg))
        upv, dx = put(up, dev, lay, 2), out((G * ns, C), F32, dev, lay, 3)
        argd = embed(torch.from_numpy(np.ascontiguousarray(res[1].numpy())).to(dev))
        attempt("ptt_pool_rows_bwd_f32", False, lambda: L("ptt_pool_rows_bwd_f32", dev, P(upv), upv.stride(0), P(argd), G, ns, C, P(dx), dx.stride(0)),
                (dx,), (G * ns, C, lay))
        checked(dx, inputs=(upv, argd))
        dxh = dx.cpu().view(G, ns, C)
        assert torch.equal(dxh.sum(1), up) and int((dxh != 0).sum()) <= G * C           # tests/test_train_gpu.py:93
        assert torch.equal(torch.gather(dxh, 1, res[1].long()[:, None, :])[:, 0], up)
        runs[lay] = (True, tuple(res) + host(dx), ("pooled", "arg", "pooled (deferred)", "arg (deferred)", "dx"))     # one kernel: one class
    classes(runs)


@pytest.mark.parametrize("G,ns,C", [(3, 1, 4), (3, 16, 4), (3, 64, 4), (5, 16, 132), (40, 64, 64), (3, 16, 33)])
def test_bn_bwd_pooled(dev, G, ns, C):
    """ptt_bn_bwd_pooled_f32 / _sums_f64 / _apply_f32 (ldp, ldz, ldd) against pool backward + BatchNorm backward in float64."""
    R = G * ns
    d = bn_data(R, C)
    act = torch.relu(d["z"] * d["a"] + d["b"])
    arg = act.view(G, ns, C).max(dim=1)[1].int()
    up = torch.randn(G, C, generator=gen(R + C))
    dense_up = torch.zeros(G, ns, C).scatter_(1, arg.long()[:, None, :], up[:, None, :]).view(R, C)
    d["up"] = dense_up
    ref = bn_bwd_reference(d, True)
    runs = {}
    for lay in ["dense", "strided", "off1", "odd"]:
        z, dp, argv = put(d["z"], dev, lay, 0), put(up, dev, lay, 1), embed(arg.to(dev))
        mean, invstd, gamma, a, b = (embed(d[k].to(dev)) for k in ("mean", "invstd", "gamma", "a", "b"))
        dz, dg, db = out((R, C), F32, dev, lay, 2), guarded((C,), F32, device=dev), guarded((C,), F32, device=dev)
        w, n = ws_of("ptt_bn_stats_workspace", dev, R, C)
        aligned = vec4(z, dp, dz)
        key = (R, C, lay)
        ran = attempt("ptt_bn_bwd_pooled_f32", aligned,
                      lambda: L("ptt_bn_bwd_pooled_f32", dev, P(dp), dp.stride(0), P(argv), ns, P(z), z.stride(0), P(mean), P(invstd), P(gamma), R, C,
                                P(dz), dz.stride(0), P(dg), P(db), P(w), n, P(a), P(b)), (dz, dg, db, w), key)
        sums = guarded((2, C), F64, device=dev)
        w2, _ = ws_of("ptt_bn_stats_workspace", dev, R, C)
        ran2 = attempt("ptt_bn_bwd_pooled_sums_f64", aligned,
                       lambda: L("ptt_bn_bwd_pooled_sums_f64", dev, P(dp), dp.stride(0), P(argv), ns, P(z), z.stride(0), P(mean), P(invstd), R, C, P(sums),
                                 P(w2), n, P(a), P(b)), (sums, w2), key)
        s32 = embed(sums.float().contiguous()) if ran2 else embed(torch.zeros(2, C).to(dev))
        count = embed(torch.full((1,), float(R), dtype=F64).to(dev))
        dz3 = out((R, C), F32, dev, lay, 3)
        ran3 = attempt("ptt_bn_bwd_pooled_apply_f32", aligned,
                       lambda: L("ptt_bn_bwd_pooled_apply_f32", dev, P(dp), dp.stride(0), P(argv), ns, P(z), z.stride(0), P(mean), P(invstd), P(gamma),
                                 s32[0].data_ptr(), s32[1].data_ptr(), P(count), R, C, P(dz3), dz3.stride(0), P(a), P(b)), (dz3,), key)
        assert ran == ran2 == ran3 == aligned
        if not ran:
            continue
        checked(dz, dg, db, sums, dz3, inputs=[z, dp, argv, w, w2, mean, invstd, gamma, a, b, s32, count])
        # tests/test_train_gpu.py:503-506 hold it to the two-step kernels at 2e-6 / 1e-5; the float64 reference's own bound for that
        # two-step form is :45-48 — the weaker of the two existing bounds is what a float64 comparison can assert
        bn_bwd_bounds(dz, dg, db, ref)
        scale = float(ref[0].abs().max())
        assert float((dz3 - dz).abs().max()) <= 1e-6 * scale                              # tests/test_train_gpu.py:513
        runs[lay] = (True, host(dz, dg, db, w, sums, dz3), ("dz", "dgamma", "dbeta", "partials", "sums", "dz (apply)"))
    assert (C % 4 == 0) == ("dense" in runs)
    classes(runs)


# ------------------------------------------------------------------------------------------------------------------ colsum
@pytest.mark.parametrize("R,C", [(1, 4), (255, 64), (257, 132), (2049, 4), (300, 1028), (2049, 7), (9000, 64)])
def test_colsum(dev, R, C):
    from ptt_amd import ops
    x = torch.randn(R, C, generator=gen(R + C))
    ref = x.double().sum(0)
    bound = 2e-6 * float(x.abs().double().sum(0).max())                                   # tests/test_step_ops_gpu.py:163
    runs = {}
    for lay in bn_layouts(C):
        res = []
        for partials in (False, True):
            xv, o = put(x, dev, lay, 0), guarded((C,), F32, device=dev)
            w, n = ws_of("ptt_colsum_workspace", dev, R, C)
            if partials:
                nch = ctypes.c_int(0)
                attempt("ptt_colsum_f32", vec4(xv), lambda: L("ptt_colsum_partials_f32", dev, P(xv), R, C, xv.stride(0), P(w), n, ctypes.byref(nch)), (w,),
                        (R, C, lay + "/partials"))
                assert nch.value * C * 4 == n                                             # the query is exact
                check_guard(w)
                got = w.view(F32).view(nch.value, C).double().sum(0).cpu()
            else:
                attempt("ptt_colsum_f32", vec4(xv), lambda: L("ptt_colsum_f32", dev, P(xv), R, C, xv.stride(0), P(o), P(w), n), (o, w), (R, C, lay))
                checked(o, inputs=(w,))
                got = o.cpu().double()
            check_guard(xv, all_written=False)
            assert float((got - ref).abs().max()) <= bound
            res += list(host(o if not partials else w))
        runs[lay] = (vec4(xv), tuple(res), ("colsum", "partials"))
    classes(runs)
    assert ops._host("ptt_colsum_workspace", R, C) > 0


# ------------------------------------------------------------------------------------------- persistent row GEMM (gemm_ops.hip)
# (K, N) -> the tile rows of its geometry class (rows_gemm_geom): 64-row tiles with KC 128, 128-row tiles with RT 4, 128-row
# tiles of two wave rows; (128, 1536) x 5505 rows: 87 tiles x 6 column groups >= 2 x 256 CUs, the two-column-tile form (CT 2)
GEMM_GEOM = [(128, 128, 64), (64, 128, 128), (64, 64, 128)]
GEMM_CASES = [(r, K, N) for K, N, TR in GEMM_GEOM for r in (17, TR + 1, 3 * TR + 5)] + [(5505, 128, 1536)]
# layout -> (pad, column offset) of X, of out, of residual / mask / z
GEMM_LAYOUTS = {"dense": ((0, 0), (0, 0), (0, 0)), "strided": ((4, 4), (4, 4), (8, 4)), "strided, ldo = N + 3": ((4, 4), (3, 1), (8, 4))}


def gput(t, dev, pad_off, rows_around=128):
    """A GEMM operand with whole tiles of NaN rows in front of and behind it (a staged tile that reads a row too many meets them)."""
    pad, off = pad_off
    ld = t.shape[-1] + pad
    return embed(t.to(dev), ld=ld, col_off=off, lead=rows_around * ld, tail=rows_around * ld)


def gout(shape, dev, pad_off, dtype=F32):
    pad, off = pad_off
    return guarded(shape, dtype, ld=shape[-1] + pad, col_off=off, device=dev)


def gemm_data(R, K, N):
    g = gen(R + K + N)
    d = dict(x=torch.randn(R, K, generator=g), w=torch.randn(N, K, generator=g) / K ** 0.5, a=torch.rand(K, generator=g) + 0.5,
             b=torch.randn(K, generator=g) * 0.3, bias=torch.randn(N, generator=g), res=torch.randn(R, N, generator=g),
             mask=torch.randn(R, N, generator=g), zp=torch.randn(R, N, generator=g))
    d["ref"] = d["x"].double() @ d["w"].double().t()
    d["xact"] = torch.relu(d["x"].double() * d["a"].double() + d["b"].double())
    return d


def stats_of(part, chunks, N, rows):
    """(mean, var) from a guarded 1-D buffer of chunks * 2 * N doubles — ptt_bn_finish_partials_f32."""
    from ptt_amd import ops
    mean, var, _ = ops.bn_finish_partials(part.view(chunks, 2, N), rows, EPS)
    return mean, var


@pytest.mark.parametrize("R,K,N", GEMM_CASES)
def test_rows_gemm(dev, R, K, N):
    """ptt_rows_gemm_f32 (plain + statistics, deferred input activation, bias + ReLU + residual), _masked_f32, _bnbwd_f32."""
    from ptt_amd import ops
    d = gemm_data(R, K, N)
    wp = ops.pack_weight(d["w"].to(dev))
    chunks = int(ops._host("ptt_rows_gemm_stat_chunks", R, K, N))
    assert chunks > 0
    a, b, bias = embed(d["a"].to(dev)), embed(d["b"].to(dev)), embed(d["bias"].to(dev))
    mp, ip, ap, bp = (embed(t.to(dev)) for t in (torch.zeros(N), torch.ones(N), torch.ones(N), torch.zeros(N)))
    ref, rmax = d["ref"], float(d["ref"].abs().max())
    first = None
    for lay, (lx, lo, lr) in GEMM_LAYOUTS.items():
        x = gput(d["x"], dev, lx)
        assert ops._host("ptt_rows_gemm_supported", R, K, N, x.stride(0), N + lo[0]) == 1
        new_stats = lambda: guarded((chunks * 2 * N,), F64, device=dev)
        # plain, with statistics: the NaN rows behind the last row of X reach neither the partials nor the output
        y, st = gout((R, N), dev, lo), new_stats()
        L("ptt_rows_gemm_f32", dev, P(x), R, K, x.stride(0), None, None, P(wp), N, None, 0, None, N, P(y), y.stride(0), P(st), st.numel())
        checked(y, st, inputs=(x,))
        assert float((y.cpu().double() - ref).abs().max()) <= 3e-6 * rmax                  # tests/test_gemm_gpu.py:29
        mean, var = stats_of(st, chunks, N, R)
        v64, m64 = torch.var_mean(y.double(), 0, unbiased=False)
        assert float((mean.double() - m64).abs().max()) <= 1e-6                            # :32
        assert float(((var.double() - v64) / v64).abs().max()) <= 3e-6                     # :33
        # deferred activation on the input + bias + ReLU + residual
        res, y3 = gput(d["res"], dev, lr), gout((R, N), dev, lo)
        L("ptt_rows_gemm_f32", dev, P(x), R, K, x.stride(0), P(a), P(b), P(wp), N, P(bias), 1, P(res), res.stride(0), P(y3), y3.stride(0), None, 0)
        checked(y3, inputs=(x, res, a, b, bias))
        ref3 = torch.relu(d["xact"] @ d["w"].double().t() + d["bias"].double()) + d["res"].double()
        assert float((y3.cpu().double() - ref3).abs().max()) <= 2e-6 * float(ref3.abs().max())      # :51
        # deferred activation + statistics: rows past the end are not zeros inside the kernel, the statistics must not see them
        y4, st4 = gout((R, N), dev, lo), new_stats()
        L("ptt_rows_gemm_f32", dev, P(x), R, K, x.stride(0), P(a), P(b), P(wp), N, None, 0, None, N, P(y4), y4.stride(0), P(st4), st4.numel())
        checked(y4, st4, inputs=(x,))
        m4, v4 = stats_of(st4, chunks, N, R)
        v64d, m64d = torch.var_mean(y4.double(), 0, unbiased=False)
        assert float((m4.double() - m64d).abs().max()) <= 1e-6 and float(((v4.double() - v64d) / v64d).abs().max()) <= 3e-6    # :56
        # the ReLU-backward epilogue and its column sums
        mask, ym, stm = gput(d["mask"], dev, lr), gout((R, N), dev, lo), new_stats()
        L("ptt_rows_gemm_masked_f32", dev, P(x), R, K, x.stride(0), P(wp), N, P(mask), mask.stride(0), P(ym), ym.stride(0), P(stm), stm.numel())
        checked(ym, stm, inputs=(x, mask))
        refm = torch.where(d["mask"].double() > 0, ref, torch.zeros_like(ref))
        assert float((ym.cpu().double() - refm).abs().max()) <= 3e-6 * rmax                # :61
        colsum = ops.bn_sums_partials(stm.view(chunks, 2, N), R)[:N].float()
        assert float((colsum.cpu().double() - refm.sum(0)).abs().max()) <= 2e-5 * float(refm.abs().sum(0).max())       # :62
        # the BatchNorm-backward sums of the producing layer out of the epilogue (ldz)
        zp, yb, stb = gput(d["zp"], dev, lr), gout((R, N), dev, lo), new_stats()
        L("ptt_rows_gemm_bnbwd_f32", dev, P(x), R, K, x.stride(0), P(wp), N, P(zp), zp.stride(0), P(mp), P(ip), P(ap), P(bp), P(yb), yb.stride(0),
          P(stb), stb.numel())
        checked(yb, stb, inputs=(x, zp))
        assert float((yb.cpu().double() - ref).abs().max()) <= 2e-6 * rmax                 # tests/test_round5_gpu.py:260
        dy = torch.where(zp > 0, yb, torch.zeros_like(yb)).double()
        sums = stb.view(chunks, 2, N).sum(0)
        assert float((sums[0] - dy.sum(0)).abs().max()) <= 1e-6 * float(dy.abs().sum(0).max())                         # :264
        assert float((sums[1] - (dy * zp.double()).sum(0)).abs().max()) <= 1e-6 * float((dy * zp.double()).abs().sum(0).max())   # :265
        got = host(y, st, y3, y4, st4, ym, stm, yb, stb)
        if first is None:
            first = got
        else:           # one code path for every supported layout
            same_bits(first, got, ["%s (%s)" % (n, lay) for n in ("y", "stats", "y3", "y4", "stats4", "masked", "masked stats", "bnbwd", "bnbwd sums")])
        PATHS[("ptt_rows_gemm_f32 / _masked / _bnbwd", R, K, N, lay)] = "vector"
    # ldx % 4 != 0 is refused: by the query and by the launch, which writes nothing
    xo = embed(d["x"].to(dev), ld=K + 3)
    y = gout((R, N), dev, (0, 0))
    assert ops._host("ptt_rows_gemm_supported", R, K, N, K + 3, N) == 0
    with pytest.raises(RuntimeError, match="PTT_EUNSUPPORTED"):
        L("ptt_rows_gemm_f32", dev, P(xo), R, K, K + 3, None, None, P(wp), N, None, 0, None, N, P(y), N, None, 0)
    guard.assert_untouched(y)
    PATHS[("ptt_rows_gemm_f32", R, K, N, "ldx = K + 3")] = "refused"


@pytest.mark.parametrize("G,K,N,ns", [(5, 128, 128, 16), (7, 128, 128, 32), (3, 128, 256, 64), (5, 64, 128, 32), (86, 128, 1536, 64)])
def test_rows_gemm_pool_and_pool_select(dev, G, K, N, ns):
    """ptt_rows_gemm_pool_f32 + ptt_pool_select_f32 against ptt_rows_gemm_f32 + ptt_pool_rows_f32, bit for bit
    (tests/test_gemm_gpu.py:196-205), dense and strided; z against float64."""
    from ptt_amd import ops
    R = G * ns
    d = gemm_data(R, K, N)
    d["x"][5::7] = d["x"][3::7][:d["x"][5::7].shape[0]]                 # duplicated rows: ties inside groups (:185)
    xact = torch.relu(d["x"].double() * d["a"].double() + d["b"].double())
    ref = xact @ d["w"].double().t()
    g = gen(R)
    sa = torch.randn(N, generator=g)
    sa[::5] = 0.0
    sb = torch.randn(N, generator=g) * 0.3
    wp = ops.pack_weight(d["w"].to(dev))
    chunks = int(ops._host("ptt_rows_gemm_stat_chunks", R, K, N))
    a, b, sav, sbv = (embed(t.to(dev)) for t in (d["a"], d["b"], sa, sb))
    first = None
    for lay, (lx, lo, _) in GEMM_LAYOUTS.items():
        x = gput(d["x"], dev, lx)
        assert ops._host("ptt_rows_gemm_pool_supported", R, K, N, x.stride(0), ns) == 1
        z0, st0 = gout((R, N), dev, lo), guarded((chunks * 2 * N,), F64, device=dev)
        L("ptt_rows_gemm_f32", dev, P(x), R, K, x.stride(0), P(a), P(b), P(wp), N, None, 0, None, N, P(z0), z0.stride(0), P(st0), st0.numel())
        z1, st1 = gout((R, N), dev, lo), guarded((chunks * 2 * N,), F64, device=dev)
        pmax, pmin = guarded((G, N), F32, device=dev), guarded((G, N), F32, device=dev)
        amax, amin = guarded((G, N), I32, device=dev), guarded((G, N), I32, device=dev)
        L("ptt_rows_gemm_pool_f32", dev, P(x), R, K, x.stride(0), P(a), P(b), P(wp), N, P(z1), z1.stride(0), P(st1), st1.numel(), ns,
          P(pmax), P(pmin), P(amax), P(amin))
        checked(z0, st0, z1, st1, pmax, pmin, amax, amin, inputs=(x, a, b))
        assert float((z1.cpu().double() - ref).abs().max()) <= 3e-6 * float(ref.abs().max())         # tests/test_gemm_gpu.py:29
        same_bits(host(z0, st0), host(z1, st1), ("z", "stats"))                                       # :196
        p0, arg0 = gout((G, N), dev, lo), guarded((G, N), I32, device=dev)
        L("ptt_pool_rows_f32", dev, P(z0), z0.stride(0), G, ns, N, P(p0), p0.stride(0), P(arg0), P(sav), P(sbv))
        p1, arg1 = guarded((G, N), F32, device=dev), guarded((G, N), I32, device=dev)
        L("ptt_pool_select_f32", dev, P(pmax), P(pmin), P(amax), P(amin), P(sav), P(sbv), G, N, P(p1), P(arg1))
        checked(p0, arg0, p1, arg1, inputs=(pmax, pmin, amax, amin, z0))
        assert torch.equal(p0, p1)                                                                    # :199
        zc = z1.contiguous()
        act = torch.relu(zc * sav + sbv).view(G, ns, N)
        picked = act.gather(1, arg1.long().unsqueeze(1)).squeeze(1)
        assert torch.equal(picked, act.max(dim=1)[0])                                                 # :202
        pos = sav > 0
        firstrow = (zc.view(G, ns, N) == pmax.unsqueeze(1)).float().argmax(dim=1)
        assert torch.equal(arg1[:, pos], firstrow[:, pos].int())                                      # :205
        got = host(z1, st1, pmax, pmin, amax, amin, p1, arg1)
        if first is None:
            first = got
        else:
            same_bits(first, got, ["%s (%s)" % (n, lay) for n in ("z", "stats", "pmax", "pmin", "amax", "amin", "pooled", "arg")])
        PATHS[("ptt_rows_gemm_pool_f32 + ptt_pool_select_f32", R, K, N, "ns=%d" % ns, lay)] = "vector"


@pytest.mark.parametrize("R,K,N,hd", [(16, 128, 128, 0), (80, 128, 256, 0), (208, 256, 128, 0), (5504, 128, 1536, 0),
                                      (16, 256, 256, 128), (80, 512, 512, 256), (208, 256, 256, 128), (5504, 1536, 1536, 256)])
def test_rows_gemm_rsum16(dev, R, K, N, hd):
    """ptt_rows_gemm_rsum16_f32 and (hd > 0) ptt_rows_gemm_rsum16_heads_f32: ldx, ldr, ldo, ldp, ldg all different."""
    from ptt_amd import ops
    g = gen(R + K + hd)
    x, res = torch.randn(R, K, generator=g), torch.randn(R, N, generator=g) * 100.0
    w = torch.randn(hd or N, hd or K, generator=g) / (hd or K) ** 0.5
    if hd:
        want = torch.cat([x[:, h * hd:(h + 1) * hd].double() @ w.double().t() for h in range(K // hd)], 1)
    else:
        want = x.double() @ w.double().t()
    wsum = want.view(R // 16, 16, N).sum(1)
    wp = ops.pack_weight(w.to(dev))
    first = None
    for lay, lds in (("dense", [(0, 0)] * 5), ("strided", [(4, 4), (8, 4), (4, 0), (12, 8), (16, 4)]), ("strided, odd outputs", [(4, 4), (8, 4), (3, 1), (5, 2), (7, 3)])):
        xv, rv = gput(x, dev, lds[0]), gput(res, dev, lds[1])
        o, plain, gsum = gout((R, N), dev, lds[2]), gout((R, N), dev, lds[3]), gout((R // 16, N), dev, lds[4])
        if hd:
            assert ops._host("ptt_rows_gemm_rsum16_heads_supported", R, K, hd, xv.stride(0)) == 1
            L("ptt_rows_gemm_rsum16_heads_f32", dev, P(xv), R, K, hd, xv.stride(0), P(wp), P(rv), rv.stride(0), P(o), o.stride(0), P(plain),
              plain.stride(0), P(gsum), gsum.stride(0))
        else:
            assert ops._host("ptt_rows_gemm_rsum16_supported", R, K, N, xv.stride(0)) == 1
            L("ptt_rows_gemm_rsum16_f32", dev, P(xv), R, K, xv.stride(0), P(wp), N, P(rv), rv.stride(0), P(o), o.stride(0), P(plain), plain.stride(0),
              P(gsum), gsum.stride(0))
        checked(o, plain, gsum, inputs=(xv, rv))
        assert float((plain.cpu().double() - want).abs().max()) < 2e-6 * float(want.abs().max())     # tests/test_attn_core_gpu.py:19
        assert torch.equal(o, plain + rv)                                                             # :20
        assert float((gsum.cpu().double() - wsum).abs().max()) < 2e-6 * float(wsum.abs().max())      # :22
        got = host(plain, o, gsum)
        if first is None:
            first = got
        else:
            same_bits(first, got, ["%s (%s)" % (n, lay) for n in ("plain", "out", "gsum")])
        PATHS[("ptt_rows_gemm_rsum16%s_f32" % ("_heads" if hd else ""), R, K, N, lay)] = "vector"
    assert ops._host("ptt_rows_gemm_rsum16_supported", R + 8, K, N, K) == 0                           # not whole groups of 16 rows (:25)


# --------------------------------------------------------------------------------------------------------- weight gradients
# 767 / 769 rows straddle PTT_WG2_MIN_ROWS = 768 (a row chunk of the 256 x 256-block kernel; that kernel itself starts at 2048 rows:
# below, ptt_linear_wgrad2_f32 must refuse and ptt_linear_wgrad_f32 runs); (1000, 64, 3) the small-K form; (65537, 64, 64) the
# streaming form, dense AND strided (wgrad_stream_ok asks nothing of the leading dimensions but R * ld < 2^29)
# None of these reaches ptt_linear_wgrad2_f32 (its geometry wants enough 768-row chunks to fill half the chip: at (2500, 512, 512)
# the query returns 0 and ops.linear_wgrad takes ptt_linear_wgrad_f32); (5377, 512, 512) is the smallest 512 x 512 shape that
# does: 8 chunks of 768 rows, the last one a single row, 16 blocks of 128 x 128 outputs each.
WGRAD_CASES = [(767, 256, 256), (769, 128, 256), (2500, 512, 512), (300, 5, 256), (1000, 64, 3), (65537, 64, 64), (5377, 512, 512)]


@pytest.mark.parametrize("R,Cout,Cin", WGRAD_CASES)
def test_linear_wgrad(dev, R, Cout, Cin):
    from ptt_amd import ops
    g = gen(R)
    dz, x = torch.randn(R, Cout, generator=g), torch.randn(R, Cin, generator=g)
    a, b = torch.rand(Cin, generator=g) + 0.5, torch.randn(Cin, generator=g) * 0.3
    ref = dz.double().t() @ x.double()
    ref2 = dz.double().t() @ torch.relu(x.double() * a.double() + b.double())
    av, bv = embed(a.to(dev)), embed(b.to(dev))
    nb2 = int(ops._host("ptt_linear_wgrad2_workspace", R, Cout, Cin))
    two = nb2 > 0
    assert two == (R == 5377) and (not two or (R >= 2048 and Cout % 128 == 0 and Cin % 128 == 0))
    entry = "ptt_linear_wgrad2" if two else "ptt_linear_wgrad"
    nbytes = nb2 if two else int(ops._host("ptt_linear_wgrad_workspace", R, Cout, Cin))
    if two:
        bound = lambda r: 2e-6 * float(r.abs().max()) + 1e-6 * np.sqrt(R)                    # tests/test_gemm_gpu.py:73,79
    else:
        bound = lambda r: 1e-5 * float(r.abs().max()) + 1e-4 * np.sqrt(R) * 1e-2             # tests/test_train_gpu.py:67,79
    first = None
    for lay, (lz, lx) in (("dense", ((0, 0), (0, 0))), ("strided", ((4, 4), (8, 4)))):
        zv, xv = gput(dz, dev, lz, 64), gput(x, dev, lx, 64)
        got = []
        for transform in ((False, True) if Cin % 4 == 0 else (False,)):
            sc, sh = (P(av), P(bv)) if transform else (None, None)
            want = ref2 if transform else ref
            dw, w = guarded((Cout, Cin), F32, device=dev), guard.workspace(nbytes, device=dev)
            L(entry + "_f32", dev, P(zv), zv.stride(0), P(xv), xv.stride(0), R, Cout, Cin, P(dw), 0, P(w), nbytes, sc, sh)
            checked(dw, inputs=(zv, xv, w))
            assert float((dw.cpu().double() - want).abs().max()) <= bound(want)
            # accumulate into a dW that holds values, NaN all around it
            acc, w2 = embed(dw.contiguous()), guard.workspace(nbytes, device=dev)
            L(entry + "_f32", dev, P(zv), zv.stride(0), P(xv), xv.stride(0), R, Cout, Cin, P(acc), 1, P(w2), nbytes, sc, sh)
            checked(inputs=(acc, w2))
            torch.testing.assert_close(acc, 2 * dw, rtol=1e-6, atol=1e-6)                    # tests/test_gemm_gpu.py:81, test_train_gpu.py:70
            # the partials form: the chunks stay in the workspace
            w3, nch = guard.workspace(nbytes, device=dev), ctypes.c_int(0)
            L(entry + "_partials_f32", dev, P(zv), zv.stride(0), P(xv), xv.stride(0), R, Cout, Cin, P(w3), nbytes, sc, sh, ctypes.byref(nch))
            check_guard(w3, all_written=False)
            assert 0 < nch.value * Cout * Cin * 4 <= nbytes
            part = w3.view(F32)[:nch.value * Cout * Cin].view(nch.value, Cout, Cin)
            assert not bool(torch.isnan(part).any())
            assert float((part.double().sum(0).cpu() - want).abs().max()) <= bound(want)
            same_bits(host(w3), host(w), ("partials",))                                      # the finishing launch is all that differs
            got += list(host(dw, acc, w))
        if first is None:
            first = got
        else:
            same_bits(first, got, ["%s (%s)" % (n, lay) for n in ("dW", "accumulated", "partials") * 2])
        form = ("large-block kernel (wgrad2)" if two else "small-K" if Cin <= 4 and Cout % 4 == 0 else
                "streaming" if (Cin == 64 and Cout in (64, 128) and R >= 65536) else "128 x 128-block kernel")
        PATHS[(entry + "_f32 (+ _partials)", R, Cout, Cin, lay, form)] = "vector"
    if not two:         # the large-block kernel refuses what its geometry does not take, and writes nothing
        dw, w = guarded((Cout, Cin), F32, device=dev), guard.workspace(max(4, nbytes), device=dev)
        with pytest.raises(RuntimeError, match="PTT_EUNSUPPORTED"):
            L("ptt_linear_wgrad2_f32", dev, P(zv), zv.stride(0), P(xv), xv.stride(0), R, Cout, Cin, P(dw), 0, P(w), nbytes, None, None)
        guard.assert_untouched(dw, w)
    # operands that are not float4-addressable: the 128 x 128-block kernel has scalar loads for either side
    # (linear_wgrad_kernel<VZ, VX>), the small-K form falls back to it, the large-block kernel refuses
    zo, xo = embed(dz.to(dev), ld=Cout + 3, col_off=1), embed(x.to(dev), ld=Cin + 5, col_off=2)
    if two:
        dw, w = guarded((Cout, Cin), F32, device=dev), guard.workspace(nbytes, device=dev)
        with pytest.raises(RuntimeError, match="PTT_EUNSUPPORTED"):
            L("ptt_linear_wgrad2_f32", dev, P(zo), zo.stride(0), P(xo), xo.stride(0), R, Cout, Cin, P(dw), 0, P(w), nbytes, None, None)
        guard.assert_untouched(dw, w)
        PATHS[("ptt_linear_wgrad2_f32", R, Cout, Cin, "misaligned")] = "refused"
    nb1 = int(ops._host("ptt_linear_wgrad_workspace", R, Cout, Cin))
    dw, w = guarded((Cout, Cin), F32, device=dev), guard.workspace(nb1, device=dev)
    L("ptt_linear_wgrad_f32", dev, P(zo), zo.stride(0), P(xo), xo.stride(0), R, Cout, Cin, P(dw), 0, P(w), nb1, None, None)
    checked(dw, inputs=(zo, xo, w))
    assert float((dw.cpu().double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max()) + 1e-4 * np.sqrt(R) * 1e-2      # test_train_gpu.py:67
    PATHS[("ptt_linear_wgrad_f32", R, Cout, Cin, "misaligned")] = "scalar"


# ----------------------------------------------------------------------------- row-wise kernels of the transformer blocks
# One wave per row, four rows per workgroup, scalar loads: one code path, so EVERY layout — misaligned ones too — is bit-identical
# to the dense run. lds of x, residual / dy, out / dx per layout:
ROW_LAYOUTS = {"dense": ((0, 0), (0, 0), (0, 0)), "strided": ((4, 4), (8, 4), (12, 8)), "off1": ((4, 1), (7, 2), (9, 3)), "odd": ((1, 0), (3, 1), (5, 0))}
LN_CS = (4, 33, 60, 512, 1024)
TOL = dict(atol=1e-4, rtol=1e-4)        # tests/test_dense_gpu.py:17, test_multitransformer_gpu.py:19, test_golden_gpu.py: the 1e-4 bar of the inference path


def ln_data(rows, C):
    rs = np.random.RandomState(131 * rows + C)                          # as tests/test_layernorm_train_gpu.py:23-30
    x = rs.standard_normal((rows, C)).astype(np.float32) * (1.0 + rs.rand(rows, 1).astype(np.float32))
    w = (1.0 + 0.3 * rs.standard_normal(C)).astype(np.float32)
    b = (0.5 * rs.standard_normal(C)).astype(np.float32)
    r = rs.standard_normal((rows, C)).astype(np.float32)
    dy = rs.standard_normal((rows, C)).astype(np.float32)
    return tuple(torch.from_numpy(a) for a in (x, w, b, r, dy))


@pytest.mark.parametrize("C", LN_CS)
@pytest.mark.parametrize("rows", (1, 3, 5))
def test_layernorm_forward(dev, rows, C):
    """ptt_layernorm_f32 (also with out aliasing x) and ptt_layernorm_train_fwd_f32."""
    x, w, b, r, _ = ln_data(rows, C)
    xd = x.double()
    ref = F.layer_norm(xd, (C,), w.double(), b.double(), EPS) + r.double()
    mu, rs = xd.mean(1), 1.0 / torch.sqrt(xd.var(1, unbiased=False) + EPS)
    wv, bv = embed(w.to(dev)), embed(b.to(dev))
    first = None
    for lay, (lx, lr, lo) in ROW_LAYOUTS.items():
        xv, rv, o = gput(x, dev, lx, 4), gput(r, dev, lr, 4), gout((rows, C), dev, lo)
        L("ptt_layernorm_f32", dev, P(xv), rows, C, xv.stride(0), P(wv), P(bv), EPS, P(rv), rv.stride(0), P(o), o.stride(0))
        checked(o, inputs=(xv, rv, wv, bv))
        np.testing.assert_allclose(o.cpu().numpy(), ref.numpy(), **TOL)                 # tests/test_multitransformer_gpu.py:19,56
        xi = gput(x, dev, lx, 4)                                                        # documented: "out may alias x"
        L("ptt_layernorm_f32", dev, P(xi), rows, C, xi.stride(0), P(wv), P(bv), EPS, P(rv), rv.stride(0), P(xi), xi.stride(0))
        check_guard(xi, all_written=False)
        same_bits(host(xi), host(o), ("out aliasing x",))
        y, mean, rstd = gout((rows, C), dev, lo), guarded((rows,), F32, device=dev), guarded((rows,), F32, device=dev)
        L("ptt_layernorm_train_fwd_f32", dev, P(xv), rows, C, xv.stride(0), P(wv), P(bv), EPS, P(rv), rv.stride(0), P(y), y.stride(0), P(mean), P(rstd))
        checked(y, mean, rstd, inputs=(xv, rv))
        np.testing.assert_allclose(y.cpu().numpy(), ref.numpy(), atol=1e-5, rtol=1e-5)  # tests/test_layernorm_train_gpu.py:44
        err = (mean.cpu().double() - mu).abs()
        assert bool((err <= 1e-6 * (mu.abs() + 1.0 / rs)).all())                        # :47-48
        np.testing.assert_allclose(rstd.cpu().numpy(), rs.numpy(), rtol=1e-6)           # :49
        got = host(o, y, mean, rstd)
        if first is None:
            first = got
        else:
            same_bits(first, got, ["%s (%s)" % (n, lay) for n in ("out", "train out", "mean", "rstd")])
        PATHS[("ptt_layernorm_f32 / _train_fwd_f32", rows, C, lay)] = "scalar"


@pytest.mark.parametrize("C", LN_CS)
@pytest.mark.parametrize("rows", (1, 3, 5, 33))             # 33: one row past the LNB_ROWS = 32 chunk
def test_layernorm_backward(dev, rows, C):
    from ptt_amd import ops
    x, w, b, _, dy = ln_data(rows, C)
    xd, wd, bd = (t.double().requires_grad_(True) for t in (x, w, b))
    F.layer_norm(xd, (C,), wd, bd, EPS).backward(dy.double())
    mu = xd.detach().mean(1)
    rs = 1.0 / torch.sqrt(xd.detach().var(1, unbiased=False) + EPS)
    xhat = ((xd - xd.mean(1, keepdim=True)) / torch.sqrt(xd.var(1, unbiased=False, keepdim=True) + EPS)).detach()
    wv, mv, rv = embed(w.to(dev)), embed(mu.float().to(dev)), embed(rs.float().to(dev))
    first = None
    for lay, (lx, lg, ld) in ROW_LAYOUTS.items():
        xv, gv, dx = gput(x, dev, lx, 4), gput(dy, dev, lg, 4), gout((rows, C), dev, ld)
        dw, db = guarded((C,), F32, device=dev), guarded((C,), F32, device=dev)
        ws, n = ws_of("ptt_layernorm_bwd_workspace", dev, rows, C)
        L("ptt_layernorm_bwd_f32", dev, P(gv), gv.stride(0), P(xv), xv.stride(0), P(mv), P(rv), P(wv), rows, C, P(dx), dx.stride(0), P(dw), P(db), P(ws), n)
        checked(dx, dw, db, ws, inputs=(xv, gv, mv, rv, wv))                            # the workspace is written whole: exact size
        np.testing.assert_allclose(dx.cpu().numpy(), xd.grad.numpy(), atol=1e-5, rtol=1e-5)            # tests/test_layernorm_train_gpu.py:61
        for got, ref, terms in ((dw, wd.grad, (dy.double() * xhat).abs().sum(0)), (db, bd.grad, dy.double().abs().sum(0))):
            err = (got.cpu().double() - ref).abs()
            assert bool((err <= 1e-5 * ref.abs() + 1e-5 * terms).all())                 # :64-67
        got = host(dx, dw, db, ws)
        if first is None:
            first = got
        else:
            same_bits(first, got, ["%s (%s)" % (n_, lay) for n_ in ("dx", "dweight", "dbias", "partials")])
        PATHS[("ptt_layernorm_bwd_f32", rows, C, lay)] = "scalar"
    assert ops._host("ptt_layernorm_bwd_workspace", rows, C) == ((rows + 31) // 32) * 2 * C * 8


@pytest.mark.parametrize("n", (1, 16, 100, 128))
@pytest.mark.parametrize("rows", (1, 3, 5))
def test_softmax_rows_in_place(dev, rows, n):
    x = torch.randn(rows, n, generator=gen(rows * 1000 + n)) * 3
    scale = 1.0 / 512 ** 0.5
    ref = torch.softmax(x.double() * scale, dim=1)
    first = None
    for lay, (lx, _, _) in ROW_LAYOUTS.items():
        xv = gput(x, dev, lx, 4)
        L("ptt_softmax_rows_f32", dev, P(xv), rows, n, xv.stride(0), scale)
        check_guard(xv, all_written=False)                                              # the gap words still hold the fill
        np.testing.assert_allclose(xv.cpu().numpy(), ref.numpy(), **TOL)                # tests/test_golden_gpu.py:102
        np.testing.assert_allclose(xv.sum(-1).cpu().numpy(), 1.0, atol=1e-5)            # :103
        if first is None:
            first = host(xv)
        else:
            same_bits(first, host(xv), ("softmax (%s)" % lay,))
        PATHS[("ptt_softmax_rows_f32", rows, n, lay)] = "scalar"


@pytest.mark.parametrize("D", (4, 64))
def test_pair_input_and_attention_on_column_slices(dev, D):
    """ptt_pt_pair_input_ld_f32 / ptt_pt_attn_fwd_ld_f32 on q | k | v column slices of NaN-surrounded (B N, 3 D + pad) buffers
    (ops.pt_pair_input_qkv, ops.pt_attn_fwd_qkv) against the contiguous entry points and the header's formulas in float64."""
    B, N, k = 2, 20, 16
    g = gen(D)
    qkv = torch.randn(B * N, 3 * D, generator=g)
    knn = torch.stack([torch.stack([torch.randperm(N, generator=g)[:k] for _ in range(N)]) for _ in range(B)]).int()     # inside the cloud
    pos, a = torch.randn(B * N * k, D, generator=g), torch.randn(B * N * k, D, generator=g) * 3
    scale = 1.0 / D ** 0.5
    q64, k64, v64 = (qkv[:, i * D:(i + 1) * D].double().view(B, N, D) for i in range(3))
    flat = (knn.long() + torch.arange(B).view(B, 1, 1) * N).view(-1)
    p64 = pos.double().view(B, N, k, D)
    t_ref = q64[:, :, None, :] - k64.reshape(B * N, D)[flat].view(B, N, k, D) + p64                                    # ptt_hip.h: ptt_pt_pair_input_f32
    at_ref = torch.softmax(a.double().view(B, N, k, D) * scale, dim=2)
    res_ref = (at_ref * (v64.reshape(B * N, D)[flat].view(B, N, k, D) + p64)).sum(2)                                    # ptt_pt_attn_train_fwd_f32
    knnv, posv, av = embed(knn.view(B * N, k).to(dev)), embed(pos.to(dev)), embed(a.to(dev))
    dense = [embed(qkv[:, i * D:(i + 1) * D].contiguous().to(dev)) for i in range(3)]
    t0, at0, r0 = guarded((B * N * k, D), F32, device=dev), guarded((B * N * k, D), F32, device=dev), guarded((B * N, D), F32, device=dev)
    L("ptt_pt_pair_input_f32", dev, P(dense[0]), P(dense[1]), P(knnv), P(posv), B, N, k, D, P(t0))
    L("ptt_pt_attn_train_fwd_f32", dev, P(av), P(dense[2]), P(knnv), P(posv), B, N, k, D, scale, P(at0), P(r0))
    checked(t0, at0, r0, inputs=dense + [knnv, posv, av])
    buf1 = embed(qkv.to(dev), ld=3 * D + 4, col_off=4, lead=64 * (3 * D + 4), tail=64 * (3 * D + 4))    # q and v: ld = 3 D + 4
    buf2 = embed(qkv.to(dev), ld=3 * D + 8, col_off=4, lead=64 * (3 * D + 8), tail=64 * (3 * D + 8))    # k: ld = 3 D + 8
    q, kf, v = buf1[:, 0:D], buf2[:, D:2 * D], buf1[:, 2 * D:]
    t1 = guarded((B * N * k, D), F32, device=dev)
    L("ptt_pt_pair_input_ld_f32", dev, P(q), q.stride(0), P(kf), kf.stride(0), P(knnv), P(posv), B, N, k, D, P(t1))
    checked(t1, inputs=(buf1, buf2, knnv, posv))
    np.testing.assert_allclose(t1.cpu().numpy(), t_ref.view(-1, D).numpy(), **TOL)       # tests/test_rowjobs_gpu.py:11,104 (the same prologue)
    same_bits(host(t1), host(t0), ("pair input",))
    for want_attn in (True, False):
        at1, r1 = guarded((B * N * k, D), F32, device=dev), guarded((B * N, D), F32, device=dev)
        L("ptt_pt_attn_fwd_ld_f32", dev, P(av), P(v), v.stride(0), P(knnv), P(posv), B, N, k, D, scale, P(at1) if want_attn else None, P(r1))
        checked(r1, inputs=(buf1, knnv, posv, av))
        np.testing.assert_allclose(r1.cpu().numpy(), res_ref.view(-1, D).numpy(), **TOL)              # tests/test_dense_gpu.py:175-176
        same_bits(host(r1), host(r0), ("res",))
        if want_attn:
            check_guard(at1)
            np.testing.assert_allclose(at1.cpu().numpy(), at_ref.view(-1, D).numpy(), **TOL)
            same_bits(host(at1), host(at0), ("attn",))
        else:
            guard.assert_untouched(at1)
    PATHS[("ptt_pt_pair_input_ld_f32 / ptt_pt_attn_fwd_ld_f32", B * N, D, "q | k | v column slices")] = "vector"
    # ldq % 4 != 0 is refused
    bad = embed(qkv.to(dev), ld=3 * D + 5)
    t2 = guarded((B * N * k, D), F32, device=dev)
    with pytest.raises(RuntimeError, match="PTT_EINVAL"):
        L("ptt_pt_pair_input_ld_f32", dev, P(bad), 3 * D + 5, P(kf), kf.stride(0), P(knnv), P(posv), B, N, k, D, P(t2))
    with pytest.raises(RuntimeError, match="PTT_EINVAL"):
        L("ptt_pt_attn_fwd_ld_f32", dev, P(av), P(bad), 3 * D + 5, P(knnv), P(posv), B, N, k, D, scale, None, P(t2))
    guard.assert_untouched(t2)


# ------------------------------------------------------------------------------------------- fp32-MFMA linear family (mfma_ops.hip)
def lin_data(rows, K, Cout):
    rs = np.random.RandomState(rows + K)                                # as tests/test_dense_gpu.py:24-28
    f = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32))
    d = dict(x=f(rows, K), w=f(Cout, K) / np.sqrt(K), sc=torch.from_numpy(rs.uniform(0.5, 1.5, Cout).astype(np.float32)), sh=f(Cout), r=f(rows, Cout))
    d["ref"] = torch.relu(d["x"].double() @ d["w"].double().t() * d["sc"].double() + d["sh"].double()) + d["r"].double()
    return d


# case -> [(layout name, (pad, off) of X, of residual, of out, the path linear_launch takes)]; within a case, layouts that share
# a path must agree bit for bit
LINEAR_CASES = {
    (33, 64, 96): [("dense", (0, 0), (0, 0), (0, 0), "linear_small_kernel"), ("strided", (4, 4), (8, 4), (12, 8), "linear_small_kernel"),
                   ("off1", (4, 1), (8, 4), (12, 8), "linear_kernel<1,false,1>, K % 4 == 0"), ("odd", (3, 0), (5, 1), (7, 2), "linear_kernel<1,false,1>, K % 4 == 0")],
    (33, 24, 64): [("dense", (0, 0), (0, 0), (0, 0), "linear_kernel<1,true,1>"), ("strided", (4, 4), (8, 4), (12, 8), "linear_kernel<1,true,1>")],
    (33, 131, 96): [("dense", (0, 0), (0, 0), (0, 0), "linear_kernel<1,false,1>, K % 4 != 0"), ("strided", (5, 4), (8, 4), (12, 8), "linear_kernel<1,false,1>, K % 4 != 0")],
    (32769, 32, 256): [("dense", (0, 0), (0, 0), (0, 0), "linear_kernel<1,true,2>"), ("strided", (4, 4), (8, 4), (12, 8), "linear_kernel<1,true,2>")],
}


@pytest.mark.parametrize("rows,K,Cout", list(LINEAR_CASES))
def test_linear(dev, rows, K, Cout):
    """ptt_linear_f32 with scale, shift, ReLU and residual, one case per path of linear_launch; ptt_linear_act_in_f32."""
    from ptt_amd import ops
    d = lin_data(rows, K, Cout)
    wp = ops.pack_weight(d["w"].to(dev))
    sc, sh = embed(d["sc"].to(dev)), embed(d["sh"].to(dev))
    g = gen(K)
    ia, ib = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g) * 0.3
    iav, ibv = embed(ia.to(dev)), embed(ib.to(dev))
    ref_act = torch.relu(d["x"].double() * ia.double() + ib.double()) @ d["w"].double().t()
    by_path = {}
    for lay, lx, lr, lo, path in LINEAR_CASES[(rows, K, Cout)]:
        x, r, o = gput(d["x"], dev, lx, 32), gput(d["r"], dev, lr, 32), gout((rows, Cout), dev, lo)
        vec = K % 4 == 0 and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0
        assert vec == ("false" not in path)
        L("ptt_linear_f32", dev, P(x), rows, K, x.stride(0), P(wp), Cout, P(sc), P(sh), 1, P(r), r.stride(0), P(o), o.stride(0))
        checked(o, inputs=(x, r, sc, sh))
        np.testing.assert_allclose(o.cpu().numpy(), d["ref"].numpy(), **TOL)            # tests/test_dense_gpu.py:36
        got = list(host(o))
        o2 = gout((rows, Cout), dev, lo)
        if vec:
            L("ptt_linear_act_in_f32", dev, P(x), rows, K, x.stride(0), P(iav), P(ibv), P(wp), Cout, P(o2), o2.stride(0))
            checked(o2, inputs=(x, iav, ibv))
            np.testing.assert_allclose(o2.cpu().numpy(), ref_act.numpy(), **TOL)        # the same kernels: tests/test_dense_gpu.py:36
            got += list(host(o2))
        else:       # "needs K % 4 == 0, ldx % 4 == 0 and 16-byte aligned X": PTT_EINVAL
            with pytest.raises(RuntimeError, match="PTT_EINVAL"):
                L("ptt_linear_act_in_f32", dev, P(x), rows, K, x.stride(0), P(iav), P(ibv), P(wp), Cout, P(o2), o2.stride(0))
            guard.assert_untouched(o2)
        if path in by_path:
            same_bits(by_path[path], got, ["%s (%s)" % (n, lay) for n in ("out", "act_in out")])
        else:
            by_path[path] = got
        PATHS[("ptt_linear_f32 / ptt_linear_act_in_f32", rows, K, Cout, lay, path)] = "vector" if vec else "scalar"


def test_linear_batched(dev):
    """ptt_linear_batched_f32: batch strides larger than rows * ld for x, residual and out; x_batch_stride % 4 != 0 once (vec_ok
    tests xb & 3: the non-vector form)."""
    from ptt_amd import ops
    Bt, rows, K, Cout = 3, 33, 64, 96
    g = gen(7)
    x, w, r = torch.randn(Bt, rows, K, generator=g), torch.randn(Bt, Cout, K, generator=g) / K ** 0.5, torch.randn(Bt, rows, Cout, generator=g)
    ref = torch.bmm(x.double(), w.double().transpose(1, 2)) + r.double()
    wp = torch.stack([ops.pack_weight(w[i].to(dev)) for i in range(Bt)]).contiguous()
    seen = {}
    for lay, (px, ox, bx), (pr, orr, br), (po, oo, bo) in (("dense", (0, 0, 0), (0, 0, 0), (0, 0, 0)), ("strided", (4, 4, 8), (8, 4, 16), (12, 8, 24)),
                                                          ("x_batch_stride % 4 != 0", (4, 4, 9), (8, 4, 16), (12, 8, 24)),
                                                          ("odd ldx", (3, 1, 9), (8, 4, 16), (12, 8, 24))):
        xv = embed(x.to(dev), ld=K + px, col_off=ox, batch_stride=rows * (K + px) + bx)
        rv = embed(r.to(dev), ld=Cout + pr, col_off=orr, batch_stride=rows * (Cout + pr) + br)
        o = guarded((Bt, rows, Cout), F32, ld=Cout + po, col_off=oo, batch_stride=rows * (Cout + po) + bo, device=dev)
        L("ptt_linear_batched_f32", dev, P(xv), rows, K, xv.stride(1), xv.stride(0), P(wp), wp.stride(0), Cout, None, None, 0, P(rv), rv.stride(1),
          rv.stride(0), P(o), o.stride(1), o.stride(0), Bt)
        checked(o, inputs=(xv, rv))
        np.testing.assert_allclose(o.cpu().numpy(), ref.numpy(), **TOL)                 # tests/test_golden_gpu.py:101
        vec = xv.stride(1) % 4 == 0 and xv.stride(0) % 4 == 0 and xv.data_ptr() % 16 == 0
        if vec in seen:
            same_bits(seen[vec], host(o), ("out (%s)" % lay,))
        else:
            seen[vec] = host(o)
        PATHS[("ptt_linear_batched_f32", Bt, rows, K, Cout, lay)] = "vector" if vec else "scalar"
    assert set(seen) == {True, False}


@pytest.mark.parametrize("widths,res", [([259, 256, 259], True), ([40, 64], False)])
@pytest.mark.parametrize("rows", (1, 33, 130))
def test_rows_mlp(dev, rows, widths, res):
    """ptt_rows_mlp_f32: ldx, ldr, ldo all different; ldo = 260 for the 259-wide output (as tests/test_dense_gpu.py:45-69)."""
    from ptt_amd import _lib, ops
    rs = np.random.RandomState(rows + len(widths))
    x = torch.from_numpy(rs.standard_normal((rows, widths[0])).astype(np.float32))
    r = torch.from_numpy(rs.standard_normal((rows, widths[-1])).astype(np.float32))
    ref = x.double()
    arr = (_lib.SaLayer * (len(widths) - 1))()
    keep = []
    for i, (cin, cout) in enumerate(zip(widths[:-1], widths[1:])):
        w = torch.from_numpy((rs.standard_normal((cout, cin)) / np.sqrt(cin)).astype(np.float32))
        sc = torch.from_numpy(rs.uniform(0.5, 1.5, cout).astype(np.float32))
        sh = torch.from_numpy(rs.standard_normal(cout).astype(np.float32))
        relu = i < len(widths) - 2
        ref = ref @ w.double().t() * sc.double() + sh.double()
        if relu:
            ref = ref.clamp_min(0)
        keep += [ops.pack_weight(w.to(dev)), embed(sc.to(dev)), embed(sh.to(dev))]
        arr[i].Wpacked, arr[i].scale, arr[i].shift = (t.data_ptr() for t in keep[-3:])
        arr[i].Cin, arr[i].Cout, arr[i].relu = cin, cout, int(relu)
    if res:
        ref = ref + r.double()
    K, Co = widths[0], widths[-1]
    seen = {}
    for lay, lx, lr, lo in (("dense", (0, 0), (0, 0), (0, 0)), ("strided", (4, 4), (9, 4), (1, 0) if Co == 259 else (12, 8)), ("off1", (4, 1), (9, 2), (5, 3))):
        xv, rv, o = gput(x, dev, lx, 32), gput(r, dev, lr, 32), gout((rows, Co), dev, lo)
        L("ptt_rows_mlp_f32", dev, P(xv), rows, K, xv.stride(0), arr, len(widths) - 1, P(rv) if res else None, rv.stride(0) if res else 0, P(o), o.stride(0))
        checked(o, inputs=(xv, rv))
        np.testing.assert_allclose(o.cpu().numpy(), ref.float().numpy(), **TOL)         # tests/test_dense_gpu.py:69
        vec = K % 4 == 0 and xv.stride(0) % 4 == 0 and xv.data_ptr() % 16 == 0          # p.vec_in
        if vec in seen:
            same_bits(seen[vec], host(o), ("out (%s)" % lay,))
        else:
            seen[vec] = host(o)
        PATHS[("ptt_rows_mlp_f32", rows, tuple(widths), lay)] = "vector" if vec else "scalar"


def test_row_jobs_write_only_their_columns(dev):
    """ptt_row_jobs_f32 through ops.row_job / ops.row_jobs, two jobs in one launch: the first job's residual is a column slice of
    a wider buffer; the second job's output is column 0:1 of a (rows, 257) buffer — vfeats[:, 0:1] of the voting head
    (centroids_voting_head.py): the 256 neighbouring columns of every row stay untouched."""
    from ptt_amd import ops
    rows, K = 130, 256
    g = gen(11)
    x, w1, sh1, res = torch.randn(rows, K, generator=g), torch.randn(256, K, generator=g) / 16, torch.randn(256, generator=g), torch.randn(rows, 256, generator=g)
    w2, sh2 = torch.randn(1, K, generator=g) / 16, torch.randn(1, generator=g)
    ref1 = torch.relu(x.double() @ w1.double().t() + sh1.double()) + res.double()
    ref2 = torch.sigmoid(x.double() @ w2.double().t() + sh2.double())
    wp1, wp2 = ops.pack_weight(w1.to(dev)), ops.pack_weight(w2.to(dev))
    s1, s2 = embed(sh1.to(dev)), embed(sh2.to(dev))
    first = None
    for lay, lx, lr, lo in (("dense", (0, 0), (0, 0), (0, 0)), ("strided", (4, 4), (3, 3), (8, 4))):
        xv, rv, o1 = gput(x, dev, lx, 32), gput(res, dev, lr, 32), gout((rows, 256), dev, lo)
        o2 = guarded((rows, 1), F32, ld=257, col_off=0, device=dev)
        raw = guarded((rows, 1), F32, ld=5, col_off=2, device=dev)
        ops.row_jobs([ops.row_job(wp1, 256, x=xv, shift=s1, act=1, res=rv, out=o1), ops.row_job(wp2, 1, x=xv, shift=s2, act=2, out=o2, raw=raw)])
        checked(o1, o2, raw, inputs=(xv, rv, s1, s2))
        np.testing.assert_allclose(o1.cpu().numpy(), ref1.numpy(), **TOL)               # tests/test_rowjobs_gpu.py:11,41
        np.testing.assert_allclose(o2.cpu().numpy(), ref2.numpy(), **TOL)
        np.testing.assert_allclose(raw.cpu().numpy(), (x.double() @ w2.double().t() + sh2.double()).numpy(), **TOL)     # :42
        if first is None:
            first = host(o1, o2, raw)
        else:
            same_bits(first, host(o1, o2, raw), ("job 1 out", "job 2 out", "job 2 raw"))
        PATHS[("ptt_row_jobs_f32", rows, K, lay)] = "vector"


# ------------------------------------------------------------------------------------ ld = C - 1: refused, nothing launched
def test_every_leading_dimension_below_the_row_length_is_refused(dev):
    """For every entry point of this file and every leading dimension it takes: ld = C - 1 raises and leaves every output word
    untouched (the check returns before the launch)."""
    from ptt_amd import _lib, ops
    R, C, ns = 32, 128, 16
    G = R // ns
    f = lambda *s: embed(torch.randn(*s).to(dev))
    x, x2, x3 = f(R, C), f(R, C), f(R, C)
    pooled = f(G, C)
    vec = [f(C) for _ in range(8)]
    arg = embed(torch.zeros(G, C, dtype=I32).to(dev))
    count = embed(torch.full((1,), float(R), dtype=F64).to(dev))
    o, o2, o3 = (guarded((R, C), F32, device=dev) for _ in range(3))
    og, og2 = guarded((G, C), F32, device=dev), guarded((G, C), F32, device=dev)
    oarg, oarg2 = guarded((G, C), I32, device=dev), guarded((G, C), I32, device=dev)
    c1, c2, c3, c4, c5 = (guarded((C,), F32, device=dev) for _ in range(5))
    sums = guarded((2 * C + 1,), F64, device=dev)
    stats = guarded((512 * 2 * C,), F64, device=dev)
    rowv = [guarded((R,), F32, device=dev) for _ in range(2)]
    ws = guard.workspace(2 << 20, device=dev)
    wsn = 2 << 20
    wp = ops.pack_weight(torch.randn(C, C).to(dev))
    knn = embed(torch.zeros(2, 16, dtype=I32).to(dev))
    nch = ctypes.c_int(0)
    layer = (_lib.SaLayer * 1)()
    layer[0].Wpacked, layer[0].Cin, layer[0].Cout = wp.data_ptr(), C, C
    outs = [o, o2, o3, og, og2, oarg, oarg2, c1, c2, c3, c4, c5, sums, stats, ws] + rowv
    v = [P(t) for t in vec]
    X, X2, X3, O, O2, O3 = P(x), P(x2), P(x3), P(o), P(o2), P(o3)
    bad = C - 1

    def each(entry, n_ld, call):
        """call(lds) launches `entry` with the list lds of its n_ld leading dimensions: every single one set to C - 1 must raise."""
        for i in range(n_ld):
            lds = [C] * n_ld
            lds[i] = bad
            with pytest.raises(RuntimeError, match="PTT_E(INVAL|UNSUPPORTED)"):
                call(lds)
            guard.assert_untouched(*outs)
        call([C] * n_ld)                            # and with every ld = C the same arguments are accepted
        for t in outs:
            t._guard.words.fill_(guard.SENTINEL)
        PATHS[(entry, "ld = C - 1")] = "refused"

    each("ptt_bn_stats_f32", 1, lambda l: L("ptt_bn_stats_f32", dev, X, R, C, l[0], EPS, P(c1), P(c2), P(c3), P(ws), wsn))
    each("ptt_bn_apply_f32", 2, lambda l: L("ptt_bn_apply_f32", dev, X, l[0], v[0], v[1], v[2], v[3], R, C, 1, O, l[1]))
    each("ptt_bn_bwd_f32", 4, lambda l: L("ptt_bn_bwd_f32", dev, X, l[0], X2, l[1], X3, l[2], v[0], v[1], v[2], R, C, 1, O, l[3], P(c1), P(c2), P(ws), wsn, None, None))
    each("ptt_bn_sums_f64", 1, lambda l: L("ptt_bn_sums_f64", dev, X, R, C, l[0], P(sums), P(ws), wsn))
    each("ptt_bn_bwd_sums_f64", 3, lambda l: L("ptt_bn_bwd_sums_f64", dev, X, l[0], X2, l[1], X3, l[2], v[0], v[1], R, C, P(sums), P(ws), wsn, None, None))
    each("ptt_bn_bwd_apply_f32", 4, lambda l: L("ptt_bn_bwd_apply_f32", dev, X, l[0], X2, l[1], X3, l[2], v[0], v[1], v[2], v[3], v[4], P(count), R, C, O, l[3],
                                                None, None))
    each("ptt_bn_bwd_from_partials_f32", 3, lambda l: L("ptt_bn_bwd_from_partials_f32", dev, P(stats), 1, X, l[0], X2, l[1], v[0], v[1], v[2], R, C, O, l[2],
                                                        P(c1), P(c2), v[3], v[4]))
    each("ptt_bn_bwd_pooled_f32", 3, lambda l: L("ptt_bn_bwd_pooled_f32", dev, P(pooled), l[0], P(arg), ns, X, l[1], v[0], v[1], v[2], R, C, O, l[2], P(c1), P(c2),
                                                 P(ws), wsn, v[3], v[4]))
    each("ptt_bn_bwd_pooled_sums_f64", 2, lambda l: L("ptt_bn_bwd_pooled_sums_f64", dev, P(pooled), l[0], P(arg), ns, X, l[1], v[0], v[1], R, C, P(sums), P(ws), wsn,
                                                      v[3], v[4]))
    each("ptt_bn_bwd_pooled_apply_f32", 3, lambda l: L("ptt_bn_bwd_pooled_apply_f32", dev, P(pooled), l[0], P(arg), ns, X, l[1], v[0], v[1], v[2], v[3], v[4],
                                                       P(count), R, C, O, l[2], v[5], v[6]))
    each("ptt_bn_bwd_pooled_consts_f32", 2, lambda l: L("ptt_bn_bwd_pooled_consts_f32", dev, P(pooled), l[0], P(arg), ns, X, l[1], v[0], v[1], v[2], R, C, P(c1), P(c2),
                                                        P(c3), P(c4), P(c5), P(ws), wsn, v[3], v[4]))
    each("ptt_pool_rows_f32", 2, lambda l: L("ptt_pool_rows_f32", dev, X, l[0], G, ns, C, P(og), l[1], P(oarg), None, None))
    each("ptt_pool_rows_bwd_f32", 2, lambda l: L("ptt_pool_rows_bwd_f32", dev, P(pooled), l[0], P(arg), G, ns, C, O, l[1]))
    each("ptt_colsum_f32", 1, lambda l: L("ptt_colsum_f32", dev, X, R, C, l[0], P(c1), P(ws), wsn))
    each("ptt_colsum_partials_f32", 1, lambda l: L("ptt_colsum_partials_f32", dev, X, R, C, l[0], P(ws), wsn, ctypes.byref(nch)))
    each("ptt_linear_wgrad_f32", 2, lambda l: L("ptt_linear_wgrad_f32", dev, X, l[0], X2, l[1], R, C, C, P(stats), 0, P(ws), wsn, None, None))
    each("ptt_linear_wgrad_partials_f32", 2, lambda l: L("ptt_linear_wgrad_partials_f32", dev, X, l[0], X2, l[1], R, C, C, P(ws), wsn, None, None, ctypes.byref(nch)))
    each("ptt_layernorm_f32", 3, lambda l: L("ptt_layernorm_f32", dev, X, R, C, l[0], v[0], v[1], EPS, X2, l[1], O, l[2]))
    each("ptt_layernorm_train_fwd_f32", 3, lambda l: L("ptt_layernorm_train_fwd_f32", dev, X, R, C, l[0], v[0], v[1], EPS, X2, l[1], O, l[2], P(rowv[0]), P(rowv[1])))
    each("ptt_layernorm_bwd_f32", 3, lambda l: L("ptt_layernorm_bwd_f32", dev, X, l[0], X2, l[1], v[0], v[1], v[2], R, C, O, l[2], P(c1), P(c2), P(ws), wsn))
    each("ptt_softmax_rows_f32", 1, lambda l: L("ptt_softmax_rows_f32", dev, O, R, C, l[0], 1.0))
    each("ptt_linear_f32", 3, lambda l: L("ptt_linear_f32", dev, X, R, C, l[0], P(wp), C, None, None, 0, X2, l[1], O, l[2]))
    each("ptt_linear_act_in_f32", 2, lambda l: L("ptt_linear_act_in_f32", dev, X, R, C, l[0], v[0], v[1], P(wp), C, O, l[1]))
    each("ptt_linear_batched_f32", 3, lambda l: L("ptt_linear_batched_f32", dev, X, R, C, l[0], 0, P(wp), 0, C, None, None, 0, X2, l[1], 0, O, l[2], 0, 1))
    each("ptt_rows_mlp_f32", 3, lambda l: L("ptt_rows_mlp_f32", dev, X, R, C, l[0], layer, 1, X2, l[1], O, l[2]))
    each("ptt_rows_gemm_f32", 3, lambda l: L("ptt_rows_gemm_f32", dev, X, R, C, l[0], None, None, P(wp), C, None, 0, X2, l[1], O, l[2], None, 0))
    each("ptt_rows_gemm_masked_f32", 3, lambda l: L("ptt_rows_gemm_masked_f32", dev, X, R, C, l[0], P(wp), C, X2, l[1], O, l[2], None, 0))
    each("ptt_rows_gemm_bnbwd_f32", 3, lambda l: L("ptt_rows_gemm_bnbwd_f32", dev, X, R, C, l[0], P(wp), C, X2, l[1], v[0], v[1], v[2], v[3], O, l[2], P(stats),
                                                   stats.numel()))
    each("ptt_rows_gemm_pool_f32", 2, lambda l: L("ptt_rows_gemm_pool_f32", dev, X, R, C, l[0], v[0], v[1], P(wp), C, O, l[1], P(stats), stats.numel(), ns, P(og),
                                                  P(og2), P(oarg), P(oarg2)))
    each("ptt_rows_gemm_rsum16_f32", 5, lambda l: L("ptt_rows_gemm_rsum16_f32", dev, X, R, C, l[0], P(wp), C, X2, l[1], O, l[2], O2, l[3], O3, l[4]))
    each("ptt_rows_gemm_rsum16_heads_f32", 5, lambda l: L("ptt_rows_gemm_rsum16_heads_f32", dev, X, R, C, C, l[0], P(wp), X2, l[1], O, l[2], O2, l[3], O3, l[4]))
    # 2 points x 16 neighbours = the 32 rows of pos / a / t: q | k | v rows of D = C channels
    each("ptt_pt_pair_input_ld_f32", 2, lambda l: L("ptt_pt_pair_input_ld_f32", dev, X, l[0], X2, l[1], P(knn), X3, 1, 2, 16, C, O))
    each("ptt_pt_attn_fwd_ld_f32", 1, lambda l: L("ptt_pt_attn_fwd_ld_f32", dev, X3, X, l[0], P(knn), X2, 1, 2, 16, C, 1.0, O, O2))
    # a row job's leading dimensions are checked by ptt_row_jobs_f32 itself
    for name in ("ldx", "ldo", "ldr"):
        job, keep = ops.row_job(wp, C, x=x, res=x2, out=o)
        setattr(job, name, bad)
        with pytest.raises(RuntimeError, match="PTT_E(INVAL|UNSUPPORTED)"):
            L("ptt_row_jobs_f32", dev, (_lib.RowJob * 1)(job), 1)
        guard.assert_untouched(*outs)
    PATHS[("ptt_row_jobs_f32", "ld = C - 1")] = "refused"


# ------------------------------------------------------------------------------------------------------ coverage report (last)
def test_zz_coverage_report():
    """Prints, per entry point, the layouts that ran in this process and the path each took (run with -s to read it)."""
    by = {}
    for (entry, *key), path in sorted(PATHS.items(), key=str):
        by.setdefault(entry, {}).setdefault(path, []).append("x".join(str(k) for k in key))
    for entry in sorted(by):
        for path, keys in sorted(by[entry].items()):
            print("%-34s %-8s %d cases: %s" % (entry, path, len(keys), ", ".join(keys[:6]) + (" ..." if len(keys) > 6 else "")))
