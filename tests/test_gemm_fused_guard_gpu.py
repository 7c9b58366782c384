"""ptt_rows_gemm_bnbwd_fused_f32 (gemm_ops.hip: rows_gemm_kernel, the AIN instantiations) behind guard bands (tests/guard.py),
against the float64 reference of tests/gemm_fused_ref.py: the input-gradient GEMM that forms a layer's BatchNorm + ReLU backward
while it stages its rows, writes that dz out once, and takes the backward sums of the layer below in its epilogue.

All 12 instantiations run — three tile geometries (class a with one and with two column tiles per wave, class c) times four
A-operand forms (dense gradient, gradient pooled over 16 / 32 / 64 rows) — on ragged row counts, with one and with several row
tiles per persistent workgroup; which geometry a shape takes is asserted from ptt_rows_gemm_stat_chunks, and the closing
test_zz_ fails unless every pair was seen. Every (shape, layout) launches three times: with dz_out, again, and with dz_out = NULL.

Every output lies in guard.guarded(), the partials buffer has exactly chunks * 2 * N doubles, every input is guard.embed()-ded:
z, g and zp between 128 NaN rows, the constant vectors between NaNs, arg between INDEX_FILL words. On a ragged tile the staged
rows past the end are c0 - c1 * mean, not zeros — only the epilogue's `in` test keeps them out of `out` and the sums; a row that
leaks shows as a written guard word or a wrong sum.

No value bound is new: each is restated with the line of tests/test_round5_gpu.py it comes from. The mask data is exact by
construction and carries planted exact zeros (tests/gemm_fused_ref.py), so the strict `> 0` of both masks is part of what the
bounds check. What this does not prove: a stray READ whose value is discarded goes unseen. Nothing here measures speed."""
import ctypes
import functools
import types

import pytest
import torch

from tests import gemm_fused_ref as R
from tests import guard
from tests.guard import check_guard, embed, guarded
from tests.test_strided_guard_gpu import checked, gout, gput, host, same_bits

pytestmark = pytest.mark.gpu
L, P = guard.launch, guard.ptr
F32, F64, I32 = torch.float32, torch.float64, torch.int32
ENTRY = "ptt_rows_gemm_bnbwd_fused_f32"
CONSTS = ("k1", "c0", "c1", "mean", "act_a", "act_b", "mp", "ip", "ap", "bp")

# layout -> (pad, column offset) of g, z, dz_out, zp, out: every leading dimension differs from the others
LAYOUTS = {
    "dense": dict(g=(0, 0), z=(0, 0), dz=(0, 0), zp=(0, 0), out=(0, 0)),
    "strided": dict(g=(4, 4), z=(8, 4), dz=(12, 8), zp=(8, 4), out=(4, 4)),
    "strided, ldo = N + 3": dict(g=(4, 4), z=(8, 4), dz=(12, 8), zp=(8, 4), out=(3, 1)),
}
RAN = {}        # (form, ns) -> the shapes that ran it: test_zz_every_instantiation_ran


# ------------------------------------------------------------------------------------------------------------------ geometry
def cap_of(CU, ncg):
    """Workgroups per column group: two per CU resident, a multiple of 8 from 8 on (rows_gemm_geom, gemm_ops.hip)."""
    cap = 2 * CU // ncg
    if cap >= 8:
        cap &= ~7
    return max(cap, 1)


def geom(rows, K, N, CU, force_ct=None):
    """rows_gemm_geom restated: -> (form, row tiles, workgroups per column group, statistics chunks); form None = refused."""
    if N % 128 == 0 and K % 128 == 0:
        TR, WR = 64, 1
        CT = 2 if N % 256 == 0 and -(-rows // 64) * (N // 256) >= 2 * CU else 1
        CT = force_ct or CT
        form = "a, CT %d" % CT
    elif N % 128 == 0 and K % 64 == 0:
        return None, 0, 0, 0                                    # class b: the fused form refuses it
    elif N % 64 == 0 and K % 64 == 0:
        TR, WR, CT, form = 128, 2, 1, "c"
    else:
        return None, 0, 0, 0
    tiles = -(-rows // TR)
    G = min(tiles, cap_of(CU, N // (32 * (4 // WR) * CT)))
    return form, tiles, G, G * WR


def resolve(spec, ns, CU):
    """The CU-dependent row counts: one row past cap + 1 whole tiles (several tiles per workgroup, a ragged last one), rounded up to
    whole groups when the gradient is pooled."""
    rows = {"ct1": 64 * (cap_of(CU, 12) + 1) + 1, "ct2": 64 * -(-2 * CU // 6) + 1, "c": 128 * (cap_of(CU, 5) + 1) + 1}[spec] if isinstance(spec, str) else spec
    return -(-rows // ns) * ns if ns else rows


SHAPES = [
    # class a, one column tile per wave
    ("a, CT 1", 17, 128, 128, 0), ("a, CT 1", 197, 256, 128, 0), ("a, CT 1", "ct1", 128, 1536, 0),
    ("a, CT 1", 1 * 16, 128, 128, 16), ("a, CT 1", 5 * 16, 128, 128, 16), ("a, CT 1", 3 * 32, 256, 128, 32), ("a, CT 1", 3 * 64, 128, 128, 64),
    # class a, two column tiles per wave: 2 CU / 6 row tiles and one row more at N = 1536
    ("a, CT 2", "ct2", 128, 1536, 0), ("a, CT 2", "ct2", 128, 1536, 16), ("a, CT 2", "ct2", 128, 1536, 32), ("a, CT 2", "ct2", 128, 1536, 64),
    # class c
    ("c", 17, 64, 64, 0), ("c", 389, 128, 64, 0), ("c", "c", 64, 320, 0),
    ("c", 9 * 16, 64, 64, 16), ("c", 5 * 32, 128, 64, 32), ("c", 3 * 64, 64, 64, 64), ("c", "c", 64, 320, 16),
]


# ------------------------------------------------------------------------------------------------------------------ operands
@functools.lru_cache(maxsize=2)
def case_of(rows, K, N, ns):
    return R.case(rows, K, N, ns, seed=1000 * rows + K + N + ns)


def operands(c, dev, lay):
    """The inputs of one launch in layout `lay`: z, g and zp between 128 NaN rows, arg contiguous between INDEX_FILL words, the
    constant vectors 16-byte aligned between NaNs."""
    o = types.SimpleNamespace(z=gput(c["z"], dev, lay["z"]), g=gput(c["g"], dev, lay["g"]), zp=gput(c["zp"], dev, lay["zp"]),
                              arg=embed(c["arg"].to(dev), aligned=True) if c["ns"] else None)
    for k in CONSTS:
        setattr(o, k, embed(c[k].to(dev), aligned=True))
    o.all = [o.z, o.g, o.zp] + ([o.arg] if o.arg is not None else []) + [getattr(o, k) for k in CONSTS]
    return o


def outputs(c, dev, lay, chunks, want_dz=True):
    return (gout((c["rows"], c["N"]), dev, lay["out"]), gout((c["rows"], c["K"]), dev, lay["dz"]) if want_dz else None,
            guarded((chunks * 2 * c["N"],), F64, device=dev))


def fire(dev, c, wp, o, out, dz, part, **over):
    """One launch of the entry point; `over` replaces members of the input descriptor or arguments (the refusals)."""
    adr = lambda t: t.data_ptr() if t is not None else None
    f = dict(g=adr(o.g), ldg=o.g.stride(0), arg=adr(o.arg), ns=c["ns"], z=adr(o.z), ldz=o.z.stride(0), k1=adr(o.k1), c0=adr(o.c0), c1=adr(o.c1),
             mean=adr(o.mean), act_a=adr(o.act_a), act_b=adr(o.act_b), dz_out=adr(dz), ldd=dz.stride(0) if dz is not None else 0)
    a = dict(rows=c["rows"], K=c["K"], N=c["N"], Z=adr(o.zp), ldzp=o.zp.stride(0), mp=adr(o.mp), ip=adr(o.ip), ap=adr(o.ap), bp=adr(o.bp),
             out=adr(out), ldo=out.stride(0), sums_partial=adr(part), partial_elems=part.numel())
    for k, v in over.items():
        (f if k in f else a)[k] = v
    from ptt_amd import _lib
    d = _lib.BnBwdInput(**f)
    V = ctypes.c_void_p
    L(ENTRY, dev, ctypes.byref(d), a["rows"], a["K"], P(wp), a["N"], V(a["Z"]), a["ldzp"], V(a["mp"]), V(a["ip"]), V(a["ap"]), V(a["bp"]),
      V(a["out"]), a["ldo"], V(a["sums_partial"]), a["partial_elems"])


def verify(c, ref, out, dz, part, chunks):
    """The value bounds of tests/test_round5_gpu.py on one launch's outputs; `ref` = the float64 reference on the device."""
    N = c["N"]
    if dz is not None:
        # |dz - ref| <= 1e-5 (1 + |ref|) for every element                                                 tests/test_round5_gpu.py:256
        bad = int(((dz.double() - ref.dz).abs() > 1e-5 * (1 + ref.dz.abs())).sum())
        assert bad == 0, "%d elements of dz are not c0 + c1 (z - mean) + (mask ? k1 g : 0)" % bad
        # mask off and c1 == 0: fma(0, z - mean, c0) is c0 itself
        off = ~ref.mask[:, ref.c1zero]
        assert bool(off.any())
        want = ref.c0.expand(c["rows"], c["K"])[:, ref.c1zero]
        assert torch.equal(dz[:, ref.c1zero][off].view(I32), want[off].view(I32)), "dz != c0 where the mask is off and c1 == 0"
    o64 = out.double()
    assert float((o64 - ref.out).abs().max()) <= 2e-6 * float(ref.out.abs().max())                          # :260
    # the backward sums of the layer below, against sums formed from the kernel's own out                   :262-265
    dy = torch.where(ref.lower_on, o64, torch.zeros_like(o64))
    dyx = dy * ref.xhat
    sums = part.view(chunks, 2, N).sum(0)
    e0, b0 = float((sums[0] - dy.sum(0)).abs().max()), 1e-6 * float(dy.abs().sum(0).max())
    e1, b1 = float((sums[1] - dyx.sum(0)).abs().max()), 1e-6 * float(dyx.abs().sum(0).max())
    print("    sum dy off by %.3g (bound %.3g), sum dy * xhat off by %.3g (bound %.3g)" % (e0, b0, e1, b1))
    assert e0 <= b0 and e1 <= b1


def device_ref(c, dev):
    ref, d = c["ref"], lambda t: t.to(dev)
    zp64 = c["zp"].double()
    return types.SimpleNamespace(dz=d(ref["dz"]), out=d(ref["out"]), mask=d(ref["mask"]), c1zero=d(c["c1"] == 0), c0=d(c["c0"]),
                                 lower_on=d(zp64 * c["ap"].double() + c["bp"].double() > 0),
                                 xhat=d((zp64 - c["mp"].double()) * c["ip"].double()))


# --------------------------------------------------------------------------------------------------------------------- the launches
@pytest.mark.parametrize("form,spec,K,N,ns", SHAPES, ids=lambda v: str(v).replace(", ", ""))
def test_fused_bnbwd_gemm(dev, form, spec, K, N, ns):
    """Three layouts against one reference; per layout: with dz_out, again, and with dz_out = NULL. Everything bit-identical across
    all nine launches, and to ptt_rows_gemm_bnbwd_f32 run on the dz that was written (the chain identity: the same LDS contents
    for the valid rows, the same MFMA order, the same epilogue; the rows past the end differ — zeros against c0 - c1 * mean —
    and must not matter)."""
    from ptt_amd import ops
    CU = torch.cuda.get_device_properties(dev).multi_processor_count
    rows = resolve(spec, ns, CU)
    got_form, tiles, G, chunks = geom(rows, K, N, CU)
    assert got_form == form, "rows=%d K=%d N=%d was meant for form %s, this device gives it %s" % (rows, K, N, form, got_form)
    assert int(ops._host("ptt_rows_gemm_stat_chunks", rows, K, N)) == chunks, "the launch took another geometry than %s" % form
    if N % 256 == 0:          # the chunk count tells the two class-a forms apart
        assert geom(rows, K, N, CU, force_ct=3 - int(form[-1]))[3] != chunks
    if isinstance(spec, str):
        assert tiles > G, "several row tiles per workgroup were meant"
    assert ops._host("ptt_rows_gemm_bnbwd_fused_supported", rows, K, N, ns) == 1
    c = case_of(rows, K, N, ns)
    ref = device_ref(c, dev)
    wp = ops.pack_weight(c["w"].to(dev))
    first = None
    names = ("out", "partials", "dz")
    for name, lay in LAYOUTS.items():
        o = operands(c, dev, lay)
        runs = []
        for want_dz in (True, True, False):
            out, dz, part = outputs(c, dev, lay, chunks, want_dz)
            fire(dev, c, wp, o, out, dz, part)
            # written once and everywhere: no element of out, dz and the partials keeps its sentinel, no word around them, in the
            # ld - K gaps or of a row past the end is touched; no input changed
            checked(out, part, *([dz] if want_dz else []), inputs=o.all)
            print("%s, %s, dz_out %s:" % (c["rows"], name, "given" if want_dz else "NULL"))
            verify(c, ref, out, dz, part, chunks)
            runs.append((out, dz, part))
        (out, dz, part), (out2, dz2, part2), (out3, _, part3) = runs
        got = host(out, part, dz)
        same_bits(got, host(out2, part2, dz2), ["%s (%s, launched again)" % (n, name) for n in names])
        same_bits(got[:2], host(out3, part3), ["%s (%s, dz_out = NULL)" % (n, name) for n in names])
        # the chain identity: the unfused epilogue kernel on X = the dz this launch wrote
        yb, _, stb = outputs(c, dev, lay, chunks, False)
        L("ptt_rows_gemm_bnbwd_f32", dev, P(dz), rows, K, dz.stride(0), P(wp), N, P(o.zp), o.zp.stride(0), P(o.mp), P(o.ip), P(o.ap), P(o.bp),
          P(yb), yb.stride(0), P(stb), stb.numel())
        checked(yb, stb, dz, inputs=(o.zp,))
        same_bits(got[:2], host(yb, stb), ["%s (%s, ptt_rows_gemm_bnbwd_f32 on the written dz)" % (n, name) for n in names])
        if first is None:
            first = got
        else:
            same_bits(first, got, ["%s (%s vs dense)" % (n, name) for n in names])
    RAN.setdefault((form, ns), []).append((rows, K, N))


# ----------------------------------------------------------------------------------------------------------------------- refusals
def refused(dev, status, c, wp, o, chunks, **over):
    """The launch with `over` must fail with `status` and leave every word of the three outputs as it was."""
    out, dz, part = outputs(c, dev, LAYOUTS["dense"], chunks)
    with pytest.raises(RuntimeError, match=status):
        fire(dev, c, wp, o, out, dz, part, **over)
    guard.assert_untouched(out, dz, part)


def test_refusals_write_nothing(dev):
    from ptt_amd import ops
    sup = lambda rows, K, N, ns: ops._host("ptt_rows_gemm_bnbwd_fused_supported", rows, K, N, ns)
    chunks_of = lambda c: max(1, int(ops._host("ptt_rows_gemm_stat_chunks", c["rows"], c["K"], c["N"])))
    pack = lambda c: ops.pack_weight(c["w"].to(dev))
    lay = LAYOUTS["dense"]
    UNS, INV = "PTT_EUNSUPPORTED", "PTT_EINVAL"
    # ---- the dense form
    c = R.case(17, 128, 128, 0, seed=1)
    K, N = c["K"], c["N"]
    o, wp, chunks = operands(c, dev, lay), pack(c), chunks_of(c)
    some_arg = embed(torch.zeros(17, K, dtype=I32).to(dev))
    assert sup(17, K, N, 0) == 1
    refused(dev, UNS, c, wp, o, chunks, ldz=K + 3)
    refused(dev, UNS, c, wp, o, chunks, ldg=K + 3)
    refused(dev, UNS, c, wp, o, chunks, ldd=K + 3)
    refused(dev, INV, c, wp, o, chunks, z=o.z.data_ptr() + 4)
    refused(dev, INV, c, wp, o, chunks, g=o.g.data_ptr() + 4)
    dz_off = guarded((17, K), F32, device=dev)
    refused(dev, INV, c, wp, o, chunks, dz_out=dz_off.data_ptr() + 4)
    guard.assert_untouched(dz_off)
    refused(dev, INV, c, wp, o, chunks, arg=some_arg.data_ptr())                    # arg given with ns = 0
    refused(dev, INV, c, wp, o, chunks, ldd=K - 4)
    refused(dev, INV, c, wp, o, chunks, ldzp=N - 1)
    refused(dev, INV, c, wp, o, chunks, partial_elems=chunks * 2 * N - 1)
    for k in CONSTS + ("Z", "sums_partial"):
        refused(dev, INV, c, wp, o, chunks, **{k: None})
    # ---- the pooled form
    c = R.case(48, 128, 128, 16, seed=2)
    o, wp, chunks = operands(c, dev, lay), pack(c), chunks_of(c)
    assert sup(48, K, N, 16) == 1 and sup(48, K, N, 8) == 0 and sup(40, K, N, 16) == 0
    refused(dev, UNS, c, wp, o, chunks, ns=8)
    refused(dev, UNS, c, wp, o, chunks, rows=40)                                    # rows % ns != 0
    refused(dev, UNS, c, wp, o, chunks, ldz=K + 3)
    refused(dev, UNS, c, wp, o, chunks, ldg=K + 3)
    refused(dev, INV, c, wp, o, chunks, arg=None)                                   # arg missing with ns = 16
    refused(dev, INV, c, wp, o, chunks, arg=o.arg.data_ptr() + 4)
    refused(dev, INV, c, wp, o, chunks, g=o.g.data_ptr() + 4)
    check_guard(o.arg, all_written=False)
    # ---- class b: 128-row x 64-channel tiles have no registers left for the second operand stream
    c = R.case(64, 64, 128, 0, seed=3)
    o, wp = operands(c, dev, lay), pack(c)
    assert sup(64, 64, 128, 0) == 0 and sup(64, 64, 128, 32) == 0
    refused(dev, UNS, c, wp, o, chunks_of(c))
    RAN["refusals"] = True


def test_query_answers_for_every_shape_as_the_launch_does(dev):
    """ptt_rows_gemm_bnbwd_fused_supported on the shapes of this file (1: test_fused_bnbwd_gemm launches them) and on their class-b and
    odd-group neighbours (0: test_refusals_write_nothing shows the launch refusing those)."""
    from ptt_amd import ops
    CU = torch.cuda.get_device_properties(dev).multi_processor_count
    sup = lambda rows, K, N, ns: ops._host("ptt_rows_gemm_bnbwd_fused_supported", rows, K, N, ns)
    for form, spec, K, N, ns in SHAPES:
        rows = resolve(spec, ns, CU)
        assert sup(rows, K, N, ns) == 1
        assert sup(rows, K, N, 8) == 0 and sup(rows, 64, 128, ns) == 0 and sup(rows, K + 4, N, ns) == 0
        if ns:
            assert sup(rows + 1, K, N, ns) == 0


# ------------------------------------------------------------------------------------------------------ coverage report (last)
def test_zz_every_instantiation_ran():
    """All 12 (tile geometry, A-operand form) pairs ran in this process — a shape that took another geometry than the one it was
    written for has already failed its own test; one that was dropped from SHAPES fails here. Needs the whole file to have run."""
    for key in sorted(k for k in RAN if k != "refusals"):
        print("%-8s %-10s %s" % (key[0], "dense" if not key[1] else "pooled %d" % key[1], ", ".join("%dx%dx%d" % s for s in RAN[key])))
    missing = [(f, ns) for f in ("a, CT 1", "a, CT 2", "c") for ns in (0, 16, 32, 64) if (f, ns) not in RAN]
    assert not missing, "instantiations that did not run: %s" % missing
