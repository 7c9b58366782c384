"""Weight packing (ptt_pack_weight_f32, _rot_f32, _strided_f32, ptt_pack_weights_f32, ptt_packed_weight_elems: mfma_ops.hip) and
ptt_grad_finish_f32 (train_ops.hip: grad_finish_kernel) behind guard bands (tests/guard.py). Every comparison here is BITWISE.

Packing: the layout every MFMA kernel reads, [K8][Cout32][64 lanes][4] of include/ptt_hip.h, is restated in numpy (packed_ref) and
compared with what the four entry points write into guarded buffers of exactly ptt_packed_weight_elems floats — ragged Cout and
K, rotated input channels with K % 8 != 0, transposed and batched strides, padding that must be +0.0.

Grad finish: "a fixed summation tree per (job list)" is emulated in numpy float32 with sequential adds only (finish_ref): chunk c
of job j goes to thread group (kbase_j + c) % G, G = 256 / out, every group adds its chunks in ascending order starting from 0,
the groups are folded 0 .. G - 1, and the total is added to what the destination holds. A float64 sum with a tolerance and
run-to-run equality (tests/test_grad_sink_gpu.py) cannot tell this tree from another valid one; the bits can: the same emulation
with the group taken as c % G (the second job of a destination starting again at group 0) is shown NOT to match the device.

What this does not prove: a stray READ whose value is discarded goes unseen."""
import ctypes

import numpy as np
import pytest
import torch

from tests import guard
from tests.guard import SENTINEL, check_guard, embed, guarded
from tests.test_strided_guard_gpu import checked, gen

pytestmark = pytest.mark.gpu
L, P = guard.launch, guard.ptr
F32, I32 = torch.float32, torch.int32


def bits(t):
    """A float32 tensor or array -> its bit patterns as a flat int32 numpy array."""
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().contiguous().numpy()
    return np.ascontiguousarray(t, dtype=np.float32).view(np.int32).reshape(-1)


# ================================================================================================================ weight packing
def packed_ref(W, rot=0):
    """include/ptt_hip.h, "Weight packing": W (Cout,K) -> [K8][Cout32][64 lanes][4], packed position k = channel (k + rot) mod K,
    zeros where col >= Cout or k >= K. -> (packed float32, the boolean map of the elements that hold a weight)."""
    Cout, K = W.shape
    NT, NKB = (Cout + 31) // 32, (K + 7) // 8
    e = np.arange(NT * NKB * 256)
    j, lane, tile = e & 3, (e >> 2) & 63, e >> 8
    ct, kb = tile % NT, tile // NT
    col, k = 32 * ct + (lane & 31), 8 * kb + 4 * (lane >> 5) + j
    real = (col < Cout) & (k < K)
    out = np.zeros(e.shape, dtype=np.float32)
    out[real] = W[col[real], (k[real] + rot) % K]
    return out, real


def weight(Cout, K, seed, batch=None):
    shape = (Cout, K) if batch is None else (batch, Cout, K)
    w = torch.randn(*shape, generator=gen(seed))
    assert bool((w != 0).all())                                 # a padding zero is never mistaken for a weight
    return w


def elems_of(Cout, K):
    from ptt_amd import ops
    n = int(ops._host("ptt_packed_weight_elems", Cout, K))
    assert n == ((Cout + 31) // 32) * ((K + 7) // 8) * 256
    return n


def assert_pack(packed, want, real, what):
    """The guards hold, every element was written, the bits are the restated layout's and the padding is +0.0."""
    check_guard(packed)
    got = bits(packed)
    assert np.array_equal(got, bits(want)), "%s: not the layout of include/ptt_hip.h" % what
    assert not got.reshape(-1, real.size)[:, ~real].any(), "%s: padding that is not +0.0" % what


PACK_SHAPES = [(1, 1), (5, 3), (32, 8), (33, 9), (64, 67), (259, 256), (256, 259)]


@pytest.mark.parametrize("Cout,K", PACK_SHAPES)
def test_pack_weight_and_rot(dev, Cout, K):
    """ptt_pack_weight_f32 and ptt_pack_weight_rot_f32 with rot in {0, 3, K - 1}: exactly ptt_packed_weight_elems floats, the
    restated layout, +0.0 padding, the same bits as ops.pack_weight, the weight untouched."""
    from ptt_amd import ops
    w = weight(Cout, K, 100 * Cout + K)
    n = elems_of(Cout, K)
    wd = embed(w.to(dev))
    want, real = packed_ref(w.numpy())
    assert want.size == n
    p = guarded((n,), F32, device=dev, aligned=True)
    L("ptt_pack_weight_f32", dev, P(wd), Cout, K, P(p))
    assert_pack(p, want, real, "ptt_pack_weight_f32")
    assert np.array_equal(bits(p), bits(ops.pack_weight(w.to(dev))))
    for rot in sorted({0, 3, K - 1}) if K > 3 else [0]:
        want, real = packed_ref(w.numpy(), rot)
        p = guarded((n,), F32, device=dev, aligned=True)
        L("ptt_pack_weight_rot_f32", dev, P(wd), Cout, K, rot, P(p))
        assert_pack(p, want, real, "ptt_pack_weight_rot_f32, rot = %d" % rot)
        assert np.array_equal(bits(p), bits(ops.pack_weight(w.to(dev), rot)))
    check_guard(wd, all_written=False)
    assert bits(wd).tolist() == bits(w).tolist()


@pytest.mark.parametrize("Cout,K", [(5, 3), (33, 9), (64, 67)])
def test_pack_weight_strided(dev, Cout, K):
    """ptt_pack_weight_strided_f32 on a plain weight with ld > K, on a transposed one (stride_out 1, stride_k = ld), on a batch of 3
    whose batch stride is larger than the matrix, and with batch = 0 (nothing written)."""
    from ptt_amd import ops
    n = elems_of(Cout, K)
    w = weight(Cout, K, 7 * Cout + K)
    want, real = packed_ref(w.numpy())
    # plain, ld = K + 5 at column 1
    wd = embed(w.to(dev), ld=K + 5, col_off=1)
    p = guarded((1, n), F32, device=dev, aligned=True)
    L("ptt_pack_weight_strided_f32", dev, P(wd), Cout, K, wd.stride(0), 1, 1, 0, P(p))
    assert_pack(p, want, real, "plain")
    assert np.array_equal(bits(p), bits(ops.pack_weight(w.to(dev))))
    assert np.array_equal(bits(ops.pack_weight_strided(wd, Cout, K, wd.stride(0), 1, 1, 0)), bits(want))
    check_guard(wd, all_written=False)
    # transposed in memory: (K, Cout) rows with ld = Cout + 3
    wt = embed(w.t().contiguous().to(dev), ld=Cout + 3, col_off=2)
    p = guarded((1, n), F32, device=dev, aligned=True)
    L("ptt_pack_weight_strided_f32", dev, P(wt), Cout, K, 1, wt.stride(0), 1, 0, P(p))
    assert_pack(p, want, real, "transposed")
    check_guard(wt, all_written=False)
    # a batch of 3, batch stride > Cout * ld
    w3 = weight(Cout, K, 11 * Cout + K, batch=3)
    ld = K + 2
    wb = embed(w3.to(dev), ld=ld, col_off=1, batch_stride=Cout * ld + 7)
    p = guarded((3, n), F32, device=dev, aligned=True)
    L("ptt_pack_weight_strided_f32", dev, P(wb), Cout, K, ld, 1, 3, Cout * ld + 7, P(p))
    want3 = np.stack([packed_ref(w3[b].numpy())[0] for b in range(3)])
    assert_pack(p, want3, real, "batch of 3")
    for b in range(3):
        assert np.array_equal(bits(p[b]), bits(ops.pack_weight(w3[b].to(dev))))
    check_guard(wb, all_written=False)
    # batch = 0: a valid call that writes nothing
    p = guarded((1, n), F32, device=dev, aligned=True)
    L("ptt_pack_weight_strided_f32", dev, P(wb), Cout, K, ld, 1, 0, Cout * ld + 7, P(p))
    guard.assert_untouched(p)


def test_pack_weights_table(dev):
    """ptt_pack_weights_f32: five jobs of mixed shapes, one of them transposed, into one arena with guard words between the packs —
    the whole arena is compared: each pack is its weight's layout, every other word still holds the sentinel."""
    from ptt_amd import ops
    shapes = [(33, 9, False), (5, 3, False), (64, 67, True), (259, 256, False), (1, 1, False)]
    gaps = [8, 4, 12, 4, 8, 16]                                  # floats in front of job 0, between the jobs, behind the last
    jobs, inputs, off = [], [], gaps[0]
    expect = []
    for k, (Cout, K, transposed) in enumerate(shapes):
        w = weight(Cout, K, 1000 + k)
        if transposed:
            wd = embed(w.t().contiguous().to(dev), ld=Cout + 4)
            so, sk = 1, wd.stride(0)
        else:
            wd = embed(w.to(dev), ld=K + 3, col_off=1)
            so, sk = wd.stride(0), 1
        assert off % 4 == 0
        jobs.append((wd.data_ptr(), off, so, sk, Cout, K))
        inputs.append(wd)
        expect.append((off, packed_ref(w.numpy())[0], w))
        off += elems_of(Cout, K) + gaps[k + 1]
    arena = guarded((off,), F32, device=dev, aligned=True)
    table = ops.pack_jobs_table(jobs, dev)
    L("ptt_pack_weights_f32", dev, P(table), len(jobs), P(arena))
    check_guard(arena, all_written=False)
    want = np.full((off,), SENTINEL, dtype=np.int32)
    for o, ref, _ in expect:
        want[o:o + ref.size] = bits(ref)
    assert np.array_equal(bits(arena), want)
    for (o, ref, w), wd in zip(expect, inputs):
        assert np.array_equal(bits(arena[o:o + ref.size]), bits(ops.pack_weight(w.to(dev))))
        check_guard(wd, all_written=False)
    # n_jobs = 0 is a valid call that writes nothing
    arena0 = guarded((off,), F32, device=dev, aligned=True)
    L("ptt_pack_weights_f32", dev, P(table), 0, P(arena0))
    guard.assert_untouched(arena0)


def test_pack_refusals_write_nothing(dev):
    from ptt_amd import ops
    Cout, K = 33, 9
    wd = embed(weight(Cout, K, 5).to(dev))
    n = elems_of(Cout, K)
    p = guarded((n,), F32, device=dev, aligned=True)
    INV = "PTT_EINVAL"
    for rot in (K, -1):
        with pytest.raises(RuntimeError, match=INV):
            L("ptt_pack_weight_rot_f32", dev, P(wd), Cout, K, rot, P(p))
    for args in ((P(wd), 0, K, P(p)), (P(wd), Cout, 0, P(p)), (None, Cout, K, P(p)), (P(wd), Cout, K, None)):
        with pytest.raises(RuntimeError, match=INV):
            L("ptt_pack_weight_f32", dev, *args)
    for args in ((P(wd), 0, K, K, 1, 1, 0, P(p)), (None, Cout, K, K, 1, 1, 0, P(p)), (P(wd), Cout, K, K, 1, 1, 0, None), (P(wd), Cout, K, K, 1, -1, 0, P(p))):
        with pytest.raises(RuntimeError, match=INV):
            L("ptt_pack_weight_strided_f32", dev, *args)
    table = ops.pack_jobs_table([(wd.data_ptr(), 0, K, 1, Cout, K)], dev)
    with pytest.raises(RuntimeError, match="PTT_EUNSUPPORTED"):
        L("ptt_pack_weights_f32", dev, P(table), 65536, P(p))
    for args in ((None, 1, P(p)), (P(table), 1, None), (P(table), -1, P(p))):
        with pytest.raises(RuntimeError, match=INV):
            L("ptt_pack_weights_f32", dev, *args)
    assert ops._host("ptt_packed_weight_elems", 0, K) == 0 and ops._host("ptt_packed_weight_elems", Cout, 0) == 0
    guard.assert_untouched(p)
    check_guard(wd, all_written=False)


# =================================================================================================================== grad finish
def finish_ref(dest, parts, out, ignore_kbase=False):
    """The fixed tree of grad_finish_kernel for one destination, float32, sequential adds only. dest (n,) = what the destination
    holds, parts = the (nchunks, n) partials of its jobs in job order, out = outputs per workgroup. ignore_kbase: the MUTANT that
    starts every job at group 0."""
    G = 256 // out
    acc = np.zeros((G, dest.size), dtype=np.float32)
    kbase = 0
    for part in parts:
        for c in range(part.shape[0]):
            grp = (c if ignore_kbase else kbase + c) % G
            acc[grp] = acc[grp] + part[c]
        kbase += part.shape[0]
    tot = acc[0].copy()
    for q in range(1, G):
        tot = tot + acc[q]
    return dest + tot


def vec_loop_counts(chunks, out):
    """-> (iterations of the four-loads-in-flight loop, iterations of the remainder loop) over all thread groups and jobs of a
    float4 destination (train_ops.hip: `for (; c + 3 * G < nchunks; c += 4 * G)`, then `for (; c < nchunks; c += G)`)."""
    G = 256 // out
    four = rem = kbase = 0
    for nch in chunks:
        for g in range(G):
            c = (g - kbase % G) % G
            m = len(range(c, nch, G))
            four, rem = four + m // 4, rem + m % 4
        kbase += nch
    return four, rem


def splits_of(T):
    """T chunks over one, two and three jobs; the first job of a split never ends on a multiple of G where G > 1 allows it."""
    s = [[T]]
    if T >= 2:
        s.append([max(1, T // 3), T - max(1, T // 3)])
    if T >= 3:
        a, b = max(1, T // 3), max(1, T // 5)
        s.append([a, b, T - a - b])
    return s


# destination -> (n, cols, ld, float4-addressable): a vec segment with ld > cols whose 257 units end inside a workgroup, a scalar
# column slice, a single element, five elements
DESTS = [(1028, 4, 8, 1), (3 * 64, 3, 67, 0), (1, 1, 1, 0), (5, 5, 5, 0)]
FINISH_TOTALS = [1, 2, 3, 8, 9, 64, 65, 256, 257, 1024, 1025]        # both sides of every step of _outputs_per_group


@pytest.mark.parametrize("T", FINISH_TOTALS)
def test_grad_finish_is_the_documented_tree(dev, T):
    from ptt_amd import _lib, ops
    out = ops.GradFinishPlan._outputs_per_group(T)
    G = 256 // out
    assert out == (4 if T > 1024 else 8 if T > 256 else 16 if T > 64 else 32 if T > 8 else 64 if T > 2 else 256)
    four = rem = 0
    offsets_seen = told_apart = False
    for chunks in splits_of(T):
        assert sum(chunks) == T and min(chunks) >= 1
        g = gen(1000 * T + len(chunks))
        # ---- the flat buffer: NaN words in front of, between and behind the destinations
        gap, dsts, pos = 12, [], 8
        for n, cols, ld, vec in DESTS:
            pos += 1 if not vec and n > 1 else 0                # the scalar slice starts off 16 bytes
            dsts.append(pos)
            pos += (n // cols - 1) * ld + cols + gap
            pos += -pos % 4
        flat0 = torch.full((pos,), float("nan"))
        flat0.view(I32)[:] = SENTINEL
        idx = [d + (np.arange(n) // cols) * ld + np.arange(n) % cols for d, (n, cols, ld, _) in zip(dsts, DESTS)]
        for ix in idx:
            flat0[torch.from_numpy(ix)] = torch.randn(ix.size, generator=g)
        flat = embed(flat0.to(dev), aligned=True)
        # ---- the tables
        segs = (_lib.GradSegment * len(DESTS))()
        jobs = (_lib.GradJob * (len(DESTS) * len(chunks)))()
        blocks, parts, part_views = [], [], []
        for si, (n, cols, ld, vec) in enumerate(DESTS):
            assert not vec or (n % 4 == 0 and cols % 4 == 0 and ld % 4 == 0 and dsts[si] % 4 == 0)
            segs[si] = _lib.GradSegment(dst=dsts[si], n=n, cols=cols, ld=ld, job0=si * len(chunks), njobs=len(chunks), out=out, vec=vec, reserved=0)
            parts.append([torch.randn(nch, n, generator=g) for nch in chunks])
            for j, pt in enumerate(parts[-1]):
                pv = embed(pt.to(dev), aligned=True if vec else None)
                part_views.append(pv)
                jobs[si * len(chunks) + j] = _lib.GradJob(partial=pv.data_ptr(), nchunks=pt.shape[0], reserved=0)
            for u in range(0, n // 4 if vec else n, out):
                blocks += [si, u]
        up = lambda raw: embed(torch.frombuffer(bytearray(raw), dtype=torch.uint8).view(I32).clone().to(dev))
        segs_d, jobs_d, blocks_d = up(bytes(segs)), up(bytes(jobs)), embed(torch.tensor(blocks, dtype=I32).to(dev))
        L("ptt_grad_finish_f32", dev, P(segs_d), P(jobs_d), P(blocks_d), len(blocks) // 2, P(flat))
        checked(inputs=[flat, segs_d, jobs_d, blocks_d] + part_views)
        # ---- the emulated tree, bit for bit; everything outside the destinations as it was
        want = flat0.numpy().copy()
        mutant = want.copy()
        for ix, pts in zip(idx, parts):
            pn = [p.numpy() for p in pts]
            want[ix] = finish_ref(flat0.numpy()[ix], pn, out)
            mutant[ix] = finish_ref(flat0.numpy()[ix], pn, out, ignore_kbase=True)
        got = bits(flat)
        where = "%d chunks as %s, out = %d" % (T, chunks, out)
        assert np.array_equal(got, bits(want)), "not the documented summation tree: " + where
        offsets_seen |= any(k % G for k in np.cumsum([0] + chunks[:-1]))
        # the tree that ignores kbase is another valid sum of the same chunks; where it gives other bits, the device sides with `want`
        told_apart |= not np.array_equal(bits(mutant), bits(want))
        f, r = vec_loop_counts(chunks, out)
        four, rem = four + f, rem + r
    assert offsets_seen or G == 1, "no job of this case starts off group 0"
    # from 8 chunks on a second job's groups differ from a fresh start in more than their fold order: the bits tell the trees apart
    # (below that the two trees add the same numbers in the same order)
    assert told_apart or T < 8, "this case cannot tell the documented tree from the one that ignores kbase"
    # both loops of the float4 path ran (counted from the chunk lists, not observed)
    assert rem > 0 and (four > 0 or T < 64), (T, four, rem)


def test_grad_finish_refusals_write_nothing(dev):
    flat = guarded((64,), F32, device=dev, aligned=True)
    t = embed(torch.zeros(16, dtype=I32).to(dev))
    V = ctypes.c_void_p
    for args in ((P(t), P(t), P(t), -1, P(flat)), (None, P(t), P(t), 1, P(flat)), (P(t), None, P(t), 1, P(flat)), (P(t), P(t), None, 1, P(flat)),
                 (P(t), P(t), P(t), 1, None), (P(t), P(t), P(t), 1, V(flat.data_ptr() + 4))):
        with pytest.raises(RuntimeError, match="PTT_EINVAL"):
            L("ptt_grad_finish_f32", dev, *args)
    L("ptt_grad_finish_f32", dev, P(t), P(t), P(t), 0, P(flat))                     # no workgroups: a valid call
    guard.assert_untouched(flat)


@pytest.mark.parametrize("R,C", [(300, 5), (9000, 64)])
def test_colsum_is_its_partials_finished_by_the_plan(dev, R, C):
    """ops.colsum (ptt_colsum_f32: the partials finished by launch_wgrad_finish) and ops.colsum_partials + GradFinishPlan into a
    zeroed buffer are the same sum, bit for bit (train_ops.hip: "the SAME function as ops.GradFinishPlan._outputs_per_group")."""
    from ptt_amd import ops
    x = torch.randn(R, C, generator=gen(R + C)).to(dev)
    ref = ops.colsum(x)
    ws, nch = ops.colsum_partials(x)
    assert nch >= 1
    flat = torch.zeros((C + 3) // 4 * 4, device=dev)
    ops.GradFinishPlan(dev).run([(0, C, C, C, ws.data_ptr(), nch)], flat)
    assert np.array_equal(bits(flat[:C]), bits(ref)), "colsum and the plan disagree at %d chunks" % nch
