"""The index ops of the C ABI (point_ops.hip, and the row gather / CSR scatter pair of train_ops.hip) write only their outputs.

The method of tests/test_strided_guard_gpu.py for entry points that take whole dense tensors: every launch goes through
guard.launch with every output in a guarded(...) buffer of exactly its size, every workspace in guard.workspace(...) of exactly
the size its query returns, and every input embed(...)-ded between NaN / INDEX_FILL words (an index read one element too far is
an index no cloud has). Asserted per launch: check_guard on every output (all written), on every workspace and input (nothing
written); the values as the existing tests assert them — bit-exact against oracle.index_ops (tests/test_point_ops_gpu.py:36,
62, 72-82, 116), exact against torch.gather (tests/test_train_gpu.py:429), and for the scatters the bounds of their tests
restated with the source line; no bound is new — and every guarded result equals, bit for bit, what the plain ops.* wrapper
returns for the same inputs (the two atomicAdd backward kernels excepted: their summation order is not fixed, so two runs of
the same launch need not agree in the last bit; they are held to the bound of tests/test_point_ops_gpu.py:103-106 only).

Shapes: B = 3 with one duplicated cloud (cloud 1 repeats cloud 0) and one all-zero cloud; N in {65, 200}, M in {7, 33}, ns in
{16, 32}, k = 16, C in {4, 131} (the row kernels need C % 4 == 0: {4, 132}); the CSR pair at (N, E) = (100, 37) and
(2049, 4096) — the second takes the bitonic path above 2048 bins.

The training-only row kernels (xcorr_z0*, sa_z0*, the partial-sum finishers, pt_attn_train_bwd, unit_rows / cos_bwd_rows) are in
tests/test_train_rows_guard_gpu.py, the fused SA / xcorr / pair kernels in tests/test_fused_guard_gpu.py, the row kernels in
tests/test_strided_guard_gpu.py (ptt_rows_gemm_bnbwd_fused_f32, the one entry point on rows_gemm_kernel that file leaves out, in
tests/test_gemm_fused_guard_gpu.py against tests/gemm_fused_ref.py; the weight packing entry points and ptt_grad_finish_f32, bit
for bit against their restated layout and summation tree, in tests/test_pack_finish_guard_gpu.py), the crop / resample / select
kernels of track_ops.hip in tests/test_track_ops_guard_gpu.py,
track_losses* and the Adam pair in tests/test_step_guard_gpu.py (ptt_optim_clip_step*: tests/test_optimization_gpu.py,
ptt_crop_scan_f32: tests/test_scan_crop_gpu.py). Out of scope of the guard-band files: ptt_box_overlap_f64 and
ptt_train_batch_f32, which have value tests at ragged sizes of their own in tests/test_eval_metrics_gpu.py and
tests/test_train_feed_gpu.py."""
import numpy as np
import pytest
import torch

from oracle import index_ops as O
from ptt_amd import _lib, ops, synth
from tests import guard
from tests.guard import check_guard, embed, guarded

pytestmark = pytest.mark.gpu
L, P = guard.launch, guard.ptr
F32, I32, I64 = torch.float32, torch.int32, torch.int64
B, K = 3, 16
RADIUS = 0.4


def clouds(N):
    s, _ = synth.frames(N, B, N, 64, K_s=max(16, N // 2))
    s[1] = s[0]                 # one duplicated cloud
    s[2] = 0.0                  # one all-zero cloud
    return s


def E(a, dev):
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    return embed(t.to(dev).contiguous())


def G(shape, dtype, dev):
    return guarded(shape, dtype, device=dev)


def WS(query, dev, *dims):
    n = (int(ops._host(query, *dims)) + 3) // 4 * 4
    return guard.workspace(n, device=dev), n


def done(outs, ins=(), ws=()):
    torch.cuda.synchronize()
    for v in outs:
        check_guard(v)
    for v in tuple(ins) + tuple(ws):
        check_guard(v, all_written=False)


def eq(got, want, what):
    want = torch.from_numpy(want) if isinstance(want, np.ndarray) else want
    assert got.dtype == want.dtype, what
    assert torch.equal(got.reshape(want.shape).cpu(), want.cpu()), what


# ------------------------------------------------------------------------------------------------------ sampling and centres
@pytest.mark.parametrize("N", [65, 200])
@pytest.mark.parametrize("M", [7, 33])
def test_fps_and_centres(dev, N, M):
    s = clouds(N)
    xyz = E(s, dev)
    ref = O.fps(s, M)
    plain = ops.furthest_point_sampling(xyz.contiguous(), M)
    out = G((B, M), I32, dev)
    L("ptt_fps_f32", dev, P(xyz), B, N, M, P(out))
    done([out], [xyz])
    eq(out, ref, "ptt_fps_f32 against the oracle")
    eq(out, plain, "ptt_fps_f32 against ops.furthest_point_sampling")

    out2, ws = G((B, M), I32, dev), guard.workspace(B * N * 4, device=dev)
    L("ptt_fps_ws_f32", dev, P(xyz), B, N, M, P(out2), P(ws), B * N)
    done([out2], [xyz], [ws])
    eq(out2, ref, "ptt_fps_ws_f32 against the oracle")

    sel = E(ref, dev)
    new_xyz, idx64 = G((B, M, 3), F32, dev), G((B, M), I64, dev)
    L("ptt_select_centres_f32", dev, P(xyz), P(sel), B, N, M, P(new_xyz), P(idx64))
    done([new_xyz, idx64], [xyz, sel])
    want = torch.gather(torch.from_numpy(s), 1, torch.from_numpy(ref).long()[..., None].expand(-1, -1, 3))
    eq(new_xyz, want, "ptt_select_centres_f32: centres")
    eq(idx64, torch.from_numpy(ref).long(), "ptt_select_centres_f32: int64 indices")
    p_new, p_64 = ops.select_centres(xyz.contiguous(), sel.contiguous(), M)
    eq(new_xyz, p_new, "against ops.select_centres")
    eq(idx64, p_64, "against ops.select_centres (idx64)")
    first = G((B, M, 3), F32, dev)                                       # idx NULL: the first M points, no idx64
    L("ptt_select_centres_f32", dev, P(xyz), None, B, N, M, P(first), None)
    done([first], [xyz])
    eq(first, torch.from_numpy(s[:, :M].copy()), "ptt_select_centres_f32 without a selection")


# --------------------------------------------------------------------------------------------------------------- ball query
@pytest.mark.parametrize("ns", [16, 32])
@pytest.mark.parametrize("N", [65, 200])
@pytest.mark.parametrize("M", [7, 33])
def test_ball_query_family(dev, N, M, ns):
    s = clouds(N)
    inds = O.fps(s, M)
    centres = np.take_along_axis(s, inds.astype(np.int64)[..., None], axis=1).copy()
    ref = O.ball_query(centres, s, RADIUS, ns)
    xyz, cen, sel = E(s, dev), E(centres, dev), E(inds, dev)
    plain = ops.ball_query(cen.contiguous(), xyz.contiguous(), RADIUS, ns)
    eq(plain, ref, "ops.ball_query against the oracle")

    out = G((B, M, ns), I32, dev)
    L("ptt_ball_query_f32", dev, P(cen), P(xyz), B, M, N, RADIUS, ns, P(out))
    done([out], [cen, xyz])
    eq(out, ref, "ptt_ball_query_f32")

    out = G((B, M, ns), I32, dev)
    ws, n = WS("ptt_ball_query_grid_workspace", dev, B, N)
    L("ptt_ball_query_grid_f32", dev, P(cen), P(xyz), B, M, N, RADIUS, ns, P(out), P(ws), n)
    done([out], [cen, xyz], [ws])
    eq(out, ref, "ptt_ball_query_grid_f32")

    for grid in (False, True):
        new_xyz, idx64, out = G((B, M, 3), F32, dev), G((B, M), I64, dev), G((B, M, ns), I32, dev)
        if grid:
            ws, n = WS("ptt_ball_query_grid_workspace", dev, B, N)
            L("ptt_centres_ball_query_grid_f32", dev, P(xyz), P(sel), B, N, M, RADIUS, ns, P(new_xyz), P(idx64), P(out), P(ws), n)
            done([new_xyz, idx64, out], [xyz, sel], [ws])
        else:
            L("ptt_centres_ball_query_f32", dev, P(xyz), P(sel), B, N, M, RADIUS, ns, P(new_xyz), P(idx64), P(out))
            done([new_xyz, idx64, out], [xyz, sel])
        what = "ptt_centres_ball_query%s_f32" % ("_grid" if grid else "")
        eq(out, ref, what)
        eq(new_xyz, centres, what + ": centres")
        eq(idx64, inds.astype(np.int64), what + ": int64 indices")
    p_new, p_64, p_idx = ops.centres_ball_query(xyz.contiguous(), sel.contiguous(), M, RADIUS, ns)
    eq(out, p_idx, "against ops.centres_ball_query")
    eq(new_xyz, p_new, "against ops.centres_ball_query (centres)")
    eq(idx64, p_64, "against ops.centres_ball_query (idx64)")


# ---------------------------------------------------------------------------------------------------------------------- kNN
@pytest.mark.parametrize("N", [16, 65, 200])
def test_knn(dev, N):
    s = clouds(N)
    ref = O.knn(s, K)
    xyz = E(s, dev)
    out = G((B, N, K), I32, dev)
    L("ptt_knn_f32", dev, P(xyz), B, N, K, P(out))
    done([out], [xyz])
    eq(out, ref, "ptt_knn_f32")
    out2, rel = G((B, N, K), I32, dev), G((B, N * K, 3), F32, dev)
    L("ptt_knn_rel_f32", dev, P(xyz), B, N, K, P(out2), P(rel))
    done([out2, rel], [xyz])
    eq(out2, ref, "ptt_knn_rel_f32")
    t = torch.from_numpy(s)
    nb = torch.gather(t, 1, torch.from_numpy(ref).long().reshape(B, N * K, 1).expand(-1, -1, 3)).view(B, N, K, 3)
    eq(rel, (t[:, :, None] - nb).reshape(B, N * K, 3), "ptt_knn_rel_f32: rel = xyz_i - xyz_neighbour")
    p_idx, p_rel = ops.knn(xyz.contiguous(), K, want_rel=True)
    eq(out2, p_idx, "against ops.knn")
    eq(rel, p_rel.view(B, N * K, 3), "against ops.knn (rel)")


# --------------------------------------------------------------------------------------------- gather / group and their backwards
@pytest.mark.parametrize("C", [4, 131])
@pytest.mark.parametrize("N,M,ns", [(65, 7, 16), (200, 33, 32), (65, 33, 32), (200, 7, 16)])
def test_gather_group_and_grads(dev, N, M, ns, C):
    rs = np.random.RandomState(N + M + C)
    feat = rs.standard_normal((B, C, N)).astype(np.float32)
    idx1 = rs.randint(0, N, (B, M)).astype(np.int32)
    idx2 = rs.randint(0, max(1, N // 4), (B, M, ns)).astype(np.int32)      # heavy duplication, as tests/test_point_ops_gpu.py:92
    idx2[0, :, 0] = N - 1
    go1 = rs.standard_normal((B, C, M)).astype(np.float32)
    go2 = rs.standard_normal((B, C, M, ns)).astype(np.float32)
    f, i1, i2, g1, g2 = E(feat, dev), E(idx1, dev), E(idx2, dev), E(go1, dev), E(go2.reshape(B, C, M * ns), dev)

    out = G((B, C, M), F32, dev)
    L("ptt_gather_f32", dev, P(f), P(i1), B, C, N, M, P(out))
    done([out], [f, i1])
    eq(out, O.gather(feat, idx1), "ptt_gather_f32")
    eq(out, ops.gather_points(f.contiguous(), i1.contiguous()), "against ops.gather_points")

    out = G((B, C, M * ns), F32, dev)
    L("ptt_group_f32", dev, P(f), P(i2), B, C, N, M, ns, P(out))
    done([out], [f, i2])
    eq(out, O.group(feat, idx2).reshape(B, C, M * ns), "ptt_group_f32")
    eq(out, ops.group_points(f.contiguous(), i2.contiguous()).view(B, C, M * ns), "against ops.group_points")

    # the deterministic scatter-add: entries added in ascending order = the oracle's sequential loop, bit-exact
    # (tests/test_point_ops_gpu.py:78-82), and what ops.gather_points_grad / group_points_grad run by default
    for src, idx, Ecount, ref, plain in ((g1, i1, M, O.gather_grad(go1, idx1, N), lambda: ops.gather_points_grad(g1.contiguous(), i1.contiguous(), N)),
                                         (g2, i2, M * ns, O.group_grad(go2, idx2, N),
                                          lambda: ops.group_points_grad(g2.contiguous().view(B, C, M, ns), i2.contiguous(), N))):
        out = G((B, C, N), F32, dev)
        ws, n = WS("ptt_scatter_add_det_workspace", dev, B, N, Ecount)
        L("ptt_scatter_add_det_f32", dev, P(src), P(idx), B, C, N, Ecount, P(out), P(ws), n)
        done([out], [src, idx], [ws])
        eq(out, ref, "ptt_scatter_add_det_f32 (E = %d)" % Ecount)
        eq(out, plain(), "against the ops.*_grad wrapper (E = %d)" % Ecount)

    # upstream's atomicAdd kernels: fp32 rounding in a free summation order (tests/test_point_ops_gpu.py:103-106)
    out = G((B, C, N), F32, dev)
    L("ptt_gather_grad_f32", dev, P(g1), P(i1), B, C, N, M, P(out))
    done([out], [g1, i1])
    np.testing.assert_allclose(out.cpu().numpy(), O.gather_grad(go1, idx1, N), rtol=1e-4, atol=1e-4)
    out = G((B, C, N), F32, dev)
    L("ptt_group_grad_f32", dev, P(g2), P(i2), B, C, N, M, ns, P(out))
    done([out], [g2, i2])
    np.testing.assert_allclose(out.cpu().numpy(), O.group_grad(go2, idx2, N), rtol=1e-4, atol=1e-4)


# ------------------------------------------------------------------------------------------------ row gather and the CSR scatter
@pytest.mark.parametrize("C", [4, 132])
@pytest.mark.parametrize("N,Ecount", [(100, 37), (2049, 4096)])
def test_rows_and_csr(dev, N, Ecount, C):
    g = torch.Generator(device="cpu").manual_seed(Ecount + C)
    rows = torch.randn(B, N, C, generator=g)
    idx = torch.randint(0, max(1, N // 3), (B, Ecount), generator=g).to(I32)
    idx[0, 0], idx[1, -1] = N - 1, N - 1                                   # the last bin is used too
    idx[2] = 0                                                             # one cloud with every entry in one bin
    up = torch.randn(B, Ecount, C, generator=g)
    minuend = torch.randn(B, N, C, generator=g)
    r, i, u, m = E(rows, dev), E(idx, dev), E(up, dev), E(minuend, dev)

    out = G((B, Ecount, C), F32, dev)
    L("ptt_gather_rows_f32", dev, P(r), P(i), B, N, Ecount, C, P(out))
    done([out], [r, i])
    eq(out, torch.gather(rows, 1, idx.long()[..., None].expand(-1, -1, C)), "ptt_gather_rows_f32")      # tests/test_train_gpu.py:429
    eq(out, ops.gather_rows(r.contiguous(), i.contiguous()), "against ops.gather_rows")

    order, start = G((B, Ecount), I32, dev), G((B, N + 1), I32, dev)
    L("ptt_scatter_csr_i32", dev, P(i), B, N, Ecount, P(order), P(start))
    done([order, start], [i])
    want_order = np.argsort(idx.numpy(), axis=1, kind="stable").astype(np.int32)        # sorted by (bin, entry)
    want_start = np.stack([np.searchsorted(np.sort(idx[b].numpy()), np.arange(N + 1), side="left") for b in range(B)]).astype(np.int32)
    eq(order, want_order, "ptt_scatter_csr_i32: order")
    eq(start, want_start, "ptt_scatter_csr_i32: start")
    p_order, p_start = ops.scatter_csr(i.contiguous(), N)
    eq(order, p_order, "against ops.scatter_csr (order)")
    eq(start, p_start, "against ops.scatter_csr (start)")

    ref = torch.zeros(B, N, C, dtype=torch.float64).index_put_((torch.arange(B)[:, None].expand(B, Ecount), idx.long()), up.double(),
                                                               accumulate=True)
    bound = lambda got, want: float((got.cpu().double() - want).abs().max()) <= 1e-5 * (float(want.abs().max()) + 1)   # test_train_gpu.py:434
    out = G((B, N, C), F32, dev)
    L("ptt_scatter_rows_csr_f32", dev, P(u), P(order), P(start), B, N, Ecount, C, P(out))
    done([out], [u, order, start])
    assert bound(out, ref), "ptt_scatter_rows_csr_f32"
    eq(out, ops.scatter_rows_det(u.contiguous(), i.contiguous(), N), "against ops.scatter_rows_det")
    for mn, want, kw in ((m, minuend.double() - ref, dict(minuend=m.contiguous())), (None, -ref, dict(negate=True))):
        out = G((B, N, C), F32, dev)
        L("ptt_scatter_rows_csr_sub_f32", dev, P(u), P(order), P(start), B, N, Ecount, C, P(mn), P(out))
        done([out], [u, order, start] + ([m] if mn is not None else []))
        assert bound(out, want), "ptt_scatter_rows_csr_sub_f32"
        eq(out, ops.scatter_rows_det(u.contiguous(), i.contiguous(), N, **kw), "against ops.scatter_rows_det(minuend / negate)")


# ------------------------------------------------------------------------------------------- spatial order and the fused launches
@pytest.mark.parametrize("N", [65, 200])
def test_spatial_order(dev, N):
    s = clouds(N)
    xyz = E(s, dev)
    out = G((B, N), I32, dev)
    L("ptt_spatial_order_f32", dev, P(xyz), B, N, P(out))
    done([out], [xyz])
    got = out.cpu()
    assert torch.equal(got.sort(dim=1)[0], torch.arange(B * N, dtype=I32).view(B, N)), "not a permutation inside every cloud"
    assert torch.equal(got[2], torch.arange(2 * N, 3 * N, dtype=I32)), "the all-zero cloud: ties by index"
    eq(out, ops.spatial_order(xyz.contiguous()), "against ops.spatial_order")


@pytest.mark.parametrize("ns", [16, 32])
@pytest.mark.parametrize("N,M,k", [(65, 7, 0), (200, 33, K), (65, 33, K)])
def test_fps_ball_knn(dev, N, M, ns, k):
    s = clouds(N)
    xyz = E(s, dev)
    inds, inds64, new_xyz, idx = G((B, M), I32, dev), G((B, M), I64, dev), G((B, M, 3), F32, dev), G((B, M, ns), I32, dev)
    knn = G((B, M, k), I32, dev) if k else None
    rel = G((B, M * k, 3), F32, dev) if k else None
    L("ptt_fps_ball_knn_f32", dev, P(xyz), B, N, M, RADIUS, ns, k, P(inds), P(inds64), P(new_xyz), P(idx), P(knn), P(rel))
    done([v for v in (inds, inds64, new_xyz, idx, knn, rel) if v is not None], [xyz])
    ref_inds = O.fps(s, M)
    centres = np.take_along_axis(s, ref_inds.astype(np.int64)[..., None], axis=1).copy()
    eq(inds, ref_inds, "ptt_fps_ball_knn_f32: samples")
    eq(inds64, ref_inds.astype(np.int64), "int64 samples")
    eq(new_xyz, centres, "centres")
    eq(idx, O.ball_query(centres, s, RADIUS, ns), "ball query")
    if k:
        eq(knn, O.knn(centres, k), "kNN of the centres")
    p = ops.fps_ball_knn(xyz.contiguous(), M, RADIUS, ns, k)
    for got, want, what in ((inds, p[0], "inds"), (inds64, p[1], "inds64"), (new_xyz, p[2], "new_xyz"), (idx, p[3], "idx")):
        eq(got, want, "against ops.fps_ball_knn (%s)" % what)
    if k:
        eq(knn, p[4][0], "against ops.fps_ball_knn (knn)")
        eq(rel, p[4][1].view(B, M * k, 3), "against ops.fps_ball_knn (rel)")


@pytest.mark.parametrize("N,npoints,nsamples,k", [(65, (7, 5, 3), (16, 16, 32), 0), (200, (33, 20, 16), (32, 16, 16), K)])
def test_point_jobs(dev, N, npoints, nsamples, k):
    """ptt_point_jobs_f32 as ops.sa_levels_point_jobs fills it: three 'sequence'-sampled levels and (k > 0) the kNN of the last
    level's centres, every output guarded; the results of ptt_centres_ball_query_f32 / ptt_knn_rel_f32 level by level."""
    s = clouds(N)
    radii = (0.3, 0.5, 0.7)
    inds0_np = O.fps(s, npoints[0])
    xyz, inds0 = E(s, dev), E(inds0_np, dev)
    n_jobs = len(npoints) + (1 if k else 0)
    arr = (_lib.PointJob * n_jobs)()
    outs, levels, n_pts = [], [], N
    inds64 = G((B, npoints[0]), I64, dev)
    outs.append(inds64)
    for l, (M, r, ns) in enumerate(zip(npoints, radii, nsamples)):
        new_xyz, idx = G((B, M, 3), F32, dev), G((B, M, ns), I32, dev)
        j = arr[l]
        j.xyz, j.centre_sel, j.point_sel = xyz.data_ptr(), inds0.data_ptr(), (inds0.data_ptr() if l > 0 else None)
        j.new_xyz, j.idx64_out, j.idx_out = new_xyz.data_ptr(), (inds64.data_ptr() if l == 0 else None), idx.data_ptr()
        j.kind, j.sel_ld, j.B, j.Nraw, j.Npts, j.M, j.nsample, j.radius = 0, npoints[0], B, N, n_pts, M, ns, float(r)
        levels.append((new_xyz, idx))
        outs += [new_xyz, idx]
        n_pts = M
    if k:
        M = npoints[-1]
        kidx, rel = G((B, M, k), I32, dev), G((B, M * k, 3), F32, dev)
        j = arr[len(npoints)]
        j.xyz, j.centre_sel, j.point_sel = xyz.data_ptr(), inds0.data_ptr(), inds0.data_ptr()
        j.idx_out, j.rel_out = kidx.data_ptr(), rel.data_ptr()
        j.kind, j.sel_ld, j.B, j.Nraw, j.Npts, j.M, j.nsample, j.radius = 1, npoints[0], B, N, M, M, k, 0.0
        outs += [kidx, rel]
    L("ptt_point_jobs_f32", dev, arr, n_jobs)
    done(outs, [xyz, inds0])
    eq(inds64, inds0_np.astype(np.int64), "level 0: the centres' raw indices")
    pts = s                                                                 # the level's own point tensor
    lvl0 = np.take_along_axis(s, inds0_np.astype(np.int64)[..., None], axis=1)
    for l, (M, r, ns) in enumerate(zip(npoints, radii, nsamples)):
        centres = lvl0[:, :M].copy()
        eq(levels[l][0], centres, "level %d: centres" % l)
        eq(levels[l][1], O.ball_query(centres, np.ascontiguousarray(pts), r, ns), "level %d: ball query" % l)
        pts = centres
    if k:
        eq(kidx, O.knn(np.ascontiguousarray(pts), k), "kNN of the last level's centres")
    p_levels, p_64, p_knn = ops.sa_levels_point_jobs(xyz.contiguous(), inds0.contiguous(), list(npoints), list(radii), list(nsamples), knn_k=k)
    eq(inds64, p_64, "against ops.sa_levels_point_jobs (inds64)")
    for l in range(len(npoints)):
        eq(levels[l][0], p_levels[l][0], "against ops.sa_levels_point_jobs (level %d centres)" % l)
        eq(levels[l][1], p_levels[l][1], "against ops.sa_levels_point_jobs (level %d idx)" % l)
    if k:
        eq(kidx, p_knn[0], "against ops.sa_levels_point_jobs (knn)")
        eq(rel, p_knn[1].view(B, -1, 3), "against ops.sa_levels_point_jobs (rel)")
