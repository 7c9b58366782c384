"""ptt_crop_scan_f32 (every crop job spread over chunks of its cloud, two launches) against ptt_crop_compact_f32 (one workgroup
per job) on the SAME job tables: the same survivors in the same order with the same float32 bits and the same count, outputs and
workspace behind guard bands, a second launch byte-identical; one case directly against the oracle's crop_center_pc."""
import numpy as np
import pytest
import torch

from oracle import tracking_ref as TR
from ptt_amd import ops
from tests import guard

pytestmark = pytest.mark.gpu
C = ops.SCAN_CROP_CHUNK

KEEP_ALL = dict(center=(0.0, 0.0, 0.0), wlh=(40.0, 40.0, 8.0), yaw=0.0)
KEEP_NONE = dict(center=(100.0, 100.0, 0.0), wlh=(2.0, 4.0, 2.0), yaw=0.0)
KEEP_30 = dict(center=(0.0, 0.0, 0.0), wlh=(8.0, 9.6, 8.0), yaw=0.0)        # 1.25 * (9.6 x 8) = 12 x 10 of the 20 x 20 cloud
YAWED = dict(center=(1.0, -2.0, 0.1), wlh=(3.0, 9.0, 3.0), yaw=0.7)


def _cloud(seed, n):
    rs = np.random.RandomState(seed)
    return (rs.uniform(-1, 1, (3, n)) * np.array([[10.0], [10.0], [1.0]])).astype(np.float32)


def _quat(yaw):
    return np.array([np.cos(yaw / 2), 0.0, 0.0, np.sin(yaw / 2)])


def _spec(points, box, n_points=None, ld=None, capacity=None, extra=0.0):
    n = points.shape[1] if n_points is None else n_points
    return dict(points=points, n=n, ld=ld, capacity=max(1, n) if capacity is None else capacity, box=box, extra=extra)


def _table(dev, specs):
    """-> (host job table with bounds and cloud fields, the device clouds). `out` / `count` are left for the caller."""
    boxes = np.zeros(len(specs), ops.TRACK_BOX)
    jobs = np.zeros(len(specs), ops.CROP_JOB)
    clouds = []
    for k, s in enumerate(specs):
        boxes['center'][k], boxes['wlh'][k], boxes['quat'][k] = s['box']['center'], s['box']['wlh'], _quat(s['box']['yaw'])
        pts = s['points'] if s['points'].shape[1] else np.zeros((3, 1), np.float32)      # an empty job still carries an address
        t = guard.embed(torch.from_numpy(np.ascontiguousarray(pts)).to(dev), ld=s['ld'])
        clouds.append(t)
        jobs['points'][k], jobs['ld'][k], jobs['n_points'][k], jobs['capacity'][k] = t.data_ptr(), t.stride(0), s['n'], s['capacity']
    ops.track_crop_bounds(boxes, 0.0, 1.25, np.array([s['extra'] for s in specs]), jobs)
    return jobs, clouds


def _run(dev, specs, max_points=None):
    """Both kernels on the same table -> per job (count, rows (min(count, capacity), 3)) of the chunked kernel, after every check
    of the module's docstring."""
    jobs, clouds = _table(dev, specs)
    n_jobs = len(specs)
    max_points = max(s['n'] for s in specs) if max_points is None else max_points
    # the reference: ptt_crop_compact_f32 into plain buffers
    ref_out = [torch.full((s['capacity'], 3), float('nan'), dtype=torch.float32, device=dev) for s in specs]
    ref_cnt = torch.full((n_jobs,), -7, dtype=torch.int32, device=dev)
    jobs['out'] = [t.data_ptr() for t in ref_out]
    jobs['count'] = ref_cnt.data_ptr() + 4 * np.arange(n_jobs)
    ops.crop_compact(ops.upload_jobs(jobs), n_jobs)
    # the chunked kernel: outputs, counts and workspace inside guard bands
    outs = [guard.guarded((s['capacity'], 3), torch.float32, device=dev) for s in specs]
    cnts = [guard.guarded((1,), torch.int32, device=dev) for _ in specs]
    nbytes = ops.crop_scan_workspace(n_jobs, max_points)
    assert nbytes == 4 * n_jobs * max(1, -(-max_points // C))
    ws = guard.workspace(nbytes, device=dev)
    jobs['out'] = [t.data_ptr() for t in outs]
    jobs['count'] = [t.data_ptr() for t in cnts]
    ops.crop_scan_check(jobs, n_jobs, max_points)
    table = ops.upload_jobs(jobs)
    args = (guard.ptr(table), n_jobs, max_points, guard.ptr(ws), nbytes)
    guard.launch("ptt_crop_scan_f32", dev, *args)
    torch.cuda.synchronize()
    first = [t._guard.words.clone() for t in outs + cnts]
    guard.launch("ptt_crop_scan_f32", dev, *args)
    torch.cuda.synchronize()
    for before, t in zip(first, outs + cnts):
        assert torch.equal(before, t._guard.words), "a second launch wrote different bytes"
    guard.check_guard(ws, all_written=True)
    res = []
    want_cnt = ref_cnt.cpu().numpy()
    for k, s in enumerate(specs):
        guard.check_guard(cnts[k], all_written=True)
        guard.check_guard(outs[k], all_written=False)
        count = int(cnts[k].item())
        assert count == int(want_cnt[k]), "job %d" % k
        m = min(count, s['capacity'])
        rows = outs[k][:m].cpu().numpy()
        np.testing.assert_array_equal(rows, ref_out[k][:m].cpu().numpy(), err_msg="job %d" % k)
        assert not np.isnan(rows).any()
        assert bool((outs[k].view(torch.int32)[m:] == guard.SENTINEL).all()), "job %d: a row from min(count, capacity) on was written" % k
        res.append((count, rows))
    del clouds
    return res


@pytest.mark.parametrize("n", [0, 1, 2, C - 1, C, C + 1, 3 * C + 17])
def test_sizes_around_the_chunk_keep_all_none_and_a_third(dev, n):
    pts = _cloud(n, n)
    (all_, _), (none, _), (third, _) = _run(dev, [_spec(pts, KEEP_ALL), _spec(pts, KEEP_NONE), _spec(pts, KEEP_30)])
    assert all_ == n and none == 0
    if n > 1000:
        assert 0.2 * n < third < 0.4 * n


def test_yawed_box_second_crop_removes_points_and_equals_the_oracle(dev):
    n = 3 * C + 17
    pts = _cloud(5, n)
    jobs, _ = _table(dev, [_spec(pts, YAWED, extra=0.3)])
    lo, hi = jobs['lo1'][0], jobs['hi1'][0]
    first = int(np.all((pts.T.astype(np.float64) > lo) & (pts.T.astype(np.float64) < hi), axis=1).sum())
    (count, rows), = _run(dev, [_spec(pts, YAWED, extra=0.3)])
    assert 0 < count < first                                   # the second crop removed points the first one kept
    box = TR.RefBox(YAWED['center'], YAWED['wlh'], _quat(YAWED['yaw']))
    want = TR.crop_center_pc(pts, box, gt_wlh1=0.5, offset=0.0, scale=1.25)               # extra = gt_wlh1 * 0.6 = 0.3
    assert want.dtype == np.float32 and want.shape[1] == count
    np.testing.assert_array_equal(rows, want.T)


def test_survivors_only_in_the_last_chunk(dev):
    n = 3 * C + 17
    pts = _cloud(6, n)
    pts[0, :3 * C] += 100.0
    (count, rows), = _run(dev, [_spec(pts, KEEP_ALL)])
    assert count == 17
    np.testing.assert_array_equal(rows, pts[:, 3 * C:].T)      # a box at the origin without yaw: the points themselves


def test_capacity_below_the_survivor_count_reports_the_full_count(dev):
    n = 2 * C + 300
    pts = _cloud(7, n)
    # the capacity ends inside chunk 1, on the boundary of chunk 1, and at a single row
    res = _run(dev, [_spec(pts, KEEP_ALL, capacity=C + 77), _spec(pts, KEEP_ALL, capacity=C), _spec(pts, KEEP_30, capacity=1)])
    assert [c for c, _ in res[:2]] == [n, n] and res[2][0] > 1
    assert [len(r) for _, r in res] == [C + 77, C, 1]


def test_leading_dimension_larger_than_the_cloud_and_max_points_larger_than_every_cloud(dev):
    n = C + 9
    pts = _cloud(8, n + 40)
    # n_points below the row length: the columns from n_points on lie inside the box and must not be looked at
    res = _run(dev, [_spec(pts, KEEP_ALL, n_points=n, ld=n + 40 + 13)], max_points=4 * C + 5)
    assert res[0][0] == n


@pytest.mark.parametrize("n_jobs", [1, 2, 13])
def test_several_jobs_in_one_launch(dev, n_jobs):
    sizes = [3 * C + 17, 0, C, 5, 2 * C - 1, C + 1, 0, 2 * C, 700, 1, C - 1, 2, 4 * C + 3][:n_jobs]
    boxes = [KEEP_30, KEEP_ALL, YAWED, KEEP_NONE]
    specs = []
    for k, n in enumerate(sizes):
        pts = _cloud(100 + k, n)
        capacity = [None, max(1, n // 3), n + 5][k % 3]
        specs.append(_spec(pts, boxes[k % 4], ld=None if k % 2 else n + 3 + k, capacity=capacity, extra=0.1 * (k % 3)))
    res = _run(dev, specs, max_points=max(sizes) + (C + 1 if n_jobs == 13 else 0))
    for (count, _), n in zip(res, sizes):
        assert 0 <= count <= n
    if n_jobs == 13:
        assert res[1][0] == 0 and res[6][0] == 0 and res[5][0] == C + 1          # the empty jobs; a keep-all job


def test_wrapper_uploads_launches_and_refuses_what_the_kernel_cannot_report(dev):
    n = 2 * C + 5
    pts = _cloud(9, n)
    jobs, clouds = _table(dev, [_spec(pts, KEEP_30), _spec(pts, YAWED)])
    out = torch.zeros((2, 2, n, 3), dtype=torch.float32, device=dev)
    cnt = torch.zeros((2, 2), dtype=torch.int32, device=dev)
    jobs['out'], jobs['count'] = [out[0, 0].data_ptr(), out[0, 1].data_ptr()], [cnt[0, 0:].data_ptr(), cnt[0, 1:].data_ptr()]
    ops.crop_compact(ops.upload_jobs(jobs), 2)
    jobs['out'], jobs['count'] = [out[1, 0].data_ptr(), out[1, 1].data_ptr()], [cnt[1, 0:].data_ptr(), cnt[1, 1:].data_ptr()]
    table = torch.zeros(jobs.nbytes, dtype=torch.uint8, device=dev)
    assert ops.crop_scan(jobs, 2, n, dev, out=table) is table
    torch.cuda.synchronize()
    assert torch.equal(cnt[0], cnt[1]) and int(cnt[0].min()) > 0
    assert torch.equal(out[0], out[1])
    before = (out.clone(), cnt.clone())
    bad = jobs.copy()
    bad['label_out'][1] = out.data_ptr()
    with pytest.raises(ValueError, match="label_out"):
        ops.crop_scan(bad, 2, n, dev)
    bad = jobs.copy()
    bad['append'][0] = 1
    with pytest.raises(ValueError, match="append"):
        ops.crop_scan(bad, 2, n, dev)
    with pytest.raises(ValueError, match="max_points"):
        ops.crop_scan(jobs, 2, n - 1, dev)
    torch.cuda.synchronize()
    assert torch.equal(before[0], out) and torch.equal(before[1], cnt)             # a refused table launches nothing
