"""The crop / resample / select kernels of ptt_amd/csrc/track_ops.hip on the C ABI, behind guard bands (tests/guard.py):
ptt_crop_compact_f32, ptt_crop_compact_host_f32, ptt_regularize_f32, ptt_crop_regularize_f32 and ptt_select_box_f32.

The method of tests/test_train_rows_guard_gpu.py: every launch goes through guard.launch, every output lies in a guarded(...)
buffer of exactly its size — the (capacity, 3) rows, the 1-word count, the 2-word info, the labels (capacity bytes, a guarded
int32 buffer of capacity / 4 words viewed as bytes) — every cloud, segment, count and draw table is embed(...)-ded, check_guard
runs after each launch, a second launch gives the same bits (for append jobs after the store and its count were put back), and
the guarded result equals what the ops.* wrapper gives. Job tables are built as tests/test_scan_crop_gpu.py builds them.

The references are bit-exact, so no tolerance appears: oracle.tracking_ref.crop_center_pc / crop_center_pc_labels /
regularize_pc (tests/golden/GOLDEN_REPORT.txt records them as bitwise equal to the reference) and np.argmax. The number of
generator outputs a resampling consumes is computed on the host from numpy's own generator — masked rejection over the raw 32-bit
outputs of RandomState(1) — never read back from the kernel.

select_box. np.argmax returns the first NaN of a row, and so does ptt_track_select_update, the host-side selection a small batch
takes; select_box_kernel used to skip NaN scores and return the largest finite one. The rows holding NaN are held to both."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import tracking_ref as TR
from ptt_amd import _lib, ops
from tests import guard
from tests.guard import check_guard, embed, guarded
from tests.test_scan_crop_gpu import KEEP_30, KEEP_ALL, KEEP_NONE, YAWED, _cloud, _quat, _spec, _table

pytestmark = pytest.mark.gpu
L, P = guard.launch, guard.ptr
F32, I32 = torch.float32, torch.int32
T = 1024                                   # points per round of crop_compact_body
MAXV = ops.CROP_JOBS_BY_VALUE_MAX
GT_WLH1 = 0.5                              # the `extra` of a search crop is gt_box.wlh[1] * 0.6
SENTINEL_BYTES = (0xef, 0xbe, 0xc0, 0x7f)  # guard.SENTINEL, little-endian


def words(t):
    return t._guard.words


def same_bits(a, b, what):
    a, b = a.contiguous().view(I32).reshape(-1), b.to(a.device).contiguous().view(I32).reshape(-1)
    assert a.numel() == b.numel() and torch.equal(a, b), "%s: not the same bits" % what


def ref_box(box):
    return TR.RefBox(box['center'], box['wlh'], _quat(box['yaw']))


# ============================================================================================================ crop_compact
def spec(points, box, extra=False, gt=None, start=None, **kw):
    """_spec of tests/test_scan_crop_gpu.py plus: extra — the second crop grown by GT_WLH1 * 0.6; gt — a ground-truth box: labels
    are written and the second crop grows by gt.wlh[1] * 0.6; start — an append job whose store holds `start` rows."""
    s = _spec(points, box, extra=(gt['wlh'][1] * 0.6 if gt is not None else (GT_WLH1 * 0.6 if extra else 0.0)), **kw)
    s.update(gt=gt, start=start, grown=extra)
    return s


def expected(s):
    """-> (rows (count, 3) float32, labels (count,) bool or None) of the oracle."""
    pts = np.ascontiguousarray(s['points'][:, :s['n']])
    if s['gt'] is not None:
        rows, lab = TR.crop_center_pc_labels(pts, ref_box(s['box']), ref_box(s['gt']), offset=0.0, scale=1.25)
        return np.ascontiguousarray(rows.T), lab
    rows = TR.crop_center_pc(pts, ref_box(s['box']), gt_wlh1=GT_WLH1 if s['grown'] else None, offset=0.0, scale=1.25)
    assert rows.dtype == np.float32
    return np.ascontiguousarray(rows.T), None


def prefill_rows(k):
    return (torch.arange(k * 3, dtype=F32).reshape(k, 3) + 0.5) * -1.0


class Crop(object):
    """A job table over guarded outputs. launch(mode) runs it through the C ABI: 'device' (an uploaded table), 'host' (by value),
    'pinned' (ptt_crop_compact_f32 reading pinned host memory)."""

    def __init__(self, dev, specs):
        self.dev, self.specs = dev, specs
        self.jobs, self.clouds = _table(dev, specs)
        self.outs = [guarded((s['capacity'], 3), F32, device=dev) for s in specs]
        self.cnts = [guarded((1,), I32, device=dev) for _ in specs]
        self.labs = [None] * len(specs)
        self.jobs['out'] = [t.data_ptr() for t in self.outs]
        self.jobs['count'] = [t.data_ptr() for t in self.cnts]
        for k, s in enumerate(specs):
            if s['gt'] is not None:
                assert s['capacity'] % 4 == 0
                gt = np.zeros(1, ops.TRACK_BOX)
                gt['center'][0], gt['wlh'][0], gt['quat'][0] = s['gt']['center'], s['gt']['wlh'], _quat(s['gt']['yaw'])
                tmp = np.zeros(1, ops.CROP_JOB)
                ops.track_crop_bounds(gt, 0.0, 1.25, None, tmp)              # get_label_by_box(pts, gt_box, offset, scale)
                for dst, src in (('ltrans', 'trans'), ('lrot', 'rot'), ('llo', 'lo2'), ('lhi', 'hi2')):
                    self.jobs[dst][k] = tmp[src][0]
                self.labs[k] = guarded((s['capacity'] // 4,), I32, device=dev)
                self.jobs['label_out'][k] = self.labs[k].data_ptr()
            if s['start'] is not None:
                self.jobs['append'][k] = 1
                held = min(s['start'], s['capacity'])
                if held:
                    self.outs[k][:held] = prefill_rows(held).to(dev)
                self.cnts[k][0] = s['start']
        self.state = self.outs + self.cnts + [t for t in self.labs if t is not None]
        self.before = [words(t).clone() for t in self.state]
        self.keep = None

    def restore(self):
        for t, w in zip(self.state, self.before):
            words(t).copy_(w)

    def launch(self, mode="device", n_jobs=None):
        n = len(self.specs) if n_jobs is None else n_jobs
        if mode == "device":
            self.keep = ops.upload_jobs(self.jobs)
            L("ptt_crop_compact_f32", self.dev, P(self.keep), n)
        elif mode == "host":
            L("ptt_crop_compact_host_f32", self.dev, ctypes.c_void_p(self.jobs.ctypes.data), n)
        else:
            self.keep = torch.from_numpy(self.jobs.view(np.uint8).reshape(-1).copy()).pin_memory()
            L("ptt_crop_compact_f32", self.dev, ctypes.c_void_p(self.keep.data_ptr()), n)
        torch.cuda.synchronize()

    def snapshot(self):
        return [words(t).clone() for t in self.state]

    def check(self, times=1):
        """Guards, counts, rows and labels of every job against the oracle, after `times` launches without a restore in between
        (more than one: append jobs only). -> the counts of one crop."""
        counts = []
        for k, s in enumerate(self.specs):
            what = "job %d" % k
            out, cnt, lab = self.outs[k], self.cnts[k], self.labs[k]
            check_guard(cnt)
            check_guard(out, all_written=False)
            for cloud in self.clouds:
                check_guard(cloud, all_written=False)
            rows, labels = expected(s)
            c, cap = rows.shape[0], s['capacity']
            counts.append(c)
            start = 0 if s['start'] is None else s['start']
            assert times == 1 or s['start'] is not None
            assert int(cnt.item()) == start + times * c, what
            got = out.cpu()
            held = min(start, cap)
            if held:
                same_bits(got[:held], prefill_rows(held), what + ": the rows the store held")
            at = start
            for _ in range(times):
                m = max(0, min(at + c, cap) - at)
                if m:
                    same_bits(got[at:at + m], torch.from_numpy(rows[:m]), what + ": rows against the oracle")
                at += c
            end = min(start + times * c, cap)
            assert bool((got[end:].view(I32) == guard.SENTINEL).all()), what + ": a row from min(count, capacity) on was written"
            if lab is not None:
                check_guard(lab, all_written=False)
                b = lab.cpu().view(torch.uint8)
                m = min(c, cap)
                assert torch.equal(b[:m], torch.from_numpy(labels[:m].astype(np.uint8))), what + ": labels against the oracle"
                pattern = torch.tensor(SENTINEL_BYTES * (cap // 4), dtype=torch.uint8)
                assert torch.equal(b[m:], pattern[m:]), what + ": a label from min(count, capacity) on was written"
        return counts

    def wrapper(self):
        """The same table through ops.crop_compact into plain copies of the outputs' starting state -> those copies."""
        now = self.snapshot()
        self.restore()
        plain = [t.clone() for t in self.state]
        for t, w in zip(self.state, now):
            words(t).copy_(w)
        jobs = self.jobs.copy()
        n = len(self.specs)
        jobs['out'] = [t.data_ptr() for t in plain[:n]]
        jobs['count'] = [t.data_ptr() for t in plain[n:2 * n]]
        rest = iter(plain[2 * n:])
        for k, lab in enumerate(self.labs):
            if lab is not None:
                jobs['label_out'][k] = next(rest).data_ptr()
        ops.crop_compact(ops.upload_jobs(jobs), n)
        torch.cuda.synchronize()
        return plain


def run_crop(dev, specs, mode="device"):
    """Launch, check against the oracle, launch again from the same starting state (same bits), compare with ops.crop_compact.
    -> (the Crop, the counts, the word buffers of every output after the launch)."""
    c = Crop(dev, specs)
    c.launch(mode)
    counts = c.check()
    first = c.snapshot()
    c.restore()
    c.launch(mode)
    for a, b in zip(first, c.snapshot()):
        assert torch.equal(a, b), "a second launch wrote different bits"
    for t, p in zip(c.state, c.wrapper()):
        same_bits(p, t, "against ops.crop_compact")
    return c, counts, first


@pytest.mark.parametrize("n", [0, 1, 2, T - 1, T, T + 1, 3 * T + 17])
def test_crop_compact_sizes_around_the_round(dev, n):
    pts = _cloud(n, n)
    _, (all_, none, third, yawed), _ = run_crop(dev, [spec(pts, KEEP_ALL), spec(pts, KEEP_NONE), spec(pts, KEEP_30), spec(pts, YAWED, extra=True)])
    assert all_ == n and none == 0
    if n > 1000:
        assert 0.2 * n < third < 0.4 * n and 0 < yawed < third


def test_crop_compact_leading_dimension_larger_than_the_cloud(dev):
    n = T + 9
    pts = _cloud(8, n + 40)                 # the columns from n_points on lie inside the box and must not be looked at
    _, counts, _ = run_crop(dev, [spec(pts, KEEP_ALL, n_points=n, ld=n + 40 + 13), spec(pts, KEEP_ALL, n_points=1, ld=n + 41)])
    assert counts == [n, 1]


def test_crop_compact_capacity_below_the_count(dev):
    n = 2 * T + 300
    pts = _cloud(7, n)
    c, counts, _ = run_crop(dev, [spec(pts, KEEP_ALL, capacity=T + 77), spec(pts, KEEP_ALL, capacity=T), spec(pts, KEEP_30, capacity=1)])
    assert counts[:2] == [n, n] and counts[2] > 1
    assert [int(t.item()) for t in c.cnts] == counts             # *count still reports the full number


GT = dict(center=(1.5, -1.5, 0.0), wlh=(2.0, 4.0, 2.0), yaw=0.5)


def test_crop_compact_labels(dev):
    n = 2 * T + 100
    pts = _cloud(11, n)
    c, counts, _ = run_crop(dev, [spec(pts, YAWED, gt=GT, capacity=n), spec(pts, YAWED, gt=GT, capacity=64), spec(pts, KEEP_NONE, gt=GT, capacity=4)])
    labels = expected(c.specs[0])[1]
    assert counts[0] == counts[1] > 64 and 0 < int(labels.sum()) < counts[0] and 0 < int(labels[:64].sum()) < 64
    assert counts[2] == 0


def test_crop_compact_append(dev):
    n = T + 476
    pts = _cloud(12, n)
    cnt = expected(spec(pts, KEEP_30))[0].shape[0]
    assert cnt > 100
    cap = cnt + 50
    specs = [spec(pts, KEEP_30, start=0, capacity=cap), spec(pts, KEEP_30, start=37, capacity=cap), spec(pts, KEEP_30, start=cap - 3, capacity=cap),
             spec(pts, KEEP_30, start=cap, capacity=cap), spec(pts, KEEP_30, start=cap + 5, capacity=cap), spec(pts, KEEP_NONE, start=9, capacity=cap),
             spec(pts, KEEP_30, capacity=cap)]
    c, counts, _ = run_crop(dev, specs)
    assert counts == [cnt] * 5 + [0, cnt]
    assert [int(t.item()) for t in c.cnts] == [cnt, 37 + cnt, cap - 3 + cnt, cap + cnt, cap + 5 + cnt, 9, cnt]


def test_crop_compact_the_same_job_twice_appends_twice(dev):
    n = T + 476
    pts = _cloud(12, n)
    cnt = expected(spec(pts, KEEP_30))[0].shape[0]
    c = Crop(dev, [spec(pts, KEEP_30, start=5, capacity=2 * cnt + 50), spec(pts, KEEP_30, start=0, capacity=cnt + cnt // 2)])
    c.launch()
    c.check()
    c.launch()
    c.check(times=2)
    assert [int(t.item()) for t in c.cnts] == [5 + 2 * cnt, 2 * cnt]


def mixed_specs(n_jobs):
    sizes = [3 * T + 17, 0, T, 5, 2 * T - 1, T + 1, 0, 2 * T, 700, 1, T - 1, 2, 4 * T + 3][:n_jobs]
    boxes = [KEEP_30, KEEP_ALL, YAWED, KEEP_NONE]
    specs = []
    for k, n in enumerate(sizes):
        capacity = [None, max(1, n // 3), n + 5][k % 3]
        specs.append(spec(_cloud(100 + k, n), boxes[k % 4], extra=bool(k % 3), ld=None if k % 2 else n + 3 + k, capacity=capacity))
    return specs, sizes


def test_crop_compact_thirteen_jobs_in_one_launch(dev):
    specs, sizes = mixed_specs(13)
    _, counts, _ = run_crop(dev, specs)
    assert counts[1] == 0 and counts[6] == 0 and counts[5] == T + 1          # the empty jobs; a keep-all job
    assert all(0 <= c <= n for c, n in zip(counts, sizes))


@pytest.mark.parametrize("mode,n_jobs", [("host", 1), ("host", MAXV), ("pinned", MAXV)])
def test_crop_compact_table_by_value_and_in_pinned_memory(dev, mode, n_jobs):
    specs, _ = mixed_specs(n_jobs)
    if n_jobs > 1:
        specs[2] = spec(_cloud(55, 900), YAWED, gt=GT, capacity=400)
        specs[4] = spec(specs[4]['points'], KEEP_30, start=7, capacity=specs[4]['n'])
    _, _, by_device = run_crop(dev, specs)
    c = Crop(dev, specs)
    c.launch(mode)
    c.check()
    for a, b in zip(by_device, c.snapshot()):
        assert torch.equal(a, b), "%s table against the device table" % mode
    if mode == "host":                                       # ops.crop_compact_host on plain outputs
        c.restore()
        plain = [t.clone() for t in c.state]
        jobs = c.jobs.copy()
        jobs['out'], jobs['count'] = [t.data_ptr() for t in plain[:n_jobs]], [t.data_ptr() for t in plain[n_jobs:2 * n_jobs]]
        rest = iter(plain[2 * n_jobs:])
        for k, lab in enumerate(c.labs):
            if lab is not None:
                jobs['label_out'][k] = next(rest).data_ptr()
        ops.crop_compact_host(jobs, n_jobs, dev)
        torch.cuda.synchronize()
        c.launch(mode)
        for t, p in zip(c.state, plain):
            same_bits(p, t, "against ops.crop_compact_host")


def test_crop_compact_refusals(dev):
    """PTT_EINVAL ("bad size" in the header's list of statuses): more jobs by value than PTT_CROP_JOBS_BY_VALUE_MAX, a negative
    n_jobs. The table is a valid one of MAX + 1 jobs: were the launch not refused, it would run inside its buffers."""
    specs, _ = mixed_specs(MAXV + 1)
    c = Crop(dev, specs)
    for mode, n in (("host", MAXV + 1), ("host", -1), ("device", -1), ("pinned", -2)):
        with pytest.raises(RuntimeError, match="PTT_EINVAL"):
            c.launch(mode, n_jobs=n)
    torch.cuda.synchronize()
    guard.assert_untouched(*c.state)


# ============================================================================================================== regularize
N_TABLE = 8192


def raw_outputs():
    """The first N_TABLE raw 32-bit outputs of numpy's MT19937 after seed(1)."""
    return np.random.RandomState(1).randint(0, 2 ** 32, size=N_TABLE, dtype=np.uint64).astype(np.uint32)


def draws_consumed(n, size, n_draws=N_TABLE):
    """np.random.randint(0, n, size) after seed(1): masked rejection over the raw outputs -> (outputs consumed, or None when
    n_draws outputs do not yield `size` indices; the number of indices the first n_draws outputs yield, capped at size)."""
    raw = raw_outputs()[:n_draws]
    mask = 0
    while mask < n - 1:
        mask = (mask << 1) | 1
    ok = np.flatnonzero((raw & np.uint32(mask)) <= n - 1)
    if len(ok) >= size:
        return int(ok[size - 1]) + 1, size
    return None, len(ok)


def test_numpy_consumes_what_draws_consumed_says():
    raw = raw_outputs()
    rs = np.random.RandomState(1)
    assert np.array_equal(rs.randint(0, 2 ** 32, size=16, dtype=np.uint64).astype(np.uint32), raw[:16])
    for n, size in ((3, 64), (33, 64), (1025, 300), (64, 300)):
        used, _ = draws_consumed(n, size)
        np.random.seed(1)
        idx = np.random.randint(low=0, high=n, size=size, dtype=np.int64)
        follow = np.random.randint(0, 2 ** 32, size=1, dtype=np.uint64)          # the generator's next raw output
        assert int(follow[0]) == int(raw[used]), (n, size)
        mask = (1 << int(n - 1).bit_length()) - 1
        acc = raw[:used] & np.uint32(mask)
        assert np.array_equal(acc[acc <= n - 1].astype(np.int64), idx)


class Seg(object):
    """One segment: `rows` valid rows inside a (capacity, 3) buffer whose other rows are NaN, and its device count (which may
    exceed the capacity: the kernel then takes `capacity` rows)."""

    def __init__(self, dev, g, count, capacity=None):
        self.capacity = max(1, count) if capacity is None else capacity
        self.count = count
        self.valid = min(count, self.capacity)
        buf = torch.full((self.capacity, 3), float("nan"), dtype=F32)
        buf[:self.valid] = torch.randn(self.valid, 3, generator=g, dtype=F32)
        self.rows = buf[:self.valid].numpy().copy()
        self.dev_rows = embed(buf.to(dev))
        self.dev_count = embed(torch.tensor([count], dtype=I32).to(dev))


def reg_table(dev, jobs_segs, size, with_info):
    """-> (host job table, outs, infos) for jobs given as lists of Seg."""
    jobs = np.zeros(len(jobs_segs), ops.REGULARIZE_JOB)
    outs = [guarded((size, 3), F32, device=dev) for _ in jobs_segs]
    infos = [guarded((2,), I32, device=dev) if w else None for w in with_info]
    for k, segs in enumerate(jobs_segs):
        assert 1 <= len(segs) <= _lib.PTT_MAX_SEGMENTS
        for s, seg in enumerate(segs):
            jobs['seg'][k][s], jobs['seg_count'][k][s], jobs['seg_capacity'][k][s] = seg.dev_rows.data_ptr(), seg.dev_count.data_ptr(), seg.capacity
        jobs['out'][k], jobs['n_seg'][k], jobs['input_size'][k] = outs[k].data_ptr(), len(segs), size
        jobs['info'][k] = infos[k].data_ptr() if infos[k] is not None else 0
    return jobs, outs, infos


def reg_expected(segs, size):
    cloud = np.concatenate([s.rows for s in segs], axis=0) if segs else np.zeros((0, 3), np.float32)
    return cloud.shape[0], np.ascontiguousarray(TR.regularize_pc(np.ascontiguousarray(cloud.T), size))


def reg_launch(dev, jobs, draws):
    table = ops.upload_jobs(jobs)
    L("ptt_regularize_f32", dev, P(table), len(jobs), P(draws), draws.numel())
    torch.cuda.synchronize()
    return table


def draw_table(dev, n_draws):
    host = torch.from_numpy(raw_outputs().view(np.int32)[:n_draws].copy())
    assert torch.equal(ops.mt19937_draws(dev, N_TABLE).cpu()[:n_draws], host)             # ptt_mt19937_fill against numpy
    return embed(host.to(dev))


def reg_check(dev, jobs_segs, outs, infos, size, n_draws, what):
    for k, segs in enumerate(jobs_segs):
        tag = "%s, job %d" % (what, k)
        n, rows = reg_expected(segs, size)
        check_guard(outs[k])
        for s in segs:
            check_guard(s.dev_rows, all_written=False)
            check_guard(s.dev_count, all_written=False)
        used, filled = (0, size) if n <= 2 or n == size else draws_consumed(n, size, n_draws)
        got = outs[k].cpu()
        same_bits(got[:filled], torch.from_numpy(rows[:filled]), tag + ": rows against regularize_pc")
        if filled < size:
            assert bool(torch.isnan(got[filled:]).all()), tag + ": the rows from the shortfall on are NaN"
        if infos[k] is not None:
            check_guard(infos[k])
            assert infos[k].cpu().tolist() == [n, -1 if used is None else used], tag + ": info"


@pytest.mark.parametrize("size", [64, 300])
def test_regularize_sizes_and_segments(dev, size):
    g = torch.Generator().manual_seed(size)
    S = lambda count, capacity=None: Seg(dev, g, count, capacity)
    jobs_segs = [
        [S(0)],                                             # n = 0, 1, 2: an all-zero cloud
        [S(0), S(1)],                                       # an empty first segment
        [S(1), S(0), S(1)],                                 # an empty middle segment
        [S(0), S(1), S(0), S(2)],                           # n = 3, PTT_MAX_SEGMENTS segments
        [S(size - 1)],
        [S(10), S(0), S(size - 30), S(20)],                 # n = size: copied through in order across the segment borders
        [S(size // 2), S(size + 1 - size // 2)],
        [S(0), S(32)],
        [S(40, capacity=20), S(13)],                        # n = 33: *seg_count above seg_capacity counts as seg_capacity
        [S(1000), S(0), S(25)],                             # n = 1025
        [S(50)],                                            # info NULL
        [S(5, capacity=9), S(size - 5, capacity=size)],     # n = size with capacities above the counts
    ]
    with_info = [True] * 10 + [False, True]
    assert [reg_expected(s, size)[0] for s in jobs_segs] == [0, 1, 2, 3, size - 1, size, size + 1, 32, 33, 1025, 50, size]
    n_draws = 1001                                          # no multiple of the 256 threads
    assert all(draws_consumed(n, size, n_draws)[0] is not None for n in (3, size - 1, size + 1, 32, 33, 1025, 50))
    draws = draw_table(dev, n_draws)
    jobs, outs, infos = reg_table(dev, jobs_segs, size, with_info)
    reg_launch(dev, jobs, draws)
    reg_check(dev, jobs_segs, outs, infos, size, n_draws, "size %d" % size)
    check_guard(draws, all_written=False)
    first = [words(t).clone() for t in outs + [i for i in infos if i is not None]]
    reg_launch(dev, jobs, draws)
    for a, t in zip(first, outs + [i for i in infos if i is not None]):
        assert torch.equal(a, words(t)), "a second launch wrote different bits"
    # ops.regularize into plain buffers
    plain_out = [torch.full((size, 3), float("nan"), dtype=F32, device=dev) for _ in jobs_segs]
    plain_info = torch.full((len(jobs_segs), 2), -7, dtype=I32, device=dev)
    pj = jobs.copy()
    pj['out'] = [t.data_ptr() for t in plain_out]
    pj['info'] = [plain_info[k].data_ptr() if with_info[k] else 0 for k in range(len(jobs_segs))]
    ops.regularize(ops.upload_jobs(pj), len(pj), draws.contiguous())
    torch.cuda.synchronize()
    for k in range(len(jobs_segs)):
        same_bits(outs[k], plain_out[k], "job %d against ops.regularize" % k)
        if with_info[k]:
            same_bits(infos[k], plain_info[k], "job %d against ops.regularize (info)" % k)


@pytest.mark.parametrize("size,n", [(64, 33), (64, 1025), (300, 33), (300, 299)])
def test_regularize_draw_table_exactly_long_enough_and_too_short(dev, size, n):
    g = torch.Generator().manual_seed(size + n)
    used, _ = draws_consumed(n, size)
    for n_draws in (used, used - 1, used // 2):
        segs = [[Seg(dev, g, n - n // 3), Seg(dev, g, n // 3)], [Seg(dev, g, 1)]]       # the second job draws nothing: info (1, 0)
        draws = draw_table(dev, n_draws)
        jobs, outs, infos = reg_table(dev, segs, size, [True, True])
        reg_launch(dev, jobs, draws)
        got_used, filled = draws_consumed(n, size, n_draws)
        assert (got_used == used and filled == size) if n_draws == used else (got_used is None and filled < size)
        if n_draws == used - 1:
            assert filled == size - 1
        reg_check(dev, segs, outs, infos, size, n_draws, "size %d, n %d, %d draws" % (size, n, n_draws))
        check_guard(draws, all_written=False)


# ========================================================================================================= crop_regularize
def test_crop_regularize_equals_crop_compact_then_regularize(dev):
    size = 64
    g = torch.Generator().manual_seed(5)
    pts = _cloud(21, T + 476)
    specs = [spec(pts, KEEP_30, extra=True), spec(pts, YAWED), spec(_cloud(22, 1100), KEEP_ALL, capacity=500), spec(pts, KEEP_NONE, capacity=8)]
    # an earlier launch's crop: the first segment of the template job (job 1)
    earlier = Crop(dev, [spec(_cloud(23, 700), KEEP_30)])
    earlier.launch()
    n_first = earlier.check()[0]
    assert n_first > 2
    first_rows = earlier.outs[0].cpu()[:n_first].numpy()
    draws = draw_table(dev, 1001)
    results = []
    for form in ("two launches", "one launch", "one launch, pinned crop table", "ops.crop_regularize_pinned"):
        c = Crop(dev, specs)
        outs = [guarded((size, 3), F32, device=dev) for _ in specs]
        infos = [guarded((2,), I32, device=dev) for _ in specs]
        rj = np.zeros(len(specs), ops.REGULARIZE_JOB)
        for k, s in enumerate(specs):
            segs = [(c.outs[k], c.cnts[k], s['capacity'])]
            if k == 1:
                segs.insert(0, (earlier.outs[0], earlier.cnts[0], earlier.specs[0]['capacity']))
            for i, (rows, cnt, cap) in enumerate(segs):
                rj['seg'][k][i], rj['seg_count'][k][i], rj['seg_capacity'][k][i] = rows.data_ptr(), cnt.data_ptr(), cap
            rj['out'][k], rj['info'][k], rj['n_seg'][k], rj['input_size'][k] = outs[k].data_ptr(), infos[k].data_ptr(), len(segs), size
        rtable = ops.upload_jobs(rj)
        n = len(specs)
        if form == "two launches":
            c.launch()
            L("ptt_regularize_f32", dev, P(rtable), n, P(draws), draws.numel())
        elif form == "one launch":
            ctable = ops.upload_jobs(c.jobs)
            L("ptt_crop_regularize_f32", dev, P(ctable), P(rtable), n, P(draws), draws.numel())
        else:
            pinned = torch.from_numpy(c.jobs.view(np.uint8).reshape(-1).copy()).pin_memory()
            if form.startswith("ops"):
                ops.crop_regularize_pinned(pinned, rtable, n, draws.contiguous())
            else:
                L("ptt_crop_regularize_f32", dev, ctypes.c_void_p(pinned.data_ptr()), P(rtable), n, P(draws), draws.numel())
        torch.cuda.synchronize()
        counts = c.check()
        for t in outs + infos:
            check_guard(t)
        check_guard(draws, all_written=False)
        check_guard(earlier.outs[0], all_written=False)
        results.append((form, [words(t).clone() for t in c.state + outs + infos], counts, outs, infos))
    for form, state, _, _, _ in results[1:]:
        for a, b in zip(results[0][1], state):
            assert torch.equal(a, b), "%s against crop_compact followed by regularize" % form
    # and directly against the oracle
    _, _, counts, outs, infos = results[1]
    assert counts[2] == 1100 and counts[3] == 0 and counts[0] > 2 and counts[1] > 2
    for k, s in enumerate(specs):
        rows = expected(s)[0][:s['capacity']]
        if k == 1:
            rows = np.concatenate([first_rows, rows], axis=0)
        n = rows.shape[0]
        want = np.ascontiguousarray(TR.regularize_pc(np.ascontiguousarray(rows.T), size))
        same_bits(outs[k], torch.from_numpy(want), "job %d against regularize_pc(crop_center_pc)" % k)
        used = 0 if n <= 2 or n == size else draws_consumed(n, size, 1001)[0]
        assert infos[k].cpu().tolist() == [n, used], "job %d: info" % k


# ============================================================================================================== select_box
PATTERNS = ["random", "max first", "max last", "tie p and p + 64", "ties across lanes", "all equal", "all -inf", "one +inf", "one NaN",
            "several NaN", "all NaN"]


def select_rows(g, kinds, Pn):
    """(len(kinds), Pn, 5) float32: offsets in [-1, 1] (never redrawn by get_box_by_offset), scores by pattern."""
    pred = torch.rand(len(kinds), Pn, 5, generator=g, dtype=F32) * 2 - 1
    for b, kind in enumerate(kinds):
        s = pred[b, :, 4]
        if kind == "max first":
            s[0] = 5.0
        elif kind == "max last":
            s[Pn - 1] = 5.0
        elif kind == "tie p and p + 64":
            p = 1 if Pn > 65 else 0
            s[p], s[p + 64 if Pn > p + 64 else Pn - 1] = 5.0, 5.0
        elif kind == "ties across lanes":
            for p in (Pn - 1, Pn // 2, min(3, Pn - 1)):
                s[p] = 5.0
        elif kind == "all equal":
            s[:] = 0.25
        elif kind == "all -inf":
            s[:] = float("-inf")
        elif kind == "one +inf":
            s[Pn // 3] = float("inf")
        elif kind == "one NaN":
            s[0] = 7.0                                      # a finite score above the rest, in front of the NaN (P > 1)
            s[Pn // 2] = float("nan")
        elif kind == "several NaN":
            for p in (Pn - 1, (2 * Pn) // 3, Pn // 3):
                s[p] = float("nan")
            if Pn > 65:
                s[Pn // 3 + 64] = float("nan")              # the same lane as the first one
        elif kind == "all NaN":
            s[:] = float("nan")
    return pred


@pytest.mark.parametrize("Pn", [1, 5, 63, 64, 65, 130])
@pytest.mark.parametrize("B", [1, 3, 4, 5, 9])
def test_select_box_equals_argmax_and_the_host_selection(dev, B, Pn):
    g = torch.Generator().manual_seed(B * 1000 + Pn)
    for first in range(0, len(PATTERNS), B):
        kinds = [PATTERNS[(first + b) % len(PATTERNS)] for b in range(B)]
        pred = select_rows(g, kinds, Pn)
        want = np.argmax(pred[:, :, 4].numpy(), axis=1)
        for b, kind in enumerate(kinds):
            if "NaN" in kind:
                assert np.isnan(pred[b, want[b], 4].item()) and not bool(torch.isnan(pred[b, :want[b], 4]).any()), kind
        rows = pred[torch.arange(B), torch.from_numpy(want)]
        pe = embed(pred.to(dev))
        tag = "B %d, P %d, %s" % (B, Pn, kinds)
        out, idx = guarded((B, 5), F32, device=dev), guarded((B,), I32, device=dev)
        L("ptt_select_box_f32", dev, P(pe), B, Pn, P(out), P(idx))
        torch.cuda.synchronize()
        check_guard(out), check_guard(idx), check_guard(pe, all_written=False)
        assert idx.cpu().tolist() == want.tolist(), tag
        same_bits(out, rows, tag + ": the selected rows")
        out2 = guarded((B, 5), F32, device=dev)
        L("ptt_select_box_f32", dev, P(pe), B, Pn, P(out2), None)                    # idx_out NULL; a second launch
        torch.cuda.synchronize()
        check_guard(out2)
        same_bits(out2, out, tag + ": idx_out NULL")
        same_bits(ops.select_box(pe.contiguous()), out, tag + " against ops.select_box")
        if Pn > 1:                                          # the host-side selection a small batch takes
            boxes = np.zeros(B, ops.TRACK_BOX)
            boxes['wlh'], boxes['quat'] = 100.0, (1.0, 0.0, 0.0, 0.0)
            est = np.full((B, 5), -3.0, np.float32)
            ops.track_select_update(pred.numpy(), np.zeros((B, 2, 2), np.int32), boxes, True, None, np.zeros(B, np.int64), est)
            same_bits(out, torch.from_numpy(est), tag + " against ptt_track_select_update")


def test_select_box_refusals(dev):
    pe = embed(torch.zeros(2, 3, 5).to(dev))
    out, idx = guarded((2, 5), F32, device=dev), guarded((2,), I32, device=dev)
    for args in ((P(pe), -1, 3, P(out), P(idx)), (P(pe), 2, 0, P(out), P(idx)), (None, 2, 3, P(out), P(idx)), (P(pe), 2, 3, None, P(idx))):
        with pytest.raises(RuntimeError, match="PTT_EINVAL"):
            L("ptt_select_box_f32", dev, *args)
    torch.cuda.synchronize()
    guard.assert_untouched(out, idx)
