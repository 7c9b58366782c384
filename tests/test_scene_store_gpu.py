"""The scan kernels and what stands on them, on the GPU, bit for bit against the numpy restatements of tests/scene_ref.py (which
fixture g26 ties to the reference's own PointCloud / crop_pc):

  1. ptt_scan_ingest_f32 on the C ABI behind guard bands — every N at which the geometry changes (one lane, one wave minus one,
     a whole chunk, a chunk plus one, two chunks plus one), 3 / 4 / 5 floats per row, aligned and one-float-offset bases (the
     16-byte load must not be taken), 0..4 steps of every kind, ld > N, ragged jobs plus an empty one in one launch, the table
     in device and in pinned host memory, and the fixture's scans;
  2. ptt_scan_preload_f32 — counting call, writing call, capacity < count, keep-none / keep-all, a bound equal to a coordinate,
     a repeated call, a short workspace, the fixture's crops;
  3. SceneStore — shared buffers and pointers, PackedTrackletRunner on the store's views == on private host arrays;
  4. SceneStore.preload -> TrainBatchFeeder in place == the feeder on host copies;
  5. OnlineTracker.step_raw == step on the restatement's scan, and its refusals.
"""
import os

import numpy as np
import pytest
import torch

from ptt_amd import synth
from tests import guard
from tests import scene_ref as SR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 1024
_cache = {}


def _g26():
    if "g26" not in _cache:
        _cache["g26"] = dict(np.load(os.path.join(ROOT, "tests", "golden", "g26_scene_store.npz")))
    return _cache["g26"]


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _same_bits(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    assert np.array_equal(g, w), "%s: %d of %d words differ" % (what, int((g != w).sum()), g.size)


def _chains():
    """Step lists of 0..4 steps that between them use every kind; translations of hundreds of metres (the float32 store between
    the steps shows)."""
    g = _g26()
    rs = np.random.RandomState(7)
    A3 = np.hstack([g["nus_r2"], [[311.25], [-1180.5], [2.125]]])
    return [[],
            [('rotate', g["nus_r1"])], [('translate', g["nus_t2"])], [('affine', g["v2c"])], [('affine', A3)],
            [('rotate', g["nus_r2"]), ('translate', g["nus_t2"])],
            [('affine', g["v2c"]), ('rotate', g["nus_r2"]), ('translate', -g["nus_t2"])],
            [('rotate', g["nus_r1"]), ('translate', g["nus_t1"]), ('rotate', g["nus_r2"]), ('translate', g["nus_t2"])],
            [('translate', rs.uniform(-500, 500, 3)), ('affine', A3), ('affine', g["v2c"]), ('rotate', rs.standard_normal((3, 3)))]]


def _raw(rs, n, c):
    return np.ascontiguousarray((rs.uniform(-1, 1, (n, c)) * ([40.0, 40.0, 3.0] + [0.5] * (c - 3))).astype(np.float32))


def _ingest_jobs(dev, specs):
    """specs: [(raw (N, C) numpy, steps, base offset in floats, ld - N)] -> (SCAN_JOB table, guarded outputs, what keeps the inputs alive)."""
    from ptt_amd import ops
    jobs = np.zeros(len(specs), ops.SCAN_JOB)
    outs, keep = [], []
    for i, (raw, steps, off, pad) in enumerate(specs):
        n, c = raw.shape
        buf = torch.full((off + n * c + 4,), float('nan'), dtype=torch.float32, device=dev)
        buf[off:off + n * c] = torch.from_numpy(raw.reshape(-1)).to(dev)
        assert buf.data_ptr() % 16 == 0
        out = guard.guarded((3, max(n, 1)), torch.float32, ld=max(n, 1) + pad, device=dev)
        recs = ops.scan_steps(steps)
        jobs['raw'][i], jobs['out'][i], jobs['ld'][i] = buf.data_ptr() + 4 * off, out.data_ptr(), out.stride(0)
        jobs['n_points'][i], jobs['row_floats'][i], jobs['n_steps'][i] = n, c, len(recs)
        jobs['steps'][i, :len(recs)] = recs
        outs.append(out)
        keep.append(buf)
    return jobs, outs, keep


def _check_ingest(specs, outs, what):
    for i, ((raw, steps, off, pad), out) in enumerate(zip(specs, outs)):
        n = raw.shape[0]
        if n == 0:
            guard.assert_untouched(out)                                   # an empty job writes nothing
            continue
        guard.check_guard(out)                                           # nothing outside out[r * ld + 0 .. n), every element written
        _same_bits(out, SR.ingest_ref(raw, steps), "%s job %d: N %d C %d offset %d, %d steps" % (what, i, n, raw.shape[1], off, len(steps)))


def _ingest_specs():
    rs = np.random.RandomState(11)
    chains = _chains()
    specs = []
    for n in (1, 63, CHUNK, CHUNK + 1, 2 * CHUNK + 1):
        for c in (3, 4, 5):
            for off in (0, 1):
                specs.append((_raw(rs, n, c), chains[len(specs) % len(chains)], off, (0, 5, 3)[len(specs) % 3]))
    specs.insert(7, (np.zeros((0, 4), np.float32), chains[3], 0, 0))       # an empty job among the others
    return specs


def test_ingest_kernel_equals_the_restatement(dev):
    """31 ragged jobs in ONE launch, from a table on the device and again from a table in pinned host memory."""
    from ptt_amd import ops
    specs = _ingest_specs()
    used = {(len(s[1]), tuple(k for k, _ in s[1])) for s in specs}
    assert {n for n, _ in used} == {0, 1, 2, 3, 4} and {k for _, ks in used for k in ks} == {'rotate', 'translate', 'affine'}
    # every (N, C) pair runs from an aligned and from a one-float-offset base, with some chain that moves the points
    max_points = max(s[0].shape[0] for s in specs)
    jobs, outs, keep = _ingest_jobs(dev, specs)
    assert any(j['row_floats'] == 4 and j['raw'] % 16 == 0 for j in jobs) and any(j['row_floats'] == 4 and j['raw'] % 16 == 4 for j in jobs)
    ops.scan_ingest(jobs, len(jobs), max_points, dev)
    torch.cuda.synchronize()
    _check_ingest(specs, outs, "device table")
    jobs2, outs2, keep2 = _ingest_jobs(dev, specs)
    pinned = torch.from_numpy(jobs2.view(np.uint8).reshape(-1).copy()).pin_memory()
    ops.scan_ingest_check(jobs2, len(jobs2), max_points)
    ops.scan_ingest_device(pinned, len(jobs2), max_points, dev)
    torch.cuda.synchronize()
    _check_ingest(specs, outs2, "pinned table")
    for a, b in zip(outs, outs2):
        if a.shape[1] > 0:
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_ingest_kernel_gives_the_fixtures_scans(dev):
    from ptt_amd import ops
    g = _g26()
    chain = [('rotate', g["nus_r1"]), ('translate', g["nus_t1"]), ('rotate', g["nus_r2"]), ('translate', g["nus_t2"])]
    specs = [(g["raw_%d" % k], [('affine', g["v2c"])], 0, 0) for k in range(3)] + [(g["raw_%d" % k], chain, 0, 0) for k in (2, 3)]
    want = [g["kitti_%d" % k] for k in range(3)] + [g["nus_%d" % k] for k in (2, 3)]
    jobs, outs, keep = _ingest_jobs(dev, specs)
    ops.scan_ingest(jobs, len(jobs), 2049, dev)
    torch.cuda.synchronize()
    for i, (out, w) in enumerate(zip(outs, want)):
        guard.check_guard(out)
        _same_bits(out, w, "fixture scan %d" % i)


def test_ingest_refuses_bad_launch_arguments(dev):
    specs = [(_raw(np.random.RandomState(1), 8, 4), [], 0, 0)]
    jobs, outs, keep = _ingest_jobs(dev, specs)
    from ptt_amd import ops
    table = ops.upload_jobs(jobs)
    for args in ((None, 1, 8), (guard.ptr(table), 0, 8), (guard.ptr(table), 65536, 8), (guard.ptr(table), 1, 0), (guard.ptr(table), -1, 8)):
        with pytest.raises(RuntimeError, match="EINVAL"):
            guard.launch("ptt_scan_ingest_f32", dev, *args)
    torch.cuda.synchronize()
    guard.assert_untouched(outs[0])


# ---------------------------------------------------------------------------------------------------------------- preload
def _preload_cases():
    """[(points (3, N) float32, lo, hi, what)]: the fixture's three crops and synthetic edge cases."""
    g = _g26()
    cases = [(g["kitti_%d" % int(g["scan_%d" % j])], g["lo_%d" % j], g["hi_%d" % j], "fixture crop %d" % j) for j in range(3)]
    rs = np.random.RandomState(5)
    big = np.ascontiguousarray(_raw(rs, 2 * CHUNK + 1, 3).T)
    cases.append((big, [-1e9] * 3, [1e9] * 3, "keep all"))
    cases.append((big, [50.0, -1e9, -1e9], [60.0, 1e9, 1e9], "keep none"))
    cases.append((big, [-20.0, -10.0, -1.0], [25.0, 30.0, 2.0], "three chunks, a part of each"))
    # strictness: the lower x bound IS point 5's x, the upper y bound IS point 700's y: both points fall, their equals too
    lo, hi = np.array([float(big[0, 5]), -1e9, -1e9]), np.array([1e9, float(big[1, 700]), 1e9])
    cases.append((big, lo, hi, "bounds equal to coordinates"))
    line = np.zeros((3, 5), np.float32)
    line[0] = [0, 1, 2, 3, 4]
    cases.append((line, [0.0, -1.0, -1.0], [4.0, 1.0, 1.0], "five points on a line, the outer two on the bounds"))
    cases.append((np.ascontiguousarray(_raw(rs, 63, 3).T), [-30.0] * 3, [30.0] * 3, "one wave minus one"))
    cases.append((np.zeros((3, 0), np.float32), [-1.0] * 3, [1.0] * 3, "empty cloud"))
    return cases


def _preload_table(dev, cases, counts_view, outs, capacity):
    from ptt_amd import ops
    jobs = np.zeros(len(cases), ops.PRELOAD_JOB)
    keep = []
    for i, (pts, lo, hi, _) in enumerate(cases):
        n = pts.shape[1]
        src = guard.embed(torch.from_numpy(np.ascontiguousarray(pts if n else np.zeros((3, 1), np.float32))).to(dev), ld=max(n, 1) + 3)
        keep.append(src)
        jobs['points'][i], jobs['ld'][i], jobs['n_points'][i] = src.data_ptr(), src.stride(0), n
        jobs['lo'][i], jobs['hi'][i] = lo, hi
        jobs['count'][i] = counts_view.data_ptr() + 4 * i
        if outs is not None:
            jobs['out'][i], jobs['out_ld'][i], jobs['capacity'][i] = outs[i].data_ptr(), outs[i].stride(0), capacity[i]
    return jobs, keep


def test_preload_kernel(dev):
    from ptt_amd import ops
    cases = _preload_cases()
    J = len(cases)
    want = [SR.preload_ref(p, lo, hi) for p, lo, hi, _ in cases]
    n_want = [w.shape[1] for w in want]
    names = [c[3] for c in cases]
    assert n_want[names.index("keep all")] == 2 * CHUNK + 1 and n_want[names.index("keep none")] == 0 and n_want[2] == 0 and n_want[0] > 50
    strict = names.index("bounds equal to coordinates")
    assert n_want[strict] < 2 * CHUNK + 1 and n_want[names.index("five points on a line, the outer two on the bounds")] == 3 and 0 < n_want[names.index("three chunks, a part of each")] < 2 * CHUNK
    max_points = 2 * CHUNK + 1
    nbytes = ops.scan_preload_workspace(J, max_points)
    assert nbytes == J * 3 * 4                                          # one int32 per job and chunk
    outs = [guard.guarded((3, max(n, 1)), torch.float32, ld=max(n, 1) + 2, device=dev) for n in n_want]

    # 1. the counting call: out = NULL; the counts are the restatement's, nothing else is written
    counts = guard.guarded((J,), torch.int32, device=dev)
    ws = guard.workspace(nbytes, device=dev)
    jobs, keep = _preload_table(dev, cases, counts, None, None)
    ops.scan_preload_device(ops.upload_jobs(jobs), J, max_points, ws)
    torch.cuda.synchronize()
    guard.check_guard(counts)
    guard.check_guard(ws)
    assert counts.cpu().tolist() == n_want
    guard.assert_untouched(*outs)

    # 2. a short workspace: PTT_EINVAL and nothing written, the counts included
    counts2 = guard.guarded((J,), torch.int32, device=dev)
    jobs, keep2 = _preload_table(dev, cases, counts2, outs, n_want)
    table = ops.upload_jobs(jobs)
    short = guard.workspace(nbytes - 4, device=dev)
    with pytest.raises(RuntimeError, match="EINVAL"):
        ops.scan_preload_device(table, J, max_points, short)
    for args in ((None, J, max_points, guard.ptr(ws), nbytes), (guard.ptr(table), 0, max_points, guard.ptr(ws), nbytes),
                 (guard.ptr(table), J, 0, guard.ptr(ws), nbytes), (guard.ptr(table), J, max_points, None, nbytes)):
        with pytest.raises(RuntimeError, match="EINVAL"):
            guard.launch("ptt_scan_preload_f32", dev, *args)
    torch.cuda.synchronize()
    guard.assert_untouched(counts2, short, *outs)

    # 3. the writing call == the restatement, behind guards; a second call writes identical bytes
    ops.scan_preload_device(table, J, max_points, ws)
    torch.cuda.synchronize()
    first = [o.clone() for o in outs]
    for i, (o, w) in enumerate(zip(outs, want)):
        if n_want[i]:
            guard.check_guard(o)
            _same_bits(o, w, names[i])
        else:
            guard.assert_untouched(o)
    assert counts2.cpu().tolist() == n_want
    ops.scan_preload_device(table, J, max_points, ws)
    torch.cuda.synchronize()
    for o, f in zip(outs, first):
        assert torch.equal(o.view(torch.int32), f.view(torch.int32))
    guard.check_guard(ws)

    # 4. capacity < count: the count is still the whole number, columns from `capacity` on are untouched
    cap = [n // 2 for n in n_want]
    small = [guard.guarded((3, max(c, 1)), torch.float32, ld=max(c, 1) + 1, device=dev) for c in cap]
    counts3 = guard.guarded((J,), torch.int32, device=dev)
    jobs, keep3 = _preload_table(dev, cases, counts3, small, cap)
    ops.scan_preload_device(ops.upload_jobs(jobs), J, max_points, ws)
    torch.cuda.synchronize()
    assert counts3.cpu().tolist() == n_want
    for i, (o, w) in enumerate(zip(small, want)):
        if cap[i]:
            guard.check_guard(o)
            _same_bits(o, w[:, :cap[i]], "%s, capacity %d of %d" % (names[i], cap[i], n_want[i]))
        else:
            guard.assert_untouched(o)


# ---------------------------------------------------------------------------------------------------------------- the scene
T = 6
SCENE = "0019"
LIVES = [(0, 0, 6), (1, 1, 5), (2, 2, 6)]                 # (tracklet, first frame, end): three tracklets over six shared scans


def _scene():
    """Six scans of ~3k points holding three synthetic tracklets 40 m apart, as the sensor would deliver them: (N, 4) or (N, 5)
    rows in a sensor frame, with the rigid transform that takes them to the frame the boxes live in."""
    if "scene" not in _cache:
        g = _g26()
        shifts = np.array([(0, 0, 0), (40, 0, 0), (0, 40, 0)], np.float32)
        tr = [synth.tracklet(600 + k, T, n_obj=(150, 400), n_bg=(600, 900)) for k in range(3)]
        rs = np.random.RandomState(3)
        v2c = g["v2c"]
        R, t = v2c[:3, :3], v2c[:3, 3]
        raws, clouds = [], []
        for f in range(T):
            pts = np.concatenate([tr[k][0][f] + shifts[k][:, None] for k in range(3)], axis=1).astype(np.float64)
            c = 5 if f == 4 else 4
            raw = np.concatenate([(R.T @ (pts - t[:, None])).T, rs.uniform(0, 1, (pts.shape[1], c - 3))], axis=1)
            raws.append(np.ascontiguousarray(raw.astype(np.float32)))
        steps = [('affine', v2c)]
        clouds = [SR.ingest_ref(r, steps) for r in raws]                   # what the reference would hold for these scans
        assert all(2000 < c.shape[1] < 4096 for c in clouds)
        boxes = [[((b[0].astype(np.float32) + shifts[k]).astype(np.float64), b[1], b[2]) for b in tr[k][1]] for k in range(3)]
        _cache["scene"] = (raws, steps, clouds, boxes)
    return _cache["scene"]


def _store(dev):
    from ptt_amd.scene_store import SceneStore
    raws, steps, clouds, boxes = _scene()
    store = SceneStore(dev)
    store.add_scans(SCENE, range(T), raws, steps=steps)
    return store


def test_scene_store_ingests_shares_and_releases(dev):
    from ptt_amd.scene_store import SceneStore
    raws, steps, clouds, boxes = _scene()
    store = _store(dev)
    total = sum(c.shape[1] for c in clouds)
    assert len(store) == T and store.nbytes == 3 * total * 4 and (SCENE, 3) in store and (SCENE, T) not in store and ("other", 3) not in store
    views = [store.scan(SCENE, f) for f in range(T)]
    for f, v in enumerate(views):
        assert v.dtype == torch.float32 and tuple(v.shape) == clouds[f].shape and v.stride() == (total, 1)
        _same_bits(v, clouds[f], "scan %d" % f)
    base = views[0].untyped_storage().data_ptr()
    assert all(v.untyped_storage().data_ptr() == base for v in views)                    # one buffer for the call
    assert [v.data_ptr() - base for v in views] == [4 * int(o) for o in np.cumsum([0] + [c.shape[1] for c in clouds[:-1]])]
    a = store.tracklet(SCENE, range(0, 6), boxes[0])
    b = store.tracklet(SCENE, range(2, 6), boxes[2][2:6])
    assert [t.data_ptr() for t in a[0][2:6]] == [t.data_ptr() for t in b[0]] and len(b[1]) == 4
    # refusals change nothing: resident again, listed twice, lengths, a bad array, bad steps, unknown frames
    for kw in (dict(frames=[9, 3], raws=raws[:2]), dict(frames=[9, 9], raws=raws[:2]), dict(frames=[9], raws=raws[:2]),
               dict(frames=[9], raws=[raws[0].astype(np.float64)]), dict(frames=[9], raws=[raws[0][:, :2].copy()]),
               dict(frames=[9], raws=[raws[0].T]), dict(frames=[9], raws=[raws[0]], steps=[('shear', np.eye(3))]),
               dict(frames=[9, 10], raws=raws[:2], steps=[[('rotate', np.eye(3))]]), dict(frames=[9], raws=[raws[0]], steps=[[('rotate', np.eye(4))]])):
        with pytest.raises(ValueError):
            store.add_scans(SCENE, **kw)
        assert len(store) == T and (SCENE, 9) not in store
    with pytest.raises(ValueError):
        store.tracklet(SCENE, [0, 1], boxes[0][:1])
    with pytest.raises(KeyError):
        store.scan(SCENE, 9)
    # a second call: numpy, pinned, device and empty scans, 4 and 5 floats per row, one step list per frame
    chains = _chains()
    mixed = [raws[0], torch.from_numpy(raws[4]).pin_memory(), torch.from_numpy(raws[2]).to(dev), np.zeros((0, 7), np.float32), raws[5][:1001].copy()]
    per = [chains[7], chains[5], None, chains[3], []]
    store.add_scans("mixed", [10, 11, 12, 13, 14], mixed, steps=per)
    for f, r, s in zip([10, 11, 12, 13, 14], [raws[0], raws[4], raws[2], mixed[3], mixed[4]], per):
        _same_bits(store.scan("mixed", f), SR.ingest_ref(r, s), "mixed scan %d" % f)
    assert store.scan("mixed", 13).shape == (3, 0) and store.frames("mixed") == [10, 11, 12, 13, 14]
    assert store.scan("mixed", 10).untyped_storage().data_ptr() != base
    # release drops the store's references; what was handed out stays valid
    n_before = store.nbytes
    store.release(SCENE)
    assert (SCENE, 3) not in store and len(store) == 5 and store.nbytes == n_before - 3 * total * 4
    _same_bits(views[3], clouds[3], "a view after release")
    store.add_scans(SCENE, [3], [raws[3]], steps=steps)                                  # ... and the frame can come back
    _same_bits(store.scan(SCENE, 3), clouds[3], "scan 3 again")
    with pytest.raises(RuntimeError):
        SceneStore("cpu")


def test_packed_runner_on_store_views_equals_private_host_arrays(dev):
    from ptt_amd.packed_runner import PackedTrackletRunner
    from tests.test_online_tracker_gpu import _tracker
    raws, steps, clouds, boxes = _scene()
    store = _store(dev)
    shared = [store.tracklet(SCENE, range(t0, t1), boxes[k][t0:t1]) for k, t0, t1 in LIVES]
    private = [([clouds[f].copy() for f in range(t0, t1)], boxes[k][t0:t1]) for k, t0, t1 in LIVES]
    assert shared[0][0][3].data_ptr() == shared[1][0][2].data_ptr() == shared[2][0][1].data_ptr()        # frame 3, three tracklets
    pr = PackedTrackletRunner(_tracker(dev), dev, slots=2)
    got = pr.run(shared)
    want = pr.run(private)
    assert [len(r) for r in got] == [t1 - t0 for _, t0, t1 in LIVES] == [len(r) for r in want]
    moved = 0
    for t, (g_rows, w_rows) in enumerate(zip(got, want)):
        for i, (g, w) in enumerate(zip(g_rows, w_rows)):
            assert len(g) == len(w)
            for a, b in zip(g[:3], w[:3]):
                np.testing.assert_array_equal(a, b, err_msg="tracklet %d frame %d" % (t, i))
            assert len(w) == 3 or g[3] == w[3]
            moved += int(i > 0 and float(np.abs(g[0] - w_rows[0][0]).max()) > 1e-6)
    assert moved > 0
    for f in range(T):                                                  # the runner read the store's scans, it did not write them
        _same_bits(store.scan(SCENE, f), clouds[f], "scan %d after the run" % f)


def test_preload_feeds_the_train_batch_feeder_in_place(dev):
    from ptt_amd.train_feed import TrainBatchFeeder
    raws, steps, clouds, boxes = _scene()
    store = _store(dev)
    offset = 2.0
    on_dev, on_host, buffers = [], [], []
    for k, t0, t1 in LIVES:
        crops, bx = store.preload(SCENE, range(t0, t1), boxes[k][t0:t1], offset)
        base = crops[0].untyped_storage()
        assert all(c.untyped_storage().data_ptr() == base.data_ptr() for c in crops) and base.nbytes() == 3 * sum(c.shape[1] for c in crops) * 4
        for f, c, b in zip(range(t0, t1), crops, bx):                   # crop_pc(scan, box, offset) per frame
            lo, hi = SR.crop_bounds(b[0], b[1], b[2], offset)
            want = SR.preload_ref(clouds[f], lo, hi)
            assert 20 < want.shape[1] < clouds[f].shape[1]
            _same_bits(c, want, "preload tracklet %d frame %d" % (k, f))
        on_dev.append((crops, bx))
        on_host.append(([c.cpu().numpy() for c in crops], bx))
        buffers.append((base.data_ptr(), base.nbytes()))
    # offset <= 0: the reference does not crop — the store's own views
    same, _ = store.preload(SCENE, range(0, 3), boxes[0][0:3], -1)
    assert [c.data_ptr() for c in same] == [store.scan(SCENE, f).data_ptr() for f in range(3)]
    kw = dict(batch_size=4, search_size=128, template_size=64, seed=26)
    fa, fb = TrainBatchFeeder(on_dev, dev, **kw), TrainBatchFeeder(on_host, dev, **kw)
    ptrs = [int(p) for p in fa.ptr]
    assert ptrs == [c.data_ptr() for crops, _ in on_dev for c in crops]                  # in place: the store's memory
    assert all(any(lo <= p < lo + n for lo, n in buffers) for p in ptrs)
    assert not any(any(lo <= int(p) < lo + n for lo, n in buffers) for p in fb.ptr)
    for b in range(2):
        ba, bb = fa.batch(0, b), fb.batch(0, b)
        torch.cuda.synchronize()
        for key in ('search_points', 'template_points', 'cls_label', 'reg_label'):
            assert torch.equal(ba[key].view(torch.int32), bb[key].view(torch.int32)), (b, key)
        assert float(ba['search_points'].abs().max()) > 0 and torch.equal(fa.last.src, fb.last.src)


# ---------------------------------------------------------------------------------------------------------------- step_raw
CAPACITY = 4096


def _state(ot):
    return (list(ot.targets), ot.boxes.copy(), ot.rng_pos.copy(), ot.cur, ot.n_prev)


def _same_state(ot, state):
    assert ot.targets == state[0] and ot.cur == state[3] and ot.n_prev == state[4]
    assert np.array_equal(ot.boxes, state[1]) and np.array_equal(ot.rng_pos, state[2])


def test_step_raw_equals_step_on_the_ingested_scan(dev):
    """Five scans: A added on scan 0, B on scan 2, A dropped on scan 3; the raw scan arrives as a numpy array, a pinned tensor, a
    device tensor and with 5 floats per row (scan 4: the staging buffer grows)."""
    from ptt_amd.online_tracker import OnlineTracker
    from tests.test_online_tracker_gpu import _tracker
    raws, steps, clouds, boxes = _scene()
    a = OnlineTracker(_tracker(dev), dev, slots=2, scan_capacity=CAPACITY)
    b = OnlineTracker(_tracker(dev), dev, slots=2, scan_capacity=CAPACITY)
    adds = {0: {"A": boxes[0][0]}, 2: {"B": boxes[1][2]}}
    drops = {3: ("A",)}
    forms = [lambda r: r, lambda r: torch.from_numpy(r).pin_memory(), lambda r: torch.from_numpy(r).to(dev), lambda r: r, lambda r: r]
    moved = 0
    for t in range(5):
        if t == 1:
            state = _state(a)
            r = raws[t]
            bad = [dict(raw=r.astype(np.float64)), dict(raw=r[:, 0].copy()), dict(raw=r[::2]), dict(raw=r[:, :2].copy()),
                   dict(raw=np.zeros((CAPACITY + 1, 4), np.float32)), dict(raw=r, steps=[('shear', np.eye(3))]),
                   dict(raw=r, steps=[('rotate', np.eye(3))] * 5), dict(raw=r, steps=[('affine', np.eye(3))]), dict(raw=list(r)),
                   dict(raw=torch.from_numpy(r).double()), dict(raw=r, drop=("nobody",)), dict(raw=r, add={"A": boxes[0][1]})]
            for kw in bad:
                kw.setdefault("steps", steps)
                with pytest.raises(ValueError):
                    a.step_raw(**kw)
                _same_state(a, state)
        got = a.step_raw(forms[t](raws[t]), steps, add=adds.get(t), drop=drops.get(t, ()))
        want = b.step(clouds[t], add=adds.get(t), drop=drops.get(t, ()))
        assert list(got) == list(want) == {0: ["A"], 1: ["A"], 2: ["A", "B"], 3: ["B"], 4: ["B"]}[t]
        for i in want:
            for x, y in zip(got[i][:3], want[i][:3]):
                np.testing.assert_array_equal(x, y, err_msg="target %s step %d" % (i, t))
            assert got[i][3] == want[i][3], (i, t, got[i][3], want[i][3])
            moved += int(want[i][3] is not None)
        _same_state(a, _state(b))
        _same_bits(a.scans[1 - a.cur, :, :a.n_prev], clouds[t], "the resident scan of step %d" % t)
    assert moved == 4 and a._raw_stage.numel() == CAPACITY * 5
    # an empty raw scan is an empty scan
    got, want = a.step_raw(np.zeros((0, 4), np.float32), steps), b.step(np.zeros((3, 0), np.float32))
    for x, y in zip(got["B"][:3], want["B"][:3]):
        np.testing.assert_array_equal(x, y)
    assert got["B"][3] == want["B"][3]
