"""Timing of the raw-scan path -> profiles/scene_store_timing.json (and the same JSON line on stdout).

    python scripts/scene_store_timing.py [--rounds 30] [--out profiles/scene_store_timing.json]

Both sides of every comparison alternate inside one loop of one process, after warm-ups; medians and minima of `--rounds` rounds.
(a) Ingest of one 131072 x 4 scan. Kernel: device events around `--reps` back-to-back ptt_scan_ingest_f32 launches (raw rows
    already on the device), per launch, without a step and with one AFFINE step. The host path it replaces, on a host clock:
    np.ascontiguousarray(raw[:, :3].T) (with the step: the reference's PointCloud.transform on top) plus the upload of the
    planar (3, N) array, ended by a device synchronise. End to end: SceneStore.add_scans of the host array (one staging upload
    of N x 4 floats + the kernel) against that host path, both from the same pageable array.
(b) OnlineTracker.step_raw(raw) against the host transpose + OnlineTracker.step(planar) at 1 and 8 live targets, N = 131072,
    with and without an AFFINE step (the host side then also runs numpy's transform): host clock around the call, which ends in
    a device synchronise.
(c) PackedTrackletRunner over synthetic scenes whose clouds are whole scans: SceneStore views (every scan uploaded and ingested
    once, tracklets share it) against per-tracklet host arrays (every tracklet uploads every scan it passes through). Bytes
    uploaded on each side, wall time of run(), and for the store the ingest of the scenes beside it.
Without a device this raises: there is no CPU figure to give.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ptt_amd import ops                                         # noqa: E402

N_SCAN = 131072
V2C = np.array([[7.533745e-03, -9.999714e-01, -6.166020e-04, -4.069766e-03],
                [1.480249e-02, 7.280733e-04, -9.998902e-01, -7.631618e-02],
                [9.998621e-01, 7.523790e-03, 1.480755e-02, -2.717806e-01],
                [0.0, 0.0, 0.0, 1.0]])                          # a velodyne -> camera calibration of the usual shape


def _stats(ms):
    return {"median_ms": round(float(np.median(ms)), 5), "min_ms": round(float(np.min(ms)), 5)}


def _raw(rs, n, c=4):
    return np.ascontiguousarray((rs.uniform(-1, 1, (n, c)) * ([50.0, 50.0, 2.0] + [0.5] * (c - 3))).astype(np.float32))


def _host_planar(raw, affine):
    """What the reference does on the host: the first three columns transposed, and PointCloud.transform where a step is asked for."""
    pts = np.ascontiguousarray(raw[:, :3].T)
    if affine is not None:
        pts[:3, :] = affine.dot(np.vstack((pts[:3, :], np.ones(pts.shape[1]))))[:3, :]
    return pts


def _wall(fn):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def ingest_timing(dev, args):
    from ptt_amd.scene_store import SceneStore
    rs = np.random.RandomState(0)
    raw = _raw(rs, N_SCAN)
    raw_dev = torch.from_numpy(raw).to(dev)
    out = torch.empty((3, N_SCAN), dtype=torch.float32, device=dev)
    rows = []
    for name, steps, affine in (("deinterleave", None, None), ("affine", [('affine', V2C)], V2C)):
        jobs = np.zeros(1, ops.SCAN_JOB)
        recs = ops.scan_steps(steps)
        jobs['raw'], jobs['out'], jobs['ld'], jobs['n_points'], jobs['row_floats'], jobs['n_steps'] = raw_dev.data_ptr(), out.data_ptr(), N_SCAN, N_SCAN, 4, len(recs)
        jobs['steps'][0, :len(recs)] = recs
        table = ops.scan_ingest(jobs, 1, N_SCAN, dev)
        torch.cuda.synchronize()
        host_planar = _host_planar(raw, affine)
        same = bool(np.array_equal(out.cpu().numpy().view(np.int32), host_planar.view(np.int32)))     # numpy's dot: compared, not assumed
        store = SceneStore(dev)
        frame = [0]

        def kernel():
            ops.scan_ingest_device(table, 1, N_SCAN)

        def host_transpose():
            return _host_planar(raw, affine)

        def host_path():
            torch.from_numpy(_host_planar(raw, affine)).to(dev)

        def store_path():
            frame[0] += 1
            store.add_scans("s", [frame[0]], [raw], steps=steps)
            store.release("s")

        for _ in range(args.warmup):
            kernel(); host_path(); store_path()
        torch.cuda.synchronize()
        ms = {"kernel": [], "host_transpose_only": [], "host_path": [], "store_add_scans": []}
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(args.rounds):
            a.record()
            for _ in range(args.reps):
                kernel()
            b.record()
            b.synchronize()
            ms["kernel"].append(a.elapsed_time(b) / args.reps)
            t0 = time.perf_counter()
            host_transpose()
            ms["host_transpose_only"].append((time.perf_counter() - t0) * 1e3)
            ms["host_path"].append(_wall(host_path))
            ms["store_add_scans"].append(_wall(store_path))
        row = {"case": name, "N": N_SCAN, "row_floats": 4, "kernel_equals_numpy_bitwise": same}
        row.update({k: _stats(v) for k, v in ms.items()})
        moved = N_SCAN * (4 + 3) * 4                              # bytes the kernel reads and writes
        row["kernel_GBps"] = round(moved / (row["kernel"]["median_ms"] * 1e-3) / 1e9, 1)
        rows.append(row)
    return rows


def _tracker(dev):
    from ptt_amd.config import StubDataset, ptt_model_cfg
    from ptt_amd.hot_path import randomize_
    from ptt_amd.models import build_network
    tracker = randomize_(build_network(ptt_model_cfg(), 1, StubDataset()), seed=2).to(dev).eval()
    with torch.no_grad():                                       # small regression outputs: the boxes stay on their objects
        tracker.box_voting_head.refine_layer[-1].conv.weight.mul_(0.05)
        tracker.box_voting_head.refine_layer[-1].conv.bias.mul_(0.05)
    return tracker


def _targets(rs, n):
    yaw = rs.uniform(-np.pi, np.pi, n)
    centers = rs.uniform(-1, 1, (n, 3)) * np.array([35.0, 35.0, 0.2])
    return [(centers[k], np.array([1.7, 4.2, 1.5]), np.array([np.cos(yaw[k] / 2), 0.0, 0.0, np.sin(yaw[k] / 2)])) for k in range(n)]


def _scene_raws(rs, n_scans, n_points, boxes, affine=None):
    """Raw (N, 4) scans: background + 400 points on every box; with `affine`, expressed in the sensor frame it maps from."""
    raws = []
    for _ in range(n_scans):
        pts = _raw(rs, n_points)[:, :3].T.astype(np.float64)
        for k, (c, wlh, _) in enumerate(boxes):
            pts[:, k * 400:(k + 1) * 400] = rs.uniform(-0.5, 0.5, (3, 400)) * np.array([[wlh[1]], [wlh[0]], [wlh[2]]]) + c[:, None]
        if affine is not None:
            pts = affine[:3, :3].T @ (pts - affine[:3, 3:4])
        raws.append(np.ascontiguousarray(np.concatenate([pts.T, rs.uniform(0, 1, (n_points, 1))], 1).astype(np.float32)))
    return raws


def step_timing(dev, args, tracker):
    from ptt_amd.online_tracker import OnlineTracker
    rows = []
    for n_targets in (1, 8):
        for name, steps, affine in (("deinterleave", None, None), ("affine", [('affine', V2C)], V2C)):
            rs = np.random.RandomState(10 + n_targets)
            boxes = _targets(rs, n_targets)
            raws = _scene_raws(rs, 4, N_SCAN, boxes, affine)
            add = dict(enumerate(boxes))
            a = OnlineTracker(tracker, dev, slots=n_targets, scan_capacity=N_SCAN)
            b = OnlineTracker(tracker, dev, slots=n_targets, scan_capacity=N_SCAN)
            a.step_raw(raws[0], steps, add=add)
            b.step(_host_planar(raws[0], affine), add=add)
            for i in range(args.warmup):
                a.step_raw(raws[(i + 1) % 4], steps)
                b.step(_host_planar(raws[(i + 1) % 4], affine))
            ms = {"step_raw": [], "host_transpose_plus_step": []}
            for i in range(args.rounds):
                r = raws[(i + 2) % 4]
                t0 = time.perf_counter()
                a.step_raw(r, steps)
                ms["step_raw"].append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                b.step(_host_planar(r, affine))
                ms["host_transpose_plus_step"].append((time.perf_counter() - t0) * 1e3)
            row = {"targets": n_targets, "N": N_SCAN, "case": name}
            row.update({k: _stats(v) for k, v in ms.items()})
            rows.append(row)
            del a, b
            torch.cuda.synchronize()
    return rows


def runner_timing(dev, args, tracker):
    from ptt_amd.packed_runner import PackedTrackletRunner
    from ptt_amd.scene_store import SceneStore
    n_scenes, n_scans, n_points, per_scene, length = 2, 10, 32768, 4, 6
    rs = np.random.RandomState(5)
    scenes = []
    for s in range(n_scenes):
        boxes = _targets(rs, per_scene)
        scenes.append((boxes, _scene_raws(rs, n_scans, n_points, boxes, V2C)))
    steps = [('affine', V2C)]
    spans = [(k, k % (n_scans - length + 1)) for k in range(per_scene)]           # tracklet k of a scene: `length` frames from there

    def store_tracklets():
        store = SceneStore(dev)
        for s, (boxes, raws) in enumerate(scenes):
            store.add_scans(s, range(n_scans), raws, steps=steps)
        return store, [store.tracklet(s, range(f0, f0 + length), [scenes[s][0][k]] * length) for s in range(n_scenes) for k, f0 in spans]

    planar = [[_host_planar(r, V2C) for r in raws] for _, raws in scenes]
    host_tracklets = [([planar[s][f] for f in range(f0, f0 + length)], [scenes[s][0][k]] * length) for s in range(n_scenes) for k, f0 in spans]
    pr = PackedTrackletRunner(tracker, dev, slots=4)
    store, shared = store_tracklets()
    got, want = pr.run(shared), pr.run(host_tracklets)
    same = all(np.array_equal(np.concatenate([np.ravel(v) for v in g[:3]]), np.concatenate([np.ravel(v) for v in w[:3]]))
               for gr, wr in zip(got, want) for g, w in zip(gr, wr))
    ms = {"store_ingest": [], "run_on_store_views": [], "run_on_host_arrays": []}
    for _ in range(max(2, args.rounds // 5)):
        del store, shared
        box = []
        ms["store_ingest"].append(_wall(lambda: box.append(store_tracklets())))
        store, shared = box[0]
        ms["run_on_store_views"].append(_wall(lambda: pr.run(shared)))
        ms["run_on_host_arrays"].append(_wall(lambda: pr.run(host_tracklets)))
    row = {"scenes": n_scenes, "scans_per_scene": n_scans, "points_per_scan": n_points, "tracklets": len(host_tracklets), "frames_per_tracklet": length,
           "slots": 4, "rows_equal_bitwise": bool(same),
           "bytes_uploaded_store": n_scenes * n_scans * n_points * 4 * 4,
           "bytes_uploaded_host_arrays": len(host_tracklets) * length * n_points * 3 * 4}
    row.update({k: _stats(v) for k, v in ms.items()})
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_store_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("scripts/scene_store_timing.py measures on the device; none is visible")
    dev = torch.device("cuda:0")
    tracker = _tracker(dev)
    out = {"what": "median / minimum of %d interleaved rounds after %d warm-ups, one process, one run on one machine; kernel: device events "
                   "around %d launches, per launch; everything else: host clock ended by a device synchronise" % (args.rounds, args.warmup, args.reps),
           "device": torch.cuda.get_device_name(0), "ingest": ingest_timing(dev, args), "step": step_timing(dev, args, tracker),
           "packed_runner": runner_timing(dev, args, tracker)}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
