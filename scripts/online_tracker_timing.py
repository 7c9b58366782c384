"""Timing of the live-scan path on the device -> profiles/online_tracker_timing.json (and the same JSON line on stdout).

    python scripts/online_tracker_timing.py [--rounds 30] [--out profiles/online_tracker_timing.json]

1. Crop: ptt_crop_scan_f32 (every job spread over chunks of its cloud) against ptt_crop_compact_f32 (one workgroup per job) on the
   SAME device job tables: N = 32768 and 131072 points per scan, 2 / 16 / 96 jobs (even jobs on one scan, odd jobs on another, as a
   step lays them out), yawed boxes that keep about 1 % of the points. Device events around `--reps` back-to-back launches (one
   launch is tens of microseconds: a single one would time the events), the two kernels alternating in the same loop, warm-ups
   first, median and minimum of `--rounds` such windows. The outputs are compared once before anything is timed.
   `scan_crop_min_points` = the smallest measured N from which (it and every larger measured N) the chunked kernel is not slower
   at 2 jobs, null if there is none: what ptt_amd.online_tracker.SCAN_CROP_MIN_POINTS is set from.
2. Step: milliseconds per OnlineTracker.step (a host clock around the call, which ends in a device synchronise) at 1 / 8 / 48 live
   targets (slots = targets) on scans of 131072 points, with the scan already on the device and from pinned host memory, chunked
   and one-workgroup crop — four trackers per target count stepping alternately on the same scans.
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

EXTENT = np.array([50.0, 50.0, 2.0])                            # the scan fills +-50 m x +-50 m x +-2 m
WLH = np.array([6.4, 10.0, 4.0])                                # x 1.25: 12.5 m x 8 m of 100 m x 100 m = 1 % of the points


def _stats(ms):
    return {"median_ms": round(float(np.median(ms)), 5), "min_ms": round(float(np.min(ms)), 5)}


def _scan(rs, n):
    return np.ascontiguousarray((rs.uniform(-1, 1, (3, n)) * EXTENT[:, None]).astype(np.float32))


def _boxes(rs, n):
    boxes = np.zeros(n, ops.TRACK_BOX)
    yaw = rs.uniform(-np.pi, np.pi, n)
    boxes['center'] = rs.uniform(-1, 1, (n, 3)) * np.array([35.0, 35.0, 0.2])
    boxes['wlh'] = WLH
    boxes['quat'][:, 0], boxes['quat'][:, 3] = np.cos(yaw / 2), np.sin(yaw / 2)
    return boxes


def crop_timing(dev, args):
    rows = []
    rs = np.random.RandomState(0)
    for N in (32768, 131072):
        scans = torch.from_numpy(np.stack([_scan(rs, N), _scan(rs, N)])).to(dev)
        for n_jobs in (2, 16, 96):
            jobs = np.zeros(n_jobs, ops.CROP_JOB)
            ops.track_crop_bounds(_boxes(rs, n_jobs), 0.0, 1.25, None, jobs)
            out = torch.zeros((2, n_jobs, N, 3), dtype=torch.float32, device=dev)
            cnt = torch.zeros((2, n_jobs), dtype=torch.int32, device=dev)
            jobs['points'] = scans.data_ptr() + (np.arange(n_jobs) % 2) * (3 * N * 4)
            jobs['ld'], jobs['n_points'], jobs['capacity'] = N, N, N
            tables = []
            for k in range(2):
                jobs['out'] = out[k].data_ptr() + np.arange(n_jobs) * (N * 3 * 4)
                jobs['count'] = cnt[k].data_ptr() + np.arange(n_jobs) * 4
                ops.crop_scan_check(jobs, n_jobs, N)
                tables.append(ops.upload_jobs(jobs))
            ws = ops._ws(ops.crop_scan_workspace(n_jobs, N), dev)
            runs = {"compact": lambda: ops.crop_compact(tables[0], n_jobs), "scan": lambda: ops.crop_scan_device(tables[1], n_jobs, N, ws)}
            for fn in runs.values():
                fn()
            torch.cuda.synchronize()
            assert torch.equal(cnt[0], cnt[1]) and torch.equal(out[0], out[1]), "the two crop kernels disagree"
            kept = float(cnt[0].float().mean()) / N
            for _ in range(args.warmup):
                for fn in runs.values():
                    fn()
            ms = {k: [] for k in runs}
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(args.rounds):
                for k, fn in runs.items():
                    a.record()
                    for _ in range(args.reps):
                        fn()
                    b.record()
                    b.synchronize()
                    ms[k].append(a.elapsed_time(b) / args.reps)
            row = {"N": N, "jobs": n_jobs, "kept_fraction": round(kept, 4), "compact": _stats(ms["compact"]), "scan": _stats(ms["scan"])}
            row["ratio_scan_over_compact"] = round(row["scan"]["median_ms"] / row["compact"]["median_ms"], 3)
            rows.append(row)
            del out, cnt, tables
    at2 = sorted((r["N"], r["ratio_scan_over_compact"] <= 1.0) for r in rows if r["jobs"] == 2)
    wins = None
    for k, (n, _) in enumerate(at2):
        if all(ok for _, ok in at2[k:]):
            wins = n
            break
    return rows, wins


def step_timing(dev, args):
    from ptt_amd.config import StubDataset, ptt_model_cfg
    from ptt_amd.hot_path import randomize_
    from ptt_amd.models import build_network
    from ptt_amd.online_tracker import OnlineTracker
    tracker = randomize_(build_network(ptt_model_cfg(), 1, StubDataset()), seed=2).to(dev).eval()
    with torch.no_grad():                                       # small regression outputs: the boxes stay on their objects
        tracker.box_voting_head.refine_layer[-1].conv.weight.mul_(0.05)
        tracker.box_voting_head.refine_layer[-1].conv.bias.mul_(0.05)
    N = 131072
    rows = []
    for n_targets in (1, 8, 48):
        rs = np.random.RandomState(n_targets)
        boxes = _boxes(rs, n_targets)
        boxes['wlh'] = (1.7, 4.2, 1.5)
        host = []
        for _ in range(4):                                      # four scans in rotation: background + 400 points on every target
            scan = _scan(rs, N)
            for k in range(n_targets):
                obj = rs.uniform(-0.5, 0.5, (3, 400)) * np.array([[4.2], [1.7], [1.5]]) + boxes['center'][k][:, None]
                scan[:, k * 400:(k + 1) * 400] = obj.astype(np.float32)
            host.append(torch.from_numpy(scan).pin_memory())
        device = [h.to(dev) for h in host]
        add = {k: (boxes['center'][k], boxes['wlh'][k], boxes['quat'][k]) for k in range(n_targets)}
        variants = {}
        for source, scans in (("device", device), ("pinned_host", host)):
            for chunked in (True, False):
                ot = OnlineTracker(tracker, dev, slots=n_targets, scan_capacity=N, scan_crop=chunked)
                ot.step(scans[0], add=add)
                variants[(source, chunked)] = (ot, scans)
        for i in range(args.warmup):
            for ot, scans in variants.values():
                ot.step(scans[(i + 1) % 4])
        ms = {k: [] for k in variants}
        for i in range(args.rounds):
            for k, (ot, scans) in variants.items():
                t0 = time.perf_counter()
                ot.step(scans[(i + 2) % 4])
                ms[k].append((time.perf_counter() - t0) * 1e3)
        for (source, chunked), v in ms.items():
            rows.append(dict(targets=n_targets, N=N, scan_from=source, crop="ptt_crop_scan_f32" if chunked else "ptt_crop_compact_f32", **_stats(v)))
        del variants, device, host
        torch.cuda.synchronize()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "online_tracker_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("scripts/online_tracker_timing.py measures on the device; none is visible")
    dev = torch.device("cuda:0")
    crop_rows, wins = crop_timing(dev, args)
    out = {"what": "median / minimum of %d interleaved rounds after %d warm-ups, one process; crop: device events around %d launches, "
                   "per launch; step: host clock around OnlineTracker.step (ends in a device synchronise)" % (args.rounds, args.warmup, args.reps),
           "device": torch.cuda.get_device_name(0), "chunk": ops.SCAN_CROP_CHUNK, "crop": crop_rows, "scan_crop_min_points": wins,
           "step": step_timing(dev, args)}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
