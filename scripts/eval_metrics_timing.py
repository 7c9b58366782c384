"""Host time of ptt_amd.eval_metrics.evaluate over a dataset-sized list of frames against the float64 numpy checker
(tests/box_overlap_ref.py) on the same host, and the device time of the one launch. For docs/experiments.md; informational.

    python scripts/eval_metrics_timing.py [--frames 6424] [--tracklets 120] [--out FILE.json]
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

from ptt_amd import eval_metrics as E, ops          # noqa: E402
from tests import box_overlap_ref as R              # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=6424)           # KITTI Car's test frames
    ap.add_argument("--tracklets", type=int, default=120)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gt, pred = R.random_pairs(5, args.frames, "lidar")
    cuts = np.linspace(0, args.frames, args.tracklets + 1).astype(int)
    box = lambda r: (r[0:3], r[3:6], r[6:10])
    tracklets = [(None, [box(r) for r in gt[a:b]]) for a, b in zip(cuts[:-1], cuts[1:])]
    results = [[box(r) for r in pred[a:b]] for a, b in zip(cuts[:-1], cuts[1:])]

    E.evaluate(results, tracklets)                                # loads the library, warms the allocator
    torch.cuda.synchronize()
    host = []
    for _ in range(5):
        t = time.perf_counter()
        out = E.evaluate(results, tracklets)
        host.append((time.perf_counter() - t) * 1e3)
    g, p = torch.from_numpy(gt).to(dev), torch.from_numpy(pred).to(dev)
    buf = torch.empty((2, args.frames), dtype=torch.float64, device=dev)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(20)]
    for a, b in ev:
        a.record()
        ops.box_overlap(g, p, "lidar", 3, out=buf)
        b.record()
    torch.cuda.synchronize()
    kernel = sorted(a.elapsed_time(b) * 1e3 for a, b in ev[5:])

    t = time.perf_counter()
    ov, acc = R.overlaps(gt, pred, "lidar", 3)
    s, pr = R.Success(), R.Precision()
    for v in ov:
        s.add_overlap(v)
    for v in acc:
        pr.add_accuracy(v)
    ref = (s.average, pr.average)
    checker = (time.perf_counter() - t) * 1e3
    line = {"frames": args.frames, "tracklets": args.tracklets, "evaluate_host_ms_median": float(np.median(host)),
            "evaluate_host_ms_min": float(min(host)), "launch_device_us_median": float(np.median(kernel)),
            "launch_device_us_min": float(kernel[0]), "numpy_checker_ms": checker, "success": out["success"],
            "precision": out["precision"], "checker_success": float(ref[0]), "checker_precision": float(ref[1]),
            "worst_overlap_diff": float(np.abs(out["overlap"] - ov).max()), "device": torch.cuda.get_device_name(0)}
    print(json.dumps(line))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
