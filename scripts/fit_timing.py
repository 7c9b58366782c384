#!/usr/bin/env python
"""What fit() costs around the captured training step, at BASELINE.json configs[3]'s shape (B = 48, 1024 search + 512 template
points, synthetic tracklets) -> profiles/fit_timing.json (or --out).

Three ways to take the same step, alternating in one process, --reps repetitions of --steps steps each:
  (a) resident   DataParallelTrainer.step on ONE resident batch, the step replayed as a hipGraph (what bench.py's train line times)
  (b) fed        the same step on batches a TrainBatchFeeder makes, ledger=None
  (c) fit        ptt_amd.fit.fit with a StepLedger: the append inside the graph, the ring fetched every --log-interval steps,
                 scalars handed to a logger that keeps them; no checkpoint is written inside the timed window
ms per step is a host clock around the steps ending in a device synchronise. Medians and the min..max spread over the repetitions
are reported. `host_ms_per_step` is the same clock stopped BEFORE the synchronise: over 100 steps it includes the waits that keep the
host from running ahead without bound (the optimizer's 64-slot hyper-parameter ring, the feeder's `depth` staging buffers, fit's
fetch), so it says how far the host is throttled, not what queuing a step costs. That cost is `issue_ms_per_step`: --burst steps
right after a synchronise, short enough to meet none of those waits (the feeder of the burst has depth = burst + 8), for (a), for
(b) and for (b) with the ledger's append in the graph.

    python scripts/fit_timing.py [--steps 100] [--reps 5] [--out profiles/fit_timing.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class _KeepScalars(object):
    def __init__(self):
        self.n = 0

    def add_scalar(self, name, value, it):
        self.n += 1


def _commit():
    try:
        return subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, stderr=subprocess.DEVNULL).decode().strip()
    except (OSError, subprocess.CalledProcessError):
        build_id = os.path.join(ROOT, "ptt_amd", "lib", "BUILD_ID")
        return open(build_id).read().strip() if os.path.exists(build_id) else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=48)
    ap.add_argument("--log-interval", type=int, default=100)
    ap.add_argument("--burst", type=int, default=32, help="steps of the host-issue measurement (below the optimizer ring's 64 slots)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fit_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fit_timing.py measures on a HIP device; none is visible")

    from ptt_amd import _lib, synth
    from ptt_amd.config import StubDataset, ptt_model_cfg
    from ptt_amd.fit import StepLedger, fit
    from ptt_amd.models import build_network
    from ptt_amd.train_feed import TrainBatchFeeder
    from ptt_amd.train_step import DataParallelTrainer, synthetic_train_batch

    dev = torch.device("cuda:0")
    B, steps = args.batch, args.steps
    # 4 candidates per frame: frames * 4 / B batches per epoch >= steps
    n_frames = -(-steps * B // 4)
    per = 40
    tracklets = [synth.tracklet(seed, per, n_obj=(100, 300), n_bg=(300, 800)) for seed in range(-(-n_frames // per))]

    def trainer(ledger=None):
        torch.manual_seed(1)
        model = build_network(ptt_model_cfg(), 1, StubDataset(training=True)).to(dev).train()
        return DataParallelTrainer(model, dev, graph=True, ledger=ledger)

    def feeder(**kw):
        f = TrainBatchFeeder(tracklets, dev, batch_size=B, seed=3, **kw)
        assert len(f) >= steps, (len(f), steps)
        return f

    class _Head(object):
        """The first `steps` batches of a feeder's epoch."""

        def __init__(self, f):
            self.f = f

        def set_epoch(self, e):
            self.f.set_epoch(e)

        def __len__(self):
            return steps

        def __iter__(self):
            for k, b in zip(range(steps), self.f):
                yield b

    ta, tb, tc = trainer(), trainer(), trainer(StepLedger(dev))
    resident = synthetic_train_batch(100, B, dev)
    fb, fc = _Head(feeder()), _Head(feeder())
    log = _KeepScalars()
    ckpt_dir = tempfile.mkdtemp()
    epoch = [0, 0]

    def run_a():
        t0 = time.perf_counter()
        for _ in range(steps):
            ta.step(resident)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        return t1 - t0, time.perf_counter() - t0

    def run_b():
        fb.set_epoch(epoch[0])
        epoch[0] += 1
        t0 = time.perf_counter()
        for batch in fb:
            tb.step(batch)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        return t1 - t0, time.perf_counter() - t0

    def run_c():
        e = epoch[1]
        epoch[1] += 1
        t0 = time.perf_counter()
        fit(tc, fc, e + 1, ckpt_dir, start_epoch=e, start_iter=tc.iteration, ckpt_save_interval=10 ** 9, tb_log=log,
            log_interval=args.log_interval)
        t1 = time.perf_counter()                               # fit() ends with a fetch: the device is idle here
        torch.cuda.synchronize()
        return t1 - t0, time.perf_counter() - t0

    runs = (("resident", run_a), ("fed", run_b), ("fit", run_c))
    for _, fn in runs:                                         # warm-up: eager steps, the capture, replays, every shape
        fn()
    assert ta.graph_steps > 0 and tb.graph_steps > 0 and tc.graph_steps > 0 and tc.captured.ledger
    deep = feeder(depth=args.burst + 8)

    def burst(trainer, fed):
        """Host ms per step to QUEUE --burst steps on an idle device."""
        deep.set_epoch(1000 + len(issue["resident"]) + len(issue["fed"]) + len(issue["fed_ledger"]))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if fed:
            for _, batch in zip(range(args.burst), deep):
                trainer.step(batch)
        else:
            for _ in range(args.burst):
                trainer.step(resident)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        return 1e3 * (t1 - t0) / args.burst

    issue = {"resident": [], "fed": [], "fed_ledger": []}
    times = {name: [] for name, _ in runs}
    for _ in range(args.reps):
        for name, fn in runs:
            times[name].append(fn())
        issue["resident"].append(burst(ta, False))
        issue["fed"].append(burst(tb, True))
        issue["fed_ledger"].append(burst(tc, True))
    out = {"commit": _commit(), "abi": _lib.ABI_VERSION, "device": torch.cuda.get_device_name(0), "batch": B, "search_points": 1024,
           "template_points": 512, "steps_per_rep": steps, "reps": args.reps, "log_interval": args.log_interval,
           "scalars_logged": log.n}
    for name, _ in runs:
        ms = [1e3 * total / steps for _, total in times[name]]
        host = [1e3 * h / steps for h, _ in times[name]]
        out[name] = {"ms_per_step_median": statistics.median(ms), "ms_per_step_min": min(ms), "ms_per_step_max": max(ms),
                     "ms_per_step": ms, "host_ms_per_step_median": statistics.median(host), "host_ms_per_step": host}
    out["issue_ms_per_step"] = {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in issue.items()}
    out["burst_steps"] = args.burst
    out["fit"]["note"] = "host time includes the ledger fetches (each waits for the device) and the logger calls"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"ms_per_step": {n: [out[n]["ms_per_step_median"], out[n]["ms_per_step_min"], out[n]["ms_per_step_max"]] for n, _ in runs},
                      "host_ms_per_step": {n: out[n]["host_ms_per_step_median"] for n, _ in runs}, "issue_ms_per_step": out["issue_ms_per_step"]}))


if __name__ == "__main__":
    main()
