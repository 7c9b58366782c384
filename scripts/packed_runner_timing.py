"""Evaluating tracklets of very uneven lengths: PackedTrackletRunner against the lockstep runner -> profiles/packed_runner_timing.json
(and the same JSON line on stdout).

    python scripts/packed_runner_timing.py [--repeats 3] [--out profiles/packed_runner_timing.json]

The workload is SYNTHETIC (no dataset is read): 120 tracklets of ptt_amd.synth.tracklet(1000 + k, length) whose lengths are
np.random.RandomState(0).geometric(1 / 50., 120) clipped to [2, 600], the longest set to 600 — a few frames to several hundred, as
tracking datasets have them. Every variant gets the tracklets as host arrays, so a run includes its uploads.

Variants, in ONE process: TrackletRunner(batch=48).run in input order (the baseline: the lockstep runner, which is not the code under
test), run_overlapped with two 48-wide runners, PackedTrackletRunner(slots=48) in both orders, and the same with drain_slots=8. Every
variant runs once as a warm-up (graph captures, weight packing), then `--repeats` rounds in which the variants ALTERNATE; a host
clock around each run, which ends in a device synchronise. Reported per variant: median / minimum / maximum wall time, tracked
frames per second at the median, steps, the live fraction of its slot-steps, and for the drain runs the largest centre distance of a
migrated tracklet's rows from the no-drain rows (recorded, not judged). The no-drain packed rows must equal the lockstep rows bit
for bit, or the script fails. Without a device this raises after the schedule counts are made: there is no CPU figure to give.
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
from ptt_amd import synth                                       # noqa: E402
from ptt_amd.packed_runner import PackedPlan, PackedTrackletRunner     # noqa: E402


TRACKLETS, LONGEST, SLOTS, DRAIN_SLOTS = 120, 600, 48, 8         # the workload is fixed: the committed numbers belong to it


def workload_lengths(n, longest):
    lengths = np.clip(np.random.RandomState(0).geometric(1 / 50., n), 2, longest)
    lengths[int(np.argmax(lengths))] = longest
    return [int(v) for v in lengths]


def lockstep_counts(lengths, batch, runners=1):
    """Steps and slot-steps of TrackletRunner.run (runners = 1) / run_overlapped: groups of `batch` in input order, max(length) - 1
    steps each; overlapped runners take the groups in turn and advance alternately, so the longer queue decides the step rounds."""
    groups = [max(lengths[g:g + batch]) - 1 for g in range(0, len(lengths), batch)]
    rounds = max(sum(groups[r::runners]) for r in range(runners))
    return dict(steps=sum(groups), step_rounds=rounds, slot_steps=sum(groups) * batch, live_slot_steps=sum(n - 1 for n in lengths))


def _same_rows(a, b):
    """Two result lists (per tracklet, per frame, (center, wlh, quat[, score])) hold the same bits."""
    return len(a) == len(b) and all(
        len(rows) == len(want) and all(len(r) == len(w) and all(np.array_equal(u, v) for u, v in zip(r, w)) for r, w in zip(rows, want))
        for rows, want in zip(a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed_runner_timing.json"))
    args = ap.parse_args()
    S, K = SLOTS, DRAIN_SLOTS
    lengths = workload_lengths(TRACKLETS, LONGEST)
    frames = sum(n - 1 for n in lengths)
    packed = {"packed_%s%s" % (order, "_drain%d" % K if drain else ""): dict(order=order, drain_slots=drain)
              for drain in (None, K) for order in ("input", "longest_first")}
    counts = {"lockstep": lockstep_counts(lengths, S), "overlapped_2": lockstep_counts(lengths, S, 2)}
    for name, kw in packed.items():
        plan = PackedPlan(lengths, S, **kw)
        counts[name] = dict(steps=plan.n_steps, slot_steps=plan.slot_steps, live_slot_steps=plan.live_slot_steps,
                            migration_step=plan.migration_step, migrated=plan.migrated)
    if not torch.cuda.is_available():
        raise RuntimeError("scripts/packed_runner_timing.py measures on the device; none is visible (schedule counts: %s)" % json.dumps(counts))
    dev = torch.device("cuda:0")

    from ptt_amd.config import StubDataset, ptt_model_cfg
    from ptt_amd.hot_path import randomize_
    from ptt_amd.models import build_network
    from ptt_amd.tracklet_runner import TrackletRunner, run_overlapped
    tracker = randomize_(build_network(ptt_model_cfg(), 1, StubDataset()), seed=2).to(dev).eval()
    with torch.no_grad():                                       # small regression outputs: the boxes stay on their objects
        tracker.box_voting_head.refine_layer[-1].conv.weight.mul_(0.05)
        tracker.box_voting_head.refine_layer[-1].conv.bias.mul_(0.05)
    tracklets = [synth.tracklet(1000 + k, n) for k, n in enumerate(lengths)]

    lock = TrackletRunner(tracker, dev, batch=S)
    pair = [TrackletRunner(tracker, dev, batch=S) for _ in range(2)]
    runs = {"lockstep": lambda: lock.run(tracklets), "overlapped_2": lambda: run_overlapped(pair, tracklets)}
    runners = {}
    for name, kw in packed.items():
        runners[name] = PackedTrackletRunner(tracker, dev, slots=S, **kw)
        runs[name] = (lambda r: lambda: r.run(tracklets))(runners[name])

    rows = {}
    for name, fn in runs.items():                               # warm-up: one whole run of every variant
        rows[name] = fn()
        torch.cuda.synchronize()
        print("warm-up", name, "done", file=sys.stderr, flush=True)
    for name in ("packed_input", "packed_longest_first"):
        if not _same_rows(rows[name], rows["lockstep"]):
            raise RuntimeError("%s does not give the lockstep runner's rows bit for bit" % name)
    for name, r in runners.items():
        st, c = r.stats, counts[name]
        assert (st["steps"], st["slot_steps"], st["live_slot_steps"], st["migrated"]) == (c["steps"], c["slot_steps"], c["live_slot_steps"], c["migrated"])
    drift = {}
    for name, r in runners.items():
        if r.drain_slots is None:
            continue
        base = rows["packed_%s" % r.order]
        moved = [t for _, _, t in r.plan.steps[r.plan.migration_step].migrate]
        drift[name] = max(float(np.linalg.norm(a[0] - b[0])) for t in moved for a, b in zip(rows[name][t], base[t]))
        others = [t for t in range(len(lengths)) if t not in moved]
        if not _same_rows([rows[name][t] for t in others], [base[t] for t in others]):
            raise RuntimeError("%s changed a tracklet that never migrated" % name)

    sec = {name: [] for name in runs}
    for _ in range(args.repeats):
        for name, fn in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            sec[name].append(time.perf_counter() - t0)
        print("round done", file=sys.stderr, flush=True)

    table = []
    for name in runs:
        med = float(np.median(sec[name]))
        c = counts[name]
        row = dict(variant=name, median_s=round(med, 4), min_s=round(min(sec[name]), 4), max_s=round(max(sec[name]), 4),
                   frames_per_s=round(frames / med, 1), steps=c["steps"], slot_steps=c["slot_steps"],
                   live_fraction=round(c["live_slot_steps"] / float(c["slot_steps"]), 4))
        if name == "overlapped_2":
            row["step_rounds"] = c["step_rounds"]
        if name in drift:
            row.update(migration_step=c["migration_step"], migrated=c["migrated"], max_centre_distance_to_no_drain_m=drift[name])
        table.append(row)
    base = table[0]
    for row in table:
        row["speedup_over_lockstep"] = round(base["median_s"] / row["median_s"], 3)
    out = {"what": "SYNTHETIC workload: %d tracklets of synth.tracklet(1000 + k, length), lengths geometric(1/50) clipped to [2, %d], "
                   "longest set to %d; one process, one warm-up run of every variant, then %d rounds in which the variants alternate; host "
                   "clock around a whole run (uploads included, ends in a device synchronise); median / min / max seconds"
                   % (len(lengths), LONGEST, LONGEST, args.repeats),
           "device": torch.cuda.get_device_name(0), "slots": S, "drain_slots": K, "lengths": lengths, "lengths_sum": int(sum(lengths)),
           "tracked_frames": frames, "runs": table}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
