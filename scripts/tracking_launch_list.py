"""Dev tool: the device work of the three tracking drivers on a fixed tiny scenario, as JSON — per scenario the ordered kernel names
and the number of memcpy events that torch.profiler records for a run AFTER the first (the steps after the warm-up for
OnlineTracker). Run it on two trees and compare the output (docs/experiments.md, "One step core"): a refactor of the drivers must
not change it. Every scenario is recorded three times: the profiler now and then loses a few kernel records of a graph replay
(identical runs of one tree then differ by 1 - 3 kernels), so the recording with the most kernels is printed, with all three counts.

    python scripts/tracking_launch_list.py [--out launches.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
from torch.profiler import ProfilerActivity, profile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ptt_amd import synth                                       # noqa: E402


def recorded(dev, fn, prepare=None):
    takes = []
    for _ in range(3):
        if prepare is not None:
            prepare()
        takes.append(_recorded(dev, fn))
    best = max(takes, key=lambda t: t["n_kernels"])
    best["n_kernels_of_each_recording"] = [t["n_kernels"] for t in takes]
    return best


def _recorded(dev, fn):
    torch.cuda.synchronize(dev)
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize(dev)
    events = sorted((e for e in prof.profiler.kineto_results.events() if e.device_type() == torch.autograd.DeviceType.CUDA),
                    key=lambda e: e.start_ns())
    copies = [e.name() for e in events if e.name().lower().startswith(("memcpy", "memset"))]
    kernels = [e for e in events if not e.name().lower().startswith(("memcpy", "memset"))]
    # a model graph has parallel branches: kernels of different streams overlap, and their order by start time is not fixed from one
    # process to the next. Per stream it is: `streams` holds each stream's kernels in order, the streams by their first kernel
    streams = {}
    for e in kernels:
        streams.setdefault(e.device_resource_id(), []).append(e.name())
    return {"kernels": [e.name() for e in kernels], "streams": list(streams.values()), "n_kernels": len(kernels),
            "n_memcpy": sum(c.lower().startswith("memcpy") for c in copies), "n_memset": sum(c.lower().startswith("memset") for c in copies)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    from ptt_amd.config import StubDataset, ptt_model_cfg
    from ptt_amd.hot_path import randomize_
    from ptt_amd.models import build_network
    from ptt_amd.online_tracker import OnlineTracker
    from ptt_amd.packed_runner import PackedTrackletRunner
    from ptt_amd.tracklet_runner import TrackletRunner
    tracker = randomize_(build_network(ptt_model_cfg(), 1, StubDataset()), seed=2).to(dev).eval()
    with torch.no_grad():                                       # small regression outputs: the boxes stay on their objects
        tracker.box_voting_head.refine_layer[-1].conv.weight.mul_(0.05)
        tracker.box_voting_head.refine_layer[-1].conv.bias.mul_(0.05)
    out = {}
    pair = [synth.tracklet(700 + k, n) for k, n in enumerate([4, 3])]
    for batch in (1, 6):
        runner = TrackletRunner(tracker, dev, batch=batch)
        runner.run(pair)
        out["lockstep_b%d" % batch] = recorded(dev, lambda: runner.run(pair))
    five = [synth.tracklet(710 + k, n) for k, n in enumerate([1, 2, 4, 7, 3])]
    pr = PackedTrackletRunner(tracker, dev, slots=2)
    pr.run(five)
    out["packed_s2"] = recorded(dev, lambda: pr.run(five))
    clouds, boxes = synth.tracklet(720, 5)
    clouds = [np.ascontiguousarray(c, np.float32) for c in clouds]
    ot = OnlineTracker(tracker, dev, slots=2, scan_capacity=16384)

    def warm_up():                                              # the model graph is captured in the first tracked step
        ot.reset()
        ot.step(clouds[0], add={"A": boxes[0]})
        ot.step(clouds[1])

    def online():
        ot.step(clouds[2])
        ot.step(clouds[3], add={"B": boxes[3]})
        ot.step(clouds[4])
    out["online_s2"] = recorded(dev, online, warm_up)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
