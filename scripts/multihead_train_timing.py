"""Training-step timing of the tracker with MulTransformerBlock in both heads on one GPU: for (heads, layers) in
{(1,1), (2,1), (4,2), (8,1)} at 48 and at 8 frames (train_step.synthetic_train_batch), ms per step of
DataParallelTrainer.step — eager and captured (graph=True: replayed as one hipGraph after the warm-up steps). HIP events
around `--reps` steps, `--rounds` rounds with eager and graphed alternating, medians; one process, nothing else of ours
on the device.

    python scripts/multihead_train_timing.py [--reps 10] [--rounds 3] [--only 4,2] [--frames 48] [--json out.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/multihead_train_timing.py --trace-step     # one (4,2) step
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ptt_amd.config import StubDataset, ptt_model_cfg                             # noqa: E402
from ptt_amd.models import build_network                                          # noqa: E402
from ptt_amd.train_step import DataParallelTrainer, synthetic_train_batch         # noqa: E402

CONFIGS = ((1, 1), (2, 1), (4, 2), (8, 1))


def _trainer(dev, heads, layers, graph):
    cfg = ptt_model_cfg()
    for head in ("CENTROID_HEAD", "BOX_HEAD"):
        tb = cfg[head]["TRANSFORMER_BLOCK"]
        tb["NAME"], tb["N_HEADS"], tb["N_LAYERS"] = "MulTransformerBlock", heads, layers
    torch.manual_seed(1)
    model = build_network(cfg, 1, StubDataset(training=True)).to(dev).train()
    return DataParallelTrainer(model, dev, graph=graph)


def _time(tr, batch, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(reps):
        tr.step(batch)
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--only", default=None, help="heads,layers")
    ap.add_argument("--frames", default="48,8")
    ap.add_argument("--modes", default="eager,graph")
    ap.add_argument("--json", default=None)
    ap.add_argument("--trace-step", action="store_true", help="warm up, then run ONE eager (4,2) step at 48 frames (for a kernel trace)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.trace_step:
        tr = _trainer(dev, 4, 2, False)
        batch = synthetic_train_batch(100, 48, dev)
        for _ in range(3):
            tr.step(batch)
        torch.cuda.synchronize()
        print("traced step follows", flush=True)
        tr.step(batch)
        torch.cuda.synchronize()
        return
    configs = [tuple(int(v) for v in a.only.split(","))] if a.only else CONFIGS
    rows = []
    for B in [int(v) for v in a.frames.split(",")]:
        batch = synthetic_train_batch(100, B, dev)
        for heads, layers in configs:
            trainers = {m: _trainer(dev, heads, layers, m == "graph") for m in a.modes.split(",")}
            for tr in trainers.values():
                for _ in range(a.warmup):
                    tr.step(batch)
            assert "graph" not in trainers or trainers["graph"].captured is not None, "the step was not captured"
            t = {m: [] for m in trainers}
            for _ in range(a.rounds):
                for name, tr in trainers.items():
                    t[name].append(_time(tr, batch, a.reps))
            r = dict(frames=B, heads=heads, layers=layers)
            for m in trainers:
                r[m + "_ms"] = round(float(np.median(t[m])), 3)
                r[m + "_runs"] = [round(v, 3) for v in t[m]]
            rows.append(r)
            print(json.dumps(r), flush=True)
            del trainers
            torch.cuda.empty_cache()
    if a.json:
        json.dump(rows, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
