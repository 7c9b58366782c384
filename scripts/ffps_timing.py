"""Timing of feature-space furthest point sampling (ptt_ffps_f32) on the device -> ONE JSON line.

    python scripts/ffps_timing.py [--batch 48] [--rounds 30] [--out profiles/<name>.json]

Per launch, B = 48 clouds, device events around each launch, warm-ups first, the median (and the minimum) of `rounds`
launches, ptt_ffps_f32 and ptt_fps_f32 of the same (N, npoint) alternating in the same loop — the coordinate op is the yardstick:
it runs the same serial chain of npoint - 1 iterations with the cloud in registers, where the feature op streams N x (C + 3)
values from L2 per iteration. Then the eval-mode tracker forward (eager launches under torch.no_grad, device events around the
whole forward) at batch x (1024 + 512) points with SAMPLE_METHOD ['fps', 'ffps', 'ffps'] + the box head's 'ffps' against the
shipped ['fps', 'sequence', 'sequence'] + 'fps', alternating. Without a device this raises: there is no CPU figure to give.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ptt_amd import ops, synth                                  # noqa: E402

SHAPES = [(512, 128, 256), (256, 256, 128), (256, 128, 128), (128, 256, 64), (128, 257, 64)]       # (N, C, npoint)


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(np.min(ms)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("scripts/ffps_timing.py measures on the device; none is visible")
    dev = torch.device("cuda:0")
    B = args.batch
    out = {"what": "ptt_ffps_f32 per launch vs ptt_fps_f32, device events, median of %d after %d warm-ups" % (args.rounds, args.warmup),
           "device": torch.cuda.get_device_name(0), "batch": B, "ops": []}
    rs = np.random.RandomState(0)
    for N, C, npoint in SHAPES:
        xyz = torch.from_numpy(np.stack([synth.cloud(rs, N, N, synth.SEARCH_BOX, synth.CAR_SIGMA, 0.7) for _ in range(B)]).astype(np.float32)).to(dev)
        rows = torch.from_numpy(rs.standard_normal((B, N, C)).astype(np.float32)).to(dev)      # point-major, as the fused path keeps them
        bcn = rows.transpose(1, 2).contiguous()
        runs = {"ffps_bcn": lambda: ops.feature_fps(xyz, bcn, npoint),
                "ffps_point_major": lambda: ops.feature_fps(xyz, rows.transpose(1, 2), npoint),
                "fps": lambda: ops.furthest_point_sampling(xyz, npoint)}
        assert torch.equal(runs["ffps_bcn"](), runs["ffps_point_major"]())
        for _ in range(args.warmup):
            for fn in runs.values():
                fn()
        ms = {k: [] for k in runs}
        for _ in range(args.rounds):
            for k, fn in runs.items():
                ms[k].append(_timed(fn))
        row = {"N": N, "C": C, "npoint": npoint}
        for k in runs:
            row[k] = _stats(ms[k])
        row["us_per_iteration_ffps_bcn"] = round(1e3 * row["ffps_bcn"]["median_ms"] / max(npoint - 1, 1), 3)
        row["us_per_iteration_fps"] = round(1e3 * row["fps"]["median_ms"] / max(npoint - 1, 1), 3)
        row["ratio_ffps_bcn_over_fps"] = round(row["ffps_bcn"]["median_ms"] / row["fps"]["median_ms"], 2)
        row["ratio_ffps_point_major_over_fps"] = round(row["ffps_point_major"]["median_ms"] / row["fps"]["median_ms"], 2)
        out["ops"].append(row)

    # the tracker forward, eval mode
    from ptt_amd.config import StubDataset, ptt_model_cfg
    from ptt_amd.hot_path import randomize_
    from ptt_amd.models import build_network
    models = {}
    for name in ("shipped", "ffps"):
        cfg = ptt_model_cfg()
        if name == "ffps":
            cfg.BACKBONE_3D.SA_CONFIG.SAMPLE_METHOD = ['fps', 'ffps', 'ffps']
            cfg.BOX_HEAD.SA_CONFIG.SAMPLE_METHOD = 'ffps'
        models[name] = randomize_(build_network(cfg, 1, StubDataset()), seed=2).to(dev).eval()
    s, t = (torch.from_numpy(a).to(dev) for a in synth.frames(7, B, 1024, 512))

    def forward(m):
        with torch.no_grad():
            return m({'search_points': s, 'template_points': t, 'batch_size': B})

    for _ in range(args.warmup):
        for m in models.values():
            forward(m)
    ms = {k: [] for k in models}
    for _ in range(args.rounds):
        for k, m in models.items():
            ms[k].append(_timed(lambda: forward(m)))
    out["tracker_forward"] = {"points": "%d x (1024 + 512)" % B, "mode": "eval, eager launches, device events around the forward",
                              "shipped_fps_sequence_sequence": _stats(ms["shipped"]), "fps_ffps_ffps_box_ffps": _stats(ms["ffps"])}
    out["tracker_forward"]["ratio"] = round(out["tracker_forward"]["fps_ffps_ffps_box_ffps"]["median_ms"]
                                            / out["tracker_forward"]["shipped_fps_sequence_sequence"]["median_ms"], 3)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
