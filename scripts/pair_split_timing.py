"""TransformerBlock.precision 'fp32' against 'bf16x2' on one GPU, alternated in one process (random weights and inputs: the
clock under bf16-MFMA load depends on the data).

  * the eval-mode block with want_attn=False at B = 48, N = 128 for all nine (DIM_MODEL, KNN): HIP-event time of the whole block
    (kNN, q|k|v projection, pair kernel, fc2 + residual) and of the pair kernel's launch alone (ops.start_kernel_timing);
  * the stress-cloud size, one cloud of N = 2048 at (512, 16);
  * the full tracker forward at B = 48 as a graph replay (GraphedHotPath over TrackerThroughput), switched with
    ptt_amd.precision.set_precision.
Median of the rounds per arm, with each arm's min and max kept. `faster` = the fp32 median exceeds the bf16x2 median by more
than the fp32 arm's own min-max spread — the rule by which a (DIM_MODEL, KNN) stays in variants.SPLIT_DISPATCH. Every pair is
measured on the split kernel whatever SPLIT_DISPATCH holds.

    python scripts/pair_split_timing.py [--reps 20] [--rounds 5] [--out profiles/pair_split_timing.json]
"""
import argparse
import json
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ptt_amd import ops, synth                                                     # noqa: E402
from ptt_amd.models.transformer_block import variants as V                         # noqa: E402
from ptt_amd.precision import set_precision                                        # noqa: E402
from tests.util import fill_state_dict_                                            # noqa: E402

PEAK = 157.3
KERNELS = {"fp32": "ptt_pt_attn_pair_f32", "bf16x2": "ptt_pt_attn_pair_split_f32"}
ARMS = ("fp32", "bf16x2")


def _time(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    fn()
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def _kernel_time(fn, name, reps):
    fn()
    ops.start_kernel_timing([name])
    for _ in range(reps):
        fn()
    t = ops.stop_kernel_timing()[name]
    assert len(t) == reps, "%s ran %d times in %d calls" % (name, len(t), reps)
    return float(np.median(t))


def _arm(ts):
    return dict(median_ms=round(float(np.median(ts)), 4), min_ms=round(float(min(ts)), 4), max_ms=round(float(max(ts)), 4))


def _verdict(a):
    spread = a["fp32"]["max_ms"] - a["fp32"]["min_ms"]
    gain = a["fp32"]["median_ms"] - a["bf16x2"]["median_ms"]
    return dict(speedup=round(a["fp32"]["median_ms"] / a["bf16x2"]["median_ms"], 3), fp32_spread_ms=round(spread, 4),
                faster=bool(gain > spread))


def block_case(B, N, D, k, dev, reps, rounds):
    xyz = torch.from_numpy(synth.frames(7 + N, B, N, 64, K_s=N)[0]).to(dev)
    feat = torch.from_numpy(np.random.RandomState(N).standard_normal((B, N, 256)).astype(np.float32)).to(dev)
    blocks = {}
    for arm in ARMS:
        blocks[arm] = fill_state_dict_(V.TransformerBlock(256, D, k), 11).to(dev).eval()
        blocks[arm].precision = arm
    ops.unfused_calls.clear()
    ops.precision_fallbacks.clear()
    block_t, kern_t = {a: [] for a in ARMS}, {a: [] for a in ARMS}
    with torch.no_grad():
        for _ in range(rounds):                                # alternate the two arithmetics
            for arm in ARMS:
                fn = lambda: blocks[arm](xyz, feat, want_attn=False)
                block_t[arm].append(_time(fn, reps))
                kern_t[arm].append(_kernel_time(fn, KERNELS[arm], reps))
    assert not ops.unfused_calls and not ops.precision_fallbacks, (ops.unfused_calls, ops.precision_fallbacks)
    flops = B * N * k * 2.0 * (3 * D + 3 * D * D)
    blk = {a: _arm(block_t[a]) for a in ARMS}
    ker = {a: _arm(kern_t[a]) for a in ARMS}
    for a in ARMS:
        ker[a]["tflops"] = round(flops / ker[a]["median_ms"] / 1e9, 1)
    return dict(B=B, N=N, D=D, k=k, pair_gflop=round(flops / 1e9, 3), block=dict(blk, **_verdict(blk)), kernel=dict(ker, **_verdict(ker)))


def tracker_case(B, dev, reps, rounds):
    from ptt_amd.config import StubDataset, ptt_model_cfg
    from ptt_amd.hot_path import GraphedHotPath, TrackerThroughput, randomize_
    from ptt_amd.models import build_network
    tracker = randomize_(build_network(ptt_model_cfg(), 1, StubDataset()), seed=4).to(dev).eval()
    s, t = (torch.from_numpy(a).to(dev) for a in synth.frames(300, B, 1024, 512))
    g = GraphedHotPath(TrackerThroughput(tracker), s, t)
    ts = {a: [] for a in ARMS}
    blocks = 0
    for _ in range(rounds):
        for arm in ARMS:
            blocks = set_precision(tracker, arm)               # the next call captures again
            ts[arm].append(_time(lambda: g(), reps))
    set_precision(tracker, "fp32")
    a = {arm: _arm(ts[arm]) for arm in ARMS}
    return dict(B=B, transformer_blocks=blocks, fallbacks={"%s: %s" % k: v for k, v in ops.precision_fallbacks.items()},
                **a, **_verdict(a))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-tracker", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_split_timing.json"))
    a = ap.parse_args()
    warnings.simplefilter("ignore")
    dev = torch.device("cuda:0")
    dispatched = sorted(V.SPLIT_DISPATCH)
    out = dict(device=torch.cuda.get_device_name(0), reps=a.reps, rounds=a.rounds, peak_fp32_tflops=PEAK, split_dispatch=dispatched,
               block=[], stress=None, tracker=None)
    try:
        out["build"] = open(os.path.join(ROOT, "ptt_amd", "lib", "BUILD_ID")).read().strip()
    except OSError:
        pass
    if not a.skip_tracker:                                     # as the library dispatches it
        out["tracker"] = tracker_case(48, dev, a.reps, a.rounds)
        print(json.dumps(out["tracker"]), flush=True)
    V.SPLIT_DISPATCH = frozenset((D, k) for D in V.FUSED_D_MODEL for k in V.FUSED_KNN)      # every pair on the split kernel
    for D in (128, 256, 512):
        for k in (8, 16, 32):
            r = block_case(48, 128, D, k, dev, a.reps, a.rounds)
            out["block"].append(r)
            print(json.dumps(r), flush=True)
    out["stress"] = block_case(1, 2048, 512, 16, dev, a.reps, a.rounds)
    print(json.dumps(out["stress"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
