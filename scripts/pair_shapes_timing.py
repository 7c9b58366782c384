"""TransformerBlock timing over DIM_MODEL 128 / 256 / 512 x KNN 8 / 16 / 32 on one GPU, B = 48 and N = 128 / 64: HIP-event time
of the eval-mode block on the fused path (kNN, q|k|v projection, pair kernel, fc2 + residual) and on the stock torch path the same
module takes when `_fusable` says no (what every shape but (512, 16) ran before the instantiations existed), alternated in one
process, median of the rounds; algorithmic TFLOP/s of the fused block by SURVEY §8(d)'s count for the pair part,
2 (3 D + 3 D^2) per (point, neighbour) row, and the fraction of the 157.3 TFLOP/s fp32-MFMA peak. Then one training step (forward +
backward of a sum loss) at (256, 8) and (512, 32) on the row kernels against train_ops.pt_block_usable forced false.

    python scripts/pair_shapes_timing.py [--reps 20] [--rounds 3] [--out profiles/pair_shapes_timing.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ptt_amd import ops, synth, train_ops                                          # noqa: E402
from ptt_amd.models.transformer_block.variants import TransformerBlock             # noqa: E402
from tests.util import fill_state_dict_                                            # noqa: E402

PEAK = 157.3
B = 48
TRAIN_PAIRS = ((256, 8), (512, 32))


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


def _inputs(N, dev):
    xyz = torch.from_numpy(synth.frames(7 + N, B, N, 64, K_s=N)[0]).to(dev)
    feat = torch.from_numpy(np.random.RandomState(N).standard_normal((B, N, 256)).astype(np.float32)).to(dev)
    return xyz, feat


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_shapes_timing.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = dict(device=torch.cuda.get_device_name(0), B=B, reps=a.reps, rounds=a.rounds, peak_tflops=PEAK, eval=[], train=[])
    try:
        out["build"] = open(os.path.join(ROOT, "ptt_amd", "lib", "BUILD_ID")).read().strip()
    except OSError:
        pass
    for N in (128, 64):
        xyz, feat = _inputs(N, dev)
        for D in (128, 256, 512):
            for k in (8, 16, 32):
                fused = fill_state_dict_(TransformerBlock(256, D, k), 11).to(dev).eval()
                stock = fill_state_dict_(TransformerBlock(256, D, k), 11).to(dev).eval()
                stock._fusable = lambda *x: False
                ops.unfused_calls.clear()
                with torch.no_grad():
                    f_fused = lambda: fused(xyz, feat, want_attn=False)
                    f_stock = lambda: stock(xyz, feat)
                    t_fused, t_stock = [], []
                    for _ in range(a.rounds):                  # alternate the two paths
                        t_fused.append(_time(f_fused, a.reps))
                        t_stock.append(_time(f_stock, a.reps))
                assert not ops.unfused_calls, ops.unfused_calls            # the fused side really was the fused path
                tf, ts = float(np.median(t_fused)), float(np.median(t_stock))
                flops = B * N * k * 2.0 * (3 * D + 3 * D * D)
                r = dict(N=N, D=D, k=k, fused_ms=round(tf, 4), stock_ms=round(ts, 4), speedup=round(ts / tf, 2),
                         pair_gflop=round(flops / 1e9, 3), fused_tflops=round(flops / tf / 1e9, 2),
                         fused_frac_peak=round(flops / tf / 1e9 / PEAK, 3))
                out["eval"].append(r)
                print(json.dumps(r), flush=True)
    usable = train_ops.pt_block_usable
    for N in (128, 64):
        xyz, feat = _inputs(N, dev)
        for D, k in TRAIN_PAIRS:
            blk = fill_state_dict_(TransformerBlock(256, D, k), 11).to(dev).train()
            f = feat.clone().requires_grad_(True)

            def step():
                blk.zero_grad(set_to_none=True)
                f.grad = None
                blk(xyz, f)[0].sum().backward()

            assert usable(blk, xyz, f)
            t_rows, t_stock = [], []
            for _ in range(a.rounds):
                train_ops.pt_block_usable = usable
                t_rows.append(_time(step, a.reps))
                train_ops.pt_block_usable = lambda *x: False
                t_stock.append(_time(step, a.reps))
            train_ops.pt_block_usable = usable
            tr, ts = float(np.median(t_rows)), float(np.median(t_stock))
            r = dict(N=N, D=D, k=k, rows_ms=round(tr, 4), stock_ms=round(ts, 4), speedup=round(ts / tr, 2))
            out["train"].append(r)
            print(json.dumps(r), flush=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
