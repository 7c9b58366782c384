"""MulTransformerBlock timing over DIM_MODEL 128 / 256 x KNN 8 / 16 / 32 x heads (hd >= 32) on one GPU, B = 48, N = 128, 1 and 2
layers: HIP-event time of the eval-mode block on the fused path (kNN once per block; per layer the q|k|v projection, the multi-head
pair kernel, proj, LayerNorm, fc2, LayerNorm + residual) and on the stock torch path the same module takes when `_fusable` says no
(what these shapes ran before the instantiations existed), alternated in one process, median of the rounds. Then one training step
(forward + backward of a sum loss) at (256, 8, heads 4) and (128, 32, heads 2), one layer, on the row kernels against
train_ops.mul_block_usable forced false.

    python scripts/mul_shapes_timing.py [--reps 20] [--rounds 3] [--out profiles/mul_shapes_timing.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ptt_amd import ops, synth, train_ops                                                   # noqa: E402
from ptt_amd.models.transformer_block.multitransformer import MulTransformerBlock           # noqa: E402
from tests.multitransformer_ref import seeded_                                              # noqa: E402

B, N = 48, 128
D_HEADS = ((128, 1), (128, 2), (128, 4), (256, 1), (256, 2), (256, 4), (256, 8))
TRAIN_SHAPES = ((256, 8, 4), (128, 32, 2))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mul_shapes_timing.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = dict(device=torch.cuda.get_device_name(0), B=B, N=N, reps=a.reps, rounds=a.rounds, eval=[], train=[])
    try:
        out["build"] = open(os.path.join(ROOT, "ptt_amd", "lib", "BUILD_ID")).read().strip()
    except OSError:
        pass
    xyz = torch.from_numpy(synth.frames(7 + N, B, N, 64, K_s=N)[0]).to(dev)
    feat = torch.from_numpy(np.random.RandomState(N).standard_normal((B, N, 256)).astype(np.float32)).to(dev)
    for layers in (1, 2):
        for D, heads in D_HEADS:
            for k in (8, 16, 32):
                fused = seeded_(MulTransformerBlock(256, D, k, heads, layers), 11).to(dev).eval()
                stock = seeded_(MulTransformerBlock(256, D, k, heads, layers), 11).to(dev).eval()
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
                r = dict(layers=layers, D=D, heads=heads, k=k, fused_ms=round(tf, 4), stock_ms=round(ts, 4), speedup=round(ts / tf, 2))
                out["eval"].append(r)
                print(json.dumps(r), flush=True)
    usable = train_ops.mul_block_usable
    for D, k, heads in TRAIN_SHAPES:
        blk = seeded_(MulTransformerBlock(256, D, k, heads, 1), 11).to(dev).train()
        f = feat.clone().requires_grad_(True)

        def step():
            blk.zero_grad(set_to_none=True)
            f.grad = None
            blk(xyz, f)[0].sum().backward()

        assert usable(blk, xyz, f)
        t_rows, t_stock = [], []
        for _ in range(a.rounds):
            train_ops.mul_block_usable = usable
            t_rows.append(_time(step, a.reps))
            train_ops.mul_block_usable = lambda *x: False
            t_stock.append(_time(step, a.reps))
        train_ops.mul_block_usable = usable
        tr, ts = float(np.median(t_rows)), float(np.median(t_stock))
        r = dict(D=D, k=k, heads=heads, layers=1, rows_ms=round(tr, 4), stock_ms=round(ts, 4), speedup=round(ts / tr, 2))
        out["train"].append(r)
        print(json.dumps(r), flush=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
