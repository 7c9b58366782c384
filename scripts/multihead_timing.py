"""MulTransformerBlock timing on one GPU: for each fused head count at B = 48 and N = 128 / 64, the per-head pair kernel
against the block-diagonal baseline (the same attention on the single-head kernel with fc_gamma expanded to a D x D
block-diagonal weight), alternated in one process; the whole block's eval forward; algorithmic TFLOP/s and the fraction of
the 157.3 TFLOP/s fp32-MFMA peak. Per (point, neighbour) row the per-head kernel's FLOPs are 2 (3 D + D^2 + 2 D hd).

    python scripts/multihead_timing.py [--reps 20] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ptt_amd import ops, synth                                                    # noqa: E402
from ptt_amd.models.transformer_block.multitransformer import MulTransformerBlock  # noqa: E402
from tests.util import fill_state_dict_                                           # noqa: E402

PEAK = 157.3
D, K = 512, 16


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
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for N in (128, 64):
        xyz = torch.from_numpy(synth.frames(7 + N, 48, N, 64, K_s=N)[0]).to(dev)
        feat = torch.from_numpy(np.random.RandomState(N).standard_normal((48, N, 256)).astype(np.float32)).to(dev)
        knn_idx, rel = ops.knn(xyz, K, want_rel=True)
        for heads, layers in ((1, 1), (2, 1), (4, 1), (8, 1), (4, 2)):
            blk = fill_state_dict_(MulTransformerBlock(256, D, K, heads, layers), 11).to(dev).eval()
            L = blk.layers[0]
            with torch.no_grad():
                P = L._params()
                qkv = ops.linear(feat, P['qkv'], 3 * D, None, P['qkv_b'])
                pair = lambda: ops.pt_attn_pair(xyz, knn_idx, qkv, P['wd1'], P['wd2'], P['bd2'], P['wg1'], P['bg1'], P['wg2'],
                                                P['bg2'], D, False, rel=rel, heads=heads)
                base = lambda: ops.pt_attn_pair(xyz, knn_idx, qkv, P['wd1'], P['wd2'], P['bd2'], P['wg1_bd'], P['bg1'],
                                                P['wg2_bd'], P['bg2'], D, False, rel=rel, heads=1)
                fwd = lambda: blk(xyz, feat, want_attn=False)
                t_pair, t_base, t_fwd = [], [], []
                for _ in range(a.rounds):                      # alternate the two kernels
                    t_pair.append(_time(pair, a.reps))
                    if heads > 1:
                        t_base.append(_time(base, a.reps))
                    t_fwd.append(_time(fwd, a.reps))
            hd = D // heads
            flops = 48 * N * K * 2.0 * (3 * D + D * D + 2 * D * hd)
            tp = float(np.median(t_pair))
            r = dict(B=48, N=N, heads=heads, layers=layers, pair_ms=round(tp, 4),
                     pair_tflops=round(flops / tp / 1e9, 2), pair_frac_peak=round(flops / tp / 1e9 / PEAK, 3),
                     block_forward_ms=round(float(np.median(t_fwd)), 4))
            if heads > 1:
                tb = float(np.median(t_base))
                r.update(blockdiag_ms=round(tb, 4), speedup=round(tb / tp, 3))
            rows.append(r)
            print(json.dumps(r), flush=True)
    if a.json:
        json.dump(rows, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
