"""The stream launch of ptt_sa_fused_fwd_f32 (hoisted 128-channel layer 0, 128 -> 128 -> 256, 32 neighbours) alone: dense
(sa_stream_kernel) against compact (compact_ws: counter reset + sa_compact_kernel<false> + sa_stream_compact_kernel).
20 calls per captured graph, median of 7 replays, us per call. Rows: the search branch's last level from 1 to 48 frames and
the other three stream shapes at 8 and 48 frames, car and ped inputs; the last level of the 16384-point stress clouds
(N = 4096 points per cloud, full balls). Output: profiles/sa2c_stream_dense_vs_compact.log.
    python scripts/sa_stream_compact_bench.py"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ptt_amd import _lib, ops, synth                 # noqa: E402
from tests.util import fold_layers, mlp_layers       # noqa: E402

dev = torch.device('cuda:0')
folded = fold_layers(mlp_layers(17, [131, 128, 128, 256]), dev, ops, scale_in_weights=True)[1:]
wx = torch.randn(3, 128, device=dev)


def measure(tag, cloud, n0, N, M, r):
    B = cloud.shape[0]
    inds = ops.furthest_point_sampling(cloud, n0).long()
    xyz = torch.gather(cloud, 1, inds[..., None].expand(-1, -1, 3))[:, :N].contiguous()
    new_xyz, _, idx = ops.centres_ball_query(xyz, None, M, r, 32)
    real = ((idx != idx[..., :1]).sum(-1) + 1).float().mean().item()
    term = torch.randn(B, N, 128, device=dev)
    ws = torch.empty((_lib.lib().ptt_sa_compact_workspace(B, M) + 3) // 4, dtype=torch.int32, device=dev)
    row = {}
    for name, c in (('dense', False), ('compact', ws)):
        def f():
            return ops.sa_fused_forward(xyz, new_xyz, idx, None, folded, r, True, True, l0=(term, wx, True), compact=c)
        f()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(20):
                f()
        ts = []
        for _ in range(7):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b) / 20 * 1e3)
        row[name] = round(float(np.median(ts)), 2)
    print(tag, 'N%d M%d' % (N, M), 'B', B, 'balls', B * M, 'real hits %.2f' % real, row, flush=True)


for kind in ('car', 'ped'):
    for (N, M, r, n0, templ) in ((256, 128, 0.7, 512, False), (512, 256, 0.5, 512, False), (256, 128, 0.5, 256, True),
                                 (128, 64, 0.7, 256, True)):
        for B in (1, 2, 4, 8, 16, 48):
            if (N, M) != (256, 128) and B not in (8, 48):
                continue
            K = (600, 300) if kind == 'car' else (60, 40)
            s, t = synth.frames(1000, B, 2048, 1024, K_s=K[0], K_t=K[1], kind=kind)
            measure('%s %s' % (kind, 'template' if templ else 'search'), torch.from_numpy(t if templ else s).to(dev), n0, N, M, r)
s, _ = synth.frames(1000, 32, 16384, 4096, K_s=16384, K_t=4096, kind='dense')
measure('stress search', torch.from_numpy(s).to(dev), 8192, 4096, 2048, 0.7)
