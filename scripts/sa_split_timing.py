"""The split-bf16 stream kernel (ptt_sa_stream_split_f32, precision 'bf16x2' of PointnetSAModuleVotes) against the dense fp32
stream kernel (sa_stream_kernel<32> behind ptt_sa_fused_fwd_f32) on one GPU, alternated in one process.

  * the kernel's launch alone (ops.start_kernel_timing) at B = 48 on the four dense-shaped levels of the car step — search SA1
    512 -> 256, search SA2 256 -> 128, template SA1 256 -> 128, template SA2 128 -> 64 — at one frame's search SA1 (B = 1) and on
    the stress shape (B = 32, 8192 -> 4096);
  * the eval-mode backbone branch (search, B = 48) with SA_CONFIG.PRECISION 'fp32' / 'bf16x2';
  * the full tracker forward at B = 48 as a graph replay, fp32 against set_precision(..., scope=('transformer',)) and
    scope=('transformer', 'sa');
  * distances, reported and not asserted: the backbone branch from fixture G4 and the full tracker from fixture G6, per arm.
Median of the rounds per arm, with each arm's min and max kept. `faster` = the fp32 median exceeds the bf16x2 median by more
than the fp32 arm's own min-max spread — the rule by which a level is dispatched (pointnet2_modules.SPLIT_STREAM_MIN_BALLS).

    python scripts/sa_split_timing.py [--reps 20] [--rounds 5] [--out profiles/sa_split_timing.json]
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
from ptt_amd.hot_path import AttrDict                                              # noqa: E402
from ptt_amd.models.backbones_3d.pointnet2 import pointnet2_modules as PM          # noqa: E402
from ptt_amd.precision import set_precision                                        # noqa: E402
from tests.util import fill_state_dict_, mlp_layers                                # noqa: E402

PEAK = 157.3
KERNELS = {"fp32": "ptt_sa_fused_fwd_f32", "bf16x2": "ptt_sa_stream_split_f32"}
ARMS = ("fp32", "bf16x2")
LEVELS = [("search SA1", 48, 512, 256, 0.5), ("search SA2", 48, 256, 128, 0.7), ("template SA1", 48, 256, 128, 0.5),
          ("template SA2", 48, 128, 64, 0.7), ("one frame, search SA1", 1, 512, 256, 0.5), ("stress search SA1", 32, 8192, 4096, 0.5)]
GOLD = os.path.join(ROOT, "tests", "golden")


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


def _verdict(a, base="fp32", arm="bf16x2"):
    spread = a[base]["max_ms"] - a[base]["min_ms"]
    gain = a[base]["median_ms"] - a[arm]["median_ms"]
    return dict(speedup=round(a[base]["median_ms"] / a[arm]["median_ms"], 3), fp32_spread_ms=round(spread, 4), faster=bool(gain > spread))


def level_case(name, B, N, M, radius, dev, reps, rounds):
    """The two kernels on one level's shape: random per-point terms and weights, centres = the first M points of FPS-ordered clouds."""
    src = torch.from_numpy(synth.frames(5 + N, B, max(N, 1024), 64, K_s=max(N, 1024))[0]).to(dev)
    order = ops.furthest_point_sampling(src, N).long()
    xyz = torch.gather(src, 1, order[..., None].expand(-1, -1, 3)).contiguous()
    new_xyz = xyz[:, :M].contiguous()
    idx = ops.ball_query(new_xyz, xyz, radius, 32)
    rs = np.random.RandomState(N + M)
    rnd = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32)).to(dev)
    term, wx = rnd(B, N, 128), rnd(3, 128) * 0.5
    W1, W2 = rnd(128, 128) * (2.0 / 128) ** 0.5, rnd(256, 128) * (2.0 / 128) ** 0.5
    sh1, sh2 = rnd(128) * 0.2, rnd(256) * 0.2
    layers = [(ops.pack_weight(W1), None, sh1, 128, 128, True), (ops.pack_weight(W2), None, sh2, 128, 256, True)]
    w1s, w2s = ops.pack_weight_split(W1), ops.pack_weight_split(W2)
    fns = {"fp32": lambda: ops.sa_fused_forward(xyz, new_xyz, idx, None, layers, radius, True, True, l0=(term, wx, True)),
           "bf16x2": lambda: ops.sa_stream_split(xyz, new_xyz, idx, (term, wx, True), w1s, sh1, w2s, sh2, radius, True)}
    y32, ysp = fns["fp32"](), fns["bf16x2"]()
    diff = float((y32 - ysp).abs().max() / y32.abs().max())
    ts = {a: [] for a in ARMS}
    for _ in range(rounds):
        for arm in ARMS:
            ts[arm].append(_kernel_time(fns[arm], KERNELS[arm], reps))
    a = {arm: _arm(ts[arm]) for arm in ARMS}
    flops = B * M * 32 * 2.0 * (128 * 128 + 128 * 256)
    for arm in ARMS:
        a[arm]["tflops"] = round(flops / a[arm]["median_ms"] / 1e9, 1)
    return dict(level=name, B=B, N=N, M=M, balls=B * M, gflop=round(flops / 1e9, 3), rel_diff_from_fp32=diff, **a, **_verdict(a))


def _backbone(dev, precision):
    from ptt_amd.models.backbones_3d.pointnet2_backbone import PointNet2BackboneLight
    from tests.test_golden_gpu import _load_mlp
    cfg = AttrDict.wrap(dict(DEBUG=False, SA_CONFIG=dict(
        SAMPLE_METHOD=['fps', 'sequence', 'sequence'], USE_XYZ=True, NORMALIZE_XYZ=True, PRECISION=precision,
        NPOINTS_SEARCH=[512, 256, 128], NPOINTS_TEMPLATE=[256, 128, 64], RADIUS=[0.3, 0.5, 0.7],
        NSAMPLE=[32, 32, 32], MLPS=[[0, 64, 64, 128], [128, 128, 128, 256], [256, 128, 128, 256]])))
    bb = PointNet2BackboneLight(cfg, input_channels=3).eval()
    specs = [[3, 64, 64, 128], [131, 128, 128, 256], [259, 128, 128, 256]]
    for i, sa in enumerate(bb.SA_modules):
        _load_mlp(sa.mlp_module, mlp_layers(400 + i, specs[i]))
    g = np.load(os.path.join(GOLD, "G4_backbone_branch.npz"))
    with torch.no_grad():
        bb.cov_final.weight.copy_(torch.from_numpy(g["cov_w"]))
        bb.cov_final.bias.copy_(torch.from_numpy(g["cov_b"]))
    return bb.to(dev), g


def branch_case(dev, reps, rounds):
    """The eval-mode search branch at B = 48 (FPS, three SA levels, cov_final) per arm, and fixture G4's distance per arm."""
    out = dict(B=48)
    bbs, dist = {}, {}
    for arm in ARMS:
        bbs[arm], g = _backbone(dev, arm)
        with torch.no_grad():
            f = bbs[arm].branch_forward(torch.from_numpy(g["pts"]).to(dev), [512, 256, 128])[1]
        d = np.abs(f.cpu().numpy() - g["feats"])
        dist[arm] = dict(max_abs=float(d.max()), tol_units=float((d / (1e-4 + 1e-4 * np.abs(g["feats"]))).max()))
    s = torch.from_numpy(synth.frames(300, 48, 1024, 512)[0]).to(dev)
    ts = {a: [] for a in ARMS}
    with torch.no_grad():
        for _ in range(rounds):
            for arm in ARMS:
                ts[arm].append(_time(lambda: bbs[arm].branch_forward(s, [512, 256, 128]), reps))
    a = {arm: _arm(ts[arm]) for arm in ARMS}
    return dict(out, G4_distance=dist, **a, **_verdict(a))


TRACKER_ARMS = (("fp32", "fp32", ("transformer", "sa")), ("transformer", "bf16x2", ("transformer",)),
                ("transformer+sa", "bf16x2", ("transformer", "sa")))


def tracker_case(B, dev, reps, rounds):
    from ptt_amd.config import StubDataset, ptt_model_cfg
    from ptt_amd.hot_path import GraphedHotPath, TrackerThroughput, randomize_
    from ptt_amd.models import build_network
    tracker = randomize_(build_network(ptt_model_cfg(), 1, StubDataset()), seed=4).to(dev).eval()
    s, t = (torch.from_numpy(a).to(dev) for a in synth.frames(300, B, 1024, 512))
    g = GraphedHotPath(TrackerThroughput(tracker), s, t)
    ts = {a[0]: [] for a in TRACKER_ARMS}
    counts = {}
    for _ in range(rounds):
        for name, precision, scope in TRACKER_ARMS:
            set_precision(tracker, "fp32", scope=("transformer", "sa"))
            counts[name] = set_precision(tracker, precision, scope=scope)      # the next call captures again
            ts[name].append(_time(lambda: g(), reps))
    set_precision(tracker, "fp32", scope=("transformer", "sa"))
    a = {name: _arm(ts[name]) for name in ts}
    return dict(B=B, modules_set=counts, fallbacks={"%s: %s" % k: v for k, v in ops.precision_fallbacks.items()}, **a,
                sa_over_transformer=_verdict(a, "transformer", "transformer+sa"), sa_over_fp32=_verdict(a, "fp32", "transformer+sa"))


def g6_case(dev):
    """The full tracker on fixture G6 per arm: the worst element of four tensors in units of the 1e-4 tolerance."""
    from ptt_amd.config import StubDataset, ptt_model_cfg
    from ptt_amd.models import build_network
    g = np.load(os.path.join(GOLD, "G6_ptt_forward.npz"))
    model = fill_state_dict_(build_network(ptt_model_cfg(), 1, StubDataset()), int(g["seed"])).to(dev).eval()
    out = {}
    for name, precision, scope in TRACKER_ARMS:
        set_precision(model, "fp32", scope=("transformer", "sa"))
        set_precision(model, precision, scope=scope)
        with torch.no_grad():
            o = model({'search_points': torch.from_numpy(g["search"]).to(dev), 'template_points': torch.from_numpy(g["template"]).to(dev),
                       'batch_size': 2})
        out[name] = {k: round(float((np.abs(o[k].cpu().numpy() - g[k]) / (1e-4 + 1e-4 * np.abs(g[k]))).max()), 4)
                     for k in ('cosine_feats', 'pred_centroids_cls', 'pred_centroids_votes', 'votes_feats')}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-tracker", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sa_split_timing.json"))
    a = ap.parse_args()
    warnings.simplefilter("ignore")
    dev = torch.device("cuda:0")
    out = dict(device=torch.cuda.get_device_name(0), reps=a.reps, rounds=a.rounds, peak_fp32_tflops=PEAK,
               split_stream_min_balls=PM.SPLIT_STREAM_MIN_BALLS, levels=[], branch=None, tracker=None, G6_tol_units=None)
    try:
        out["build"] = open(os.path.join(ROOT, "ptt_amd", "lib", "BUILD_ID")).read().strip()
    except OSError:
        pass

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")

    for lv in LEVELS:
        r = level_case(*lv, dev, a.reps, a.rounds)
        out["levels"].append(r)
        print(json.dumps(r), flush=True)
        save()
    out["branch"] = branch_case(dev, a.reps, a.rounds)
    print(json.dumps(out["branch"]), flush=True)
    save()
    if not a.skip_tracker:
        out["G6_tol_units"] = g6_case(dev)
        print(json.dumps(out["G6_tol_units"]), flush=True)
        out["tracker"] = tracker_case(48, dev, a.reps, a.rounds)
        print(json.dumps(out["tracker"]), flush=True)
    save()


if __name__ == "__main__":
    main()
