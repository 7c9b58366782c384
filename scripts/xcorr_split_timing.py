"""The split-bf16 xcorr kernel (ptt_xcorr_split_f32, precision 'bf16x2' of CosineSimAug) against the fp32 kernel
(xcorr_fused_kernel<2, false> behind ptt_xcorr_fused_fwd_f32) on one GPU, alternated in one process.

  * the kernel's launch alone (ops.start_kernel_timing) at Ns = 128, Nt = 64 and B = 48 (the car step), B = 8 and B = 5 (the
    smallest batched call), and at the stress shape's Nt = 512 (B = 8, Ns = 1024);
  * the eval-mode CosineSimAug module at B = 48 with SIMILARITY_MODULE.PRECISION 'fp32' / 'bf16x2';
  * the full tracker forward at B = 48 as a graph replay: fp32, set_precision(..., scope=('transformer', 'sa')) and
    scope=('transformer', 'sa', 'similarity');
  * distances, reported and not asserted: the full tracker from fixture G6, per arm, in units of the 1e-4 tolerance — on the
    fixture's two frames (CosineSimAug's one-frame form: fp32 under every scope) and on the same frames three times over (B = 6:
    the batched branch, where scope 'similarity' acts).
Median of the rounds per arm, with each arm's min and max kept. `faster` = the fp32 median exceeds the bf16x2 median by more
than the fp32 arm's own min-max spread — the rule by which a shape is dispatched (p2b_xcoor.SPLIT_XCORR_MIN_POINTS).

    python scripts/xcorr_split_timing.py [--reps 20] [--rounds 5] [--out profiles/xcorr_split_timing.json]
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
from ptt_amd.models.similarity_modules import p2b_xcoor as PX                      # noqa: E402
from ptt_amd.precision import set_precision                                        # noqa: E402
from tests.util import cosine_sim_params, fill_state_dict_, load_cosine_sim        # noqa: E402

PEAK = 157.3
KERNELS = {"fp32": "ptt_xcorr_fused_fwd_f32", "bf16x2": "ptt_xcorr_split_f32"}
ARMS = ("fp32", "bf16x2")
SHAPES = [("car step", 48, 128, 64), ("B = 8", 8, 128, 64), ("smallest batched", 5, 128, 64), ("stress, Nt = 512", 8, 1024, 512)]
ALL = ("transformer", "sa", "similarity")
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


def kernel_case(name, B, Ns, Nt, dev, reps, rounds):
    """The two kernels on one shape: random cosines, per-template-point terms and weights."""
    rs = np.random.RandomState(B + Ns + Nt)
    rnd = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32)).to(dev)
    cos_t = torch.from_numpy(rs.uniform(-1, 1, (B, Ns, Nt)).astype(np.float32)).to(dev)
    P, w_sim = rnd(B, Nt, 256), rnd(256) * 0.5
    W1, W2 = rnd(256, 256) * (2.0 / 256) ** 0.5, rnd(256, 256) * (2.0 / 256) ** 0.5
    sh1, sh2 = rnd(256) * 0.2, rnd(256) * 0.2
    layers = [(ops.pack_weight(W1), None, sh1, 256, 256, True), (ops.pack_weight(W2), None, sh2, 256, 256, True)]
    w1s, w2s = ops.pack_weight_split(W1), ops.pack_weight_split(W2)
    sf, tf = torch.empty((B, 4, Ns), device=dev), torch.empty((B, 4, Nt), device=dev)       # shapes only: cos_t is given
    fns = {"fp32": lambda: ops.xcorr_fused(sf, tf, P, w_sim, None, None, layers, cos_t=cos_t)[0],
           "bf16x2": lambda: ops.xcorr_split(cos_t, P, w_sim, w1s, sh1, w2s, sh2)}
    y32, ysp = fns["fp32"](), fns["bf16x2"]()
    diff = float((y32 - ysp).abs().max() / y32.abs().max())
    ts = {a: [] for a in ARMS}
    for _ in range(rounds):
        for arm in ARMS:
            ts[arm].append(_kernel_time(fns[arm], KERNELS[arm], reps))
    a = {arm: _arm(ts[arm]) for arm in ARMS}
    flops = B * Ns * Nt * 2.0 * 2 * 256 * 256
    for arm in ARMS:
        a[arm]["tflops"] = round(flops / a[arm]["median_ms"] / 1e9, 1)
    return dict(shape=name, B=B, Ns=Ns, Nt=Nt, points=B * Ns, gflop=round(flops / 1e9, 3), rel_diff_from_fp32=diff, **a, **_verdict(a))


def module_case(dev, reps, rounds):
    """The eval-mode CosineSimAug module at B = 48 (64 template and 128 search seeds, 256 feature channels) per arm."""
    mods = {}
    for arm in ARMS:
        m = PX.CosineSimAug(AttrDict.wrap(dict(DEBUG=False, PRECISION=arm, MLP=dict(CHANNELS=[260, 256, 256, 256], BN=True),
                                               CONV=dict(CHANNELS=[256, 256, 256], BN=True)))).eval()
        load_cosine_sim(m, *cosine_sim_params(9))
        mods[arm] = m.to(dev)
    rs = np.random.RandomState(48)
    rnd = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32)).to(dev)
    batch = {'search_feats': rnd(48, 128, 256).transpose(1, 2), 'template_feats': rnd(48, 64, 256).transpose(1, 2),
             'template_seeds': rnd(48, 64, 3)}
    ts = {a: [] for a in ARMS}
    with torch.no_grad():
        y = {arm: mods[arm](dict(batch))['cosine_feats'] for arm in ARMS}
        for _ in range(rounds):
            for arm in ARMS:
                ts[arm].append(_time(lambda: mods[arm](dict(batch)), reps))
    a = {arm: _arm(ts[arm]) for arm in ARMS}
    return dict(B=48, rel_diff_from_fp32=float((y["fp32"] - y["bf16x2"]).abs().max() / y["fp32"].abs().max()), **a, **_verdict(a))


TRACKER_ARMS = (("fp32", "fp32", ALL), ("transformer+sa", "bf16x2", ("transformer", "sa")), ("transformer+sa+similarity", "bf16x2", ALL))


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
            set_precision(tracker, "fp32", scope=ALL)
            counts[name] = set_precision(tracker, precision, scope=scope)      # the next call captures again
            ts[name].append(_time(lambda: g(), reps))
    set_precision(tracker, "fp32", scope=ALL)
    a = {name: _arm(ts[name]) for name in ts}
    return dict(B=B, modules_set=counts, fallbacks={"%s: %s" % k: v for k, v in ops.precision_fallbacks.items()}, **a,
                similarity_over_transformer_sa=_verdict(a, "transformer+sa", "transformer+sa+similarity"),
                all_over_fp32=_verdict(a, "fp32", "transformer+sa+similarity"))


def g6_case(dev, copies):
    """The full tracker on fixture G6 per arm: the worst element of four tensors in units of the 1e-4 tolerance. copies = 1: the
    fixture's own two frames, which CosineSimAug serves on its one-frame form (fp32 under every scope); copies = 3: the same two
    frames three times over (B = 6, 768 search seeds: the batched branch), each copy held against the fixture."""
    from ptt_amd.config import StubDataset, ptt_model_cfg
    from ptt_amd.models import build_network
    g = np.load(os.path.join(GOLD, "G6_ptt_forward.npz"))
    model = fill_state_dict_(build_network(ptt_model_cfg(), 1, StubDataset()), int(g["seed"])).to(dev).eval()
    rep = lambda a: torch.from_numpy(np.concatenate([a] * copies, axis=0)).to(dev)
    ops.precision_fallbacks.clear()
    out = {}
    for name, precision, scope in TRACKER_ARMS + (("similarity", "bf16x2", ("similarity",)),):
        set_precision(model, "fp32", scope=ALL)
        set_precision(model, precision, scope=scope)
        with torch.no_grad():
            o = model({'search_points': rep(g["search"]), 'template_points': rep(g["template"]), 'batch_size': 2 * copies})
        out[name] = {}
        for k in ('cosine_feats', 'pred_centroids_cls', 'pred_centroids_votes', 'votes_feats'):
            ref = np.concatenate([g[k]] * copies, axis=0)
            got = o[k].cpu().numpy()
            assert got.shape == ref.shape, (k, got.shape, ref.shape)
            out[name][k] = round(float((np.abs(got - ref) / (1e-4 + 1e-4 * np.abs(ref))).max()), 4)
    out["fallbacks"] = {"%s: %s" % k: v for k, v in ops.precision_fallbacks.items()}
    ops.precision_fallbacks.clear()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-tracker", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xcorr_split_timing.json"))
    a = ap.parse_args()
    warnings.simplefilter("ignore")
    dev = torch.device("cuda:0")
    out = dict(device=torch.cuda.get_device_name(0), reps=a.reps, rounds=a.rounds, peak_fp32_tflops=PEAK,
               split_xcorr_min_points=PX.SPLIT_XCORR_MIN_POINTS, kernel=[], module=None, tracker=None, G6_tol_units=None,
               G6_three_times_tol_units=None)
    try:
        out["build"] = open(os.path.join(ROOT, "ptt_amd", "lib", "BUILD_ID")).read().strip()
    except OSError:
        pass

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")

    for sh in SHAPES:
        r = kernel_case(*sh, dev, a.reps, a.rounds)
        out["kernel"].append(r)
        print(json.dumps(r), flush=True)
        save()
    out["module"] = module_case(dev, a.reps, a.rounds)
    print(json.dumps(out["module"]), flush=True)
    save()
    if not a.skip_tracker:
        out["G6_tol_units"] = g6_case(dev, 1)
        print(json.dumps(out["G6_tol_units"]), flush=True)
        out["G6_three_times_tol_units"] = g6_case(dev, 3)
        print(json.dumps(out["G6_three_times_tol_units"]), flush=True)
        out["tracker"] = tracker_case(48, dev, a.reps, a.rounds)
        print(json.dumps(out["tracker"]), flush=True)
    save()


if __name__ == "__main__":
    main()
