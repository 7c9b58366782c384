"""Timing of the OPTIMIZATION block's optimizer steps on the device -> ONE JSON line (default: profiles/optim_step_timing.json).

    python scripts/optim_step_timing.py [--steps 50] [--warmup 5] [--batch 48] [--out profiles/optim_step_timing.json]

Part 1, the optimizer step alone, on the full tracker's parameter set with clipping at 10: for each OPTIMIZER value (adam, adamw,
sgd, adam_onecycle with OneCycle moving lr and beta1 every step) the fused step (ptt_amd.optim: two launches) and
clip_grad_norm_ + the stock foreach=True optimizer — for adam_onecycle the reference's own sequence (clip_grad_norm_, p.mul_(1 -
wd lr) as one _foreach_mul_, Adam.step()) — alternating in one loop on the same seeded gradients; per form the median (and
minimum) over `steps` steps after `warmup` of the device time (events around the step) and of the host time to ISSUE it (host
clock around the calls, no synchronise inside).

Part 2, the training step of BASELINE.json configs[3] (nuScenes-Car shaped, batch 48, 1024 + 512 points) with adam_onecycle +
OneCycle in three forms: replayed as a graph, eager with the fused step, eager with the reference's sequence on stock torch; per
form device ms per step (events around a run of steps, divided) and host issue ms per step. Without a device this raises.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ptt_amd.config import EasyDict, StubDataset, ptt_model_cfg      # noqa: E402
from ptt_amd.models import build_network                             # noqa: E402
from ptt_amd.optimization import OneCycle, build_optimizer           # noqa: E402

CLIP, WD = 10.0, 0.01
CFG = dict(LR=1e-3, WEIGHT_DECAY=WD, BETAS=[0.5, 0.999], EPS=1e-6, MOMENTUM=0.9, MOMS=[0.95, 0.85], DIV_FACTOR=10, PCT_START=0.4)
STOCK = {"adam": lambda ps: torch.optim.Adam(ps, lr=1e-3, weight_decay=WD, betas=(0.5, 0.999), eps=1e-6, foreach=True),
         "adamw": lambda ps: torch.optim.AdamW(ps, lr=1e-3, weight_decay=WD, betas=(0.5, 0.999), eps=1e-6, foreach=True),
         "sgd": lambda ps: torch.optim.SGD(ps, lr=1e-3, weight_decay=WD, momentum=0.9, foreach=True),
         "adam_onecycle": lambda ps: torch.optim.Adam(ps, lr=3e-3, betas=(0.9, 0.99), weight_decay=0, foreach=True)}


def _stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(np.min(ms)), 4)}


def _timed(fn):
    """-> (device ms, host issue ms) of fn()."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    t0 = time.perf_counter()
    fn()
    host = (time.perf_counter() - t0) * 1e3
    b.record()
    b.synchronize()
    return a.elapsed_time(b), host


def _reference_step(params, opt, onecycle):
    """clip_grad_norm_ + optimizer.step() as the reference runs it; for adam_onecycle OptimWrapper.step's decay in front."""
    torch.nn.utils.clip_grad_norm_(params, CLIP)
    if onecycle:
        with torch.no_grad():
            torch._foreach_mul_(params, 1 - WD * opt.param_groups[0]['lr'])
    opt.step()


def optimizer_steps(dev, steps, warmup):
    out = []
    for name in ("adam", "adamw", "sgd", "adam_onecycle"):
        torch.manual_seed(3)
        models = [build_network(ptt_model_cfg(), 1, StubDataset(training=True)).to(dev).train() for _ in range(2)]
        models[1].load_state_dict(models[0].state_dict())
        fused = build_optimizer(models[0], EasyDict(dict(CFG, OPTIMIZER=name)))
        held = [[p for g in fused.param_groups for p in g['params']]]
        pos = {id(p): i for i, p in enumerate(models[0].parameters())}
        theirs = list(models[1].parameters())
        held.append([theirs[pos[id(p)]] for p in held[0]])
        stock = STOCK[name](held[1])
        total = steps + warmup
        scheds = [OneCycle(o, total, 3e-3, (0.95, 0.85), 10, 0.4) for o in (fused, stock)] if name == "adam_onecycle" else []
        gen = torch.Generator(device=dev).manual_seed(5)
        grads = [torch.randn(p.shape, generator=gen, device=dev) * 0.5 for p in held[0]]      # norm ~ 1100: the clip is active
        for ps in held:
            for p in ps:
                p.grad = torch.empty_like(p)
        runs = {"fused": lambda: fused.step(max_norm=CLIP), "stock": lambda: _reference_step(held[1], stock, name == "adam_onecycle")}
        ms = {k: ([], []) for k in runs}
        for it in range(total):
            for s in scheds:
                s.step(it)
            for k, fn in runs.items():
                ps = held[0] if k == "fused" else held[1]
                torch._foreach_copy_([p.grad for p in ps], grads)
                d, h = _timed(fn)
                if it >= warmup:
                    ms[k][0].append(d)
                    ms[k][1].append(h)
        worst = max(float((p.detach() - q.detach()).abs().max()) for p, q in zip(*held))
        row = {"optimizer": name, "tensors": len(held[0]), "values": int(sum(p.numel() for p in held[0])), "groups": len(fused.param_groups),
               "largest_parameter_difference_after_%d_steps" % total: worst}
        for k in runs:
            row[k] = {"device": _stats(ms[k][0]), "host_issue": _stats(ms[k][1])}
        row["ratio_stock_over_fused_device"] = round(row["stock"]["device"]["median_ms"] / row["fused"]["device"]["median_ms"], 2)
        out.append(row)
    return out


class _StockOneCycleTrainer(object):
    """The reference's loop body on stock torch: OneCycle.step(it); zero_grad; forward; backward; clip_grad_norm_; OptimWrapper.step."""

    def __init__(self, model, total):
        self.model, self.it = model, 0
        self.params = [p for p in model.parameters() if p.requires_grad]
        self.opt = STOCK["adam_onecycle"](self.params)
        self.sched = OneCycle(self.opt, total, 3e-3, (0.95, 0.85), 10, 0.4)

    def step(self, batch):
        self.sched.step(self.it)
        self.it += 1
        self.opt.zero_grad(set_to_none=True)
        ret, _, _ = self.model(dict(batch))
        loss = ret['loss'] if ret['loss'].dim() == 0 else ret['loss'].mean()
        loss.backward()
        _reference_step(self.params, self.opt, True)
        return loss


def training_steps(dev, B, steps, warmup):
    from ptt_amd.train_step import DataParallelTrainer, synthetic_train_batch
    batches = [synthetic_train_batch(500 + k, B, dev) for k in range(3)]
    total = 2 * (steps + warmup) + 8
    cfg = EasyDict(dict(CFG, OPTIMIZER="adam_onecycle", LR=3e-3, GRAD_NORM_CLIP=CLIP))

    def model():
        torch.manual_seed(4)
        return build_network(ptt_model_cfg(), 1, StubDataset(training=True)).to(dev).train()
    forms = {"graph_replay": DataParallelTrainer.from_optim_cfg(model(), dev, cfg, total, 1, graph=True, graph_warmup=3),
             "eager_fused": DataParallelTrainer.from_optim_cfg(model(), dev, cfg, total, 1, graph=False),
             "eager_stock_reference_sequence": _StockOneCycleTrainer(model(), total)}
    out = {"batch": B, "points": "%d x (1024 + 512)" % B, "optimizer": "adam_onecycle + OneCycle, GRAD_NORM_CLIP 10, WEIGHT_DECAY %g" % WD}
    for name, t in forms.items():
        for k in range(max(warmup, 4)):
            t.step(batches[k % 3])
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        host = []
        a.record()
        for k in range(steps):
            t0 = time.perf_counter()
            loss = t.step(batches[k % 3])
            host.append((time.perf_counter() - t0) * 1e3)
        b.record()
        b.synchronize()
        assert bool(torch.isfinite(loss))
        out[name] = {"device_ms_per_step": round(a.elapsed_time(b) / steps, 3), "host_issue_ms_per_step": _stats(host)}
        if name == "graph_replay":
            out[name]["graph_steps"] = t.graph_steps
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=48)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_step_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("scripts/optim_step_timing.py measures on the device; none is visible")
    dev = torch.device("cuda:0")
    out = {"what": "optimizer step (fused two-launch step vs clip_grad_norm_ + stock foreach optimizer) and the configs[3] training "
                   "step with adam_onecycle; median of %d steps after %d warm-ups; device = events, host_issue = host clock "
                   "around the calls without a synchronise" % (args.steps, args.warmup),
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "optimizer_step": optimizer_steps(dev, args.steps, args.warmup),
           "training_step": training_steps(dev, args.batch, args.steps, args.warmup)}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
