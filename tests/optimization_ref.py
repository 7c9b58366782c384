"""What fixture G25 (tests/golden/make_golden_g25.py) and the tests of ptt_amd/optimization.py share: the toy model, its seeded
weights and gradients, the four OPTIMIZATION blocks, and the comparison bar. A plain module (no fixtures, no pytest settings)."""
import os

import numpy as np
import torch
import torch.nn as nn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g25_optimization.npz")

SCHEDULES = [(50, 0.4), (37, 0.1), (7, 0.5)]                 # (total_step, pct_start)
MOMS, DIV_FACTOR, LR_MAX = (0.95, 0.85), 10, 3e-3
STEPS, RECORD, CLIP = 20, (1, 2, 10, 20), 10.0
GRAD_SCALES = (0.1, 1.0, 0.3, 2.0)                           # ~350 values: norms of about 1.9, 19, 5.6, 37 around CLIP = 10
OPTIMIZERS = ("adam", "adamw", "sgd", "adam_onecycle")


class Toy(nn.Module):
    """Six leaf layers — Conv1d, BatchNorm1d, Linear, LayerNorm, BatchNorm1d (three of them inside a Sequential), Linear with a
    FROZEN bias — and `gain`, a parameter that sits directly on the root, a module WITH children: model.parameters() holds it,
    the two groups of `adam_onecycle` do not."""

    def __init__(self):
        super().__init__()
        self.conv = nn.Conv1d(3, 8, 1)
        self.bn1 = nn.BatchNorm1d(8)
        self.block = nn.Sequential(nn.Linear(8, 16), nn.LayerNorm(16), nn.BatchNorm1d(16))
        self.head = nn.Linear(16, 4)
        self.head.bias.requires_grad_(False)
        self.gain = nn.Parameter(torch.ones(4))


def toy(seed=2500):
    """The toy model with every parameter drawn from numpy.random.RandomState(seed), in named_parameters() order."""
    m = Toy()
    rs = np.random.RandomState(seed)
    with torch.no_grad():
        for _, p in m.named_parameters():
            p.copy_(torch.from_numpy((rs.standard_normal(tuple(p.shape)) * 0.5).astype(np.float32)))
    return m


def assign_grads(model, step, held=None):
    """Seeded gradients ASSIGNED to every trainable parameter for (0-based) `step`, scaled by GRAD_SCALES so that clipping at
    CLIP is active on some steps only. held (optional): ids of the parameters the optimizer holds — the others get no gradient,
    so that the norm over model.parameters() (the reference's clip_grad_norm_) is the norm over the optimizer's parameters."""
    rs = np.random.RandomState(7000 + step)
    for _, p in model.named_parameters():
        g = (rs.standard_normal(tuple(p.shape)) * GRAD_SCALES[step % len(GRAD_SCALES)]).astype(np.float32)
        p.grad = torch.from_numpy(g).to(p.device) if p.requires_grad and (held is None or id(p) in held) else None


def optim_cfg(name, easydict):
    """The OPTIMIZATION block of trajectory `name`; adam_onecycle has no SCHEDULER key (OneCycle over 1 epoch x STEPS)."""
    cfg = dict(OPTIMIZER=name, LR=0.01, WEIGHT_DECAY=0.01, BETAS=[0.5, 0.999], EPS=1e-6, MOMENTUM=0.9, GRAD_NORM_CLIP=CLIP,
               SCHEDULER='step', STEP_SIZE=12, GAMMA=0.2)
    if name == "adam_onecycle":
        del cfg['SCHEDULER']
        cfg.update(LR=LR_MAX, MOMS=list(MOMS), DIV_FACTOR=DIV_FACTOR, PCT_START=0.4)
    return easydict(cfg)


def flat_params(model):
    return torch.cat([p.detach().reshape(-1).cpu() for _, p in model.named_parameters()]).numpy()


STATE_KEYS = {"sgd": ("momentum_buffer",)}


def flat_state(model, optimizer, name):
    """{key: the state tensors `key` of every parameter that has state, concatenated in named_parameters() order} + 'step'."""
    keys = STATE_KEYS.get(name, ("exp_avg", "exp_avg_sq"))
    have = [p for _, p in model.named_parameters() if len(optimizer.state.get(p, {})) > 0]
    out = {k: torch.cat([optimizer.state[p][k].reshape(-1).cpu() for p in have]).numpy() for k in keys}
    if name != "sgd":
        out["step"] = np.array([float(optimizer.state[p]["step"]) for p in have])
    return out


def run_trajectory(model, optimizer, scheduler, clip_and_step, device=None):
    """STEPS steps of (scheduler.step(it); assign gradients; clip_and_step()) -> {step number: flat parameters} at RECORD."""
    held = {id(p) for g in optimizer.param_groups for p in g['params']}
    out = {}
    for it in range(STEPS):
        if scheduler is not None:
            scheduler.step(it)
        assign_grads(model, it, held)
        clip_and_step()
        if it + 1 in RECORD:
            out[it + 1] = flat_params(model)
    return out


def _pieces(flat, sizes):
    flat = np.asarray(flat, np.float64)
    assert flat.size == sum(sizes), (flat.size, sum(sizes))
    cuts = np.cumsum([0] + list(sizes))
    return [flat[a:b] for a, b in zip(cuts[:-1], cuts[1:])]


def param_sizes(model):
    return [p.numel() for _, p in model.named_parameters()]


def state_sizes(model, optimizer):
    return [p.numel() for _, p in model.named_parameters() if len(optimizer.state.get(p, {})) > 0]


def params_excess(got, ref, sizes):
    """The bar tests/test_step_ops_gpu.py holds ClipAdam to against torch, tensor by tensor: |got - ref| <= 1e-6 max|ref| + 2e-9.
    -> the largest (difference - bound) over the tensors, and the largest difference."""
    d = [(float(np.abs(g - r).max()), 1e-6 * float(np.abs(r).max()) + 2e-9) for g, r in zip(_pieces(got, sizes), _pieces(ref, sizes))]
    return max(a - b for a, b in d), max(a for a, _ in d)


def moments_excess(got, ref, sizes):
    """Moments within 2e-6 of their scale (the tensor's largest reference value), tensor by tensor."""
    d = [(float(np.abs(g - r).max()), 2e-6 * float(np.abs(r).max()) + 1e-12) for g, r in zip(_pieces(got, sizes), _pieces(ref, sizes))]
    return max(a - b for a, b in d), max(a for a, _ in d)


def group_indices(model, optimizer):
    """Per parameter group: the positions, in named_parameters() order, of its parameters."""
    pos = {id(p): i for i, (_, p) in enumerate(model.named_parameters())}
    return [[pos[id(p)] for p in g['params']] for g in optimizer.param_groups]
