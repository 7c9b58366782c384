"""The OPTIMIZATION block of a reference config (tools/train_utils/optimization/__init__.py): build_optimizer and
build_scheduler under the reference's names and signatures, returning this project's optimizers (ptt_amd/optim.py: clip + update
in two launches on a HIP device, the stock torch path elsewhere).

    OPTIMIZER      adam -> ClipAdam, adamw -> ClipAdamW, sgd -> ClipSGD, adam_onecycle -> OneCycleAdamW (two parameter groups)
    SCHEDULER      absent -> OneCycle (stepped once per ITERATION: train_utils.py:26-27), 'step' -> torch's StepLR

`adam_onecycle` in the reference is fastai's OptimWrapper around torch.optim.Adam(betas=(0.9, 0.99)) with true_wd=True, bn_wd=True:
before every Adam step it multiplies every trainable parameter of both groups by 1 - wd * lr and runs Adam with weight_decay 0
(fastai_optim.py:132-149). That is torch.optim.AdamW's update, so OneCycleAdamW IS a ClipAdamW over the same two groups.

One departure: a trainable parameter that received NO gradient is left untouched here (torch.optim.AdamW's rule), while OptimWrapper
would still decay it. No shipped model has such a parameter.
"""
import math

import torch
import torch.nn as nn

from .optim import ClipAdam, ClipAdamW, ClipSGD

BN_TYPES = (nn.BatchNorm1d, nn.BatchNorm2d, nn.BatchNorm3d, nn.SyncBatchNorm)


def _set_lr(optimizer, value):
    for g in optimizer.param_groups:
        g['lr'] = float(value)


def _set_mom(optimizer, value):
    """beta1 of an Adam-like optimizer, `momentum` of an SGD-like one, on every group."""
    for g in optimizer.param_groups:
        if 'betas' in g:
            g['betas'] = (float(value), g['betas'][1])
        elif 'momentum' in g:
            g['momentum'] = float(value)


def onecycle_param_groups(model):
    """The reference's two groups, in its order: the parameters (requires_grad only) of the LEAF modules of `model` — modules
    without children, in traversal order — that are not BatchNorm, then those of the BatchNorm leaves. A parameter that sits
    directly on a module WITH children belongs to no leaf and is not collected, as in the reference."""
    groups, seen = ([], []), set()
    for m in model.modules():
        if next(m.children(), None) is not None:
            continue
        dst = groups[1] if isinstance(m, BN_TYPES) else groups[0]
        for p in m.parameters(recurse=False):
            if p.requires_grad and id(p) not in seen:
                seen.add(id(p))
                dst.append(p)
    return list(groups)


class OneCycleAdamW(ClipAdamW):
    """The `adam_onecycle` optimizer: ClipAdamW(betas=(0.9, 0.99)) over onecycle_param_groups(model) with the hyper-parameters as
    the attributes the reference's training loop and its OneCycle schedule use — .lr, .mom (beta1), .wd read the last group and
    write EVERY group (both groups always hold the same values: bn_wd=True)."""

    def __init__(self, model, lr=3e-3, wd=0.0):
        # torch refuses an empty group only when NO group has parameters; an empty BatchNorm group is kept, as the reference keeps it
        super().__init__([{'params': ps} for ps in onecycle_param_groups(model)], lr=lr, betas=(0.9, 0.99), weight_decay=wd)

    @property
    def lr(self):
        return self.param_groups[-1]['lr']

    @lr.setter
    def lr(self, value):
        _set_lr(self, value)

    @property
    def mom(self):
        return self.param_groups[-1]['betas'][0]

    @mom.setter
    def mom(self, value):
        _set_mom(self, value)

    @property
    def wd(self):
        return self.param_groups[-1]['weight_decay']

    @wd.setter
    def wd(self, value):
        for g in self.param_groups:
            g['weight_decay'] = float(value)


def build_optimizer(model, optim_cfg):
    name = optim_cfg.OPTIMIZER
    if name == 'adam':
        return ClipAdam(model.parameters(), lr=optim_cfg.LR, weight_decay=optim_cfg.WEIGHT_DECAY, betas=tuple(optim_cfg.BETAS),
                        eps=float(optim_cfg.EPS))
    if name == 'adamw':
        return ClipAdamW(model.parameters(), lr=optim_cfg.LR, weight_decay=optim_cfg.WEIGHT_DECAY, betas=tuple(optim_cfg.BETAS),
                         eps=float(optim_cfg.EPS), amsgrad=False)
    if name == 'sgd':
        return ClipSGD(model.parameters(), lr=optim_cfg.LR, weight_decay=optim_cfg.WEIGHT_DECAY, momentum=optim_cfg.MOMENTUM)
    if name == 'adam_onecycle':
        return OneCycleAdamW(model, lr=3e-3, wd=optim_cfg.WEIGHT_DECAY)
    raise NotImplementedError("OPTIMIZATION.OPTIMIZER: %r (adam, adamw, sgd or adam_onecycle)" % (name,))


def _cos_anneal(start, end, pct):
    return end + (start - end) / 2 * (math.cos(math.pi * pct) + 1)


class OneCycle(object):
    """The one-cycle schedule of learning_schedules_fastai.py:60-77, stepped once per iteration with the iteration number: the lr
    rises from lr_max / div_factor to lr_max over the first int(total_step * pct_start) steps and falls to lr_max / div_factor /
    1e4 over the rest, both on half a cosine; the momentum (beta1, or SGD's momentum) runs moms[0] -> moms[1] -> moms[0] on the
    same two phases. Every parameter group receives both values."""

    def __init__(self, optimizer, total_step, lr_max, moms, div_factor, pct_start):
        self.optimizer = optimizer
        self.total_step = total_step
        self.lr_max, self.moms, self.div_factor, self.pct_start = lr_max, tuple(moms), div_factor, pct_start
        self.boundary = int(total_step * pct_start)         # the first step of the falling phase
        self.low_lr = lr_max / div_factor
        _set_lr(optimizer, self.low_lr)
        _set_mom(optimizer, self.moms[0])

    def values(self, it):
        """(lr, momentum) of iteration `it`."""
        if it >= self.boundary:                              # the later phase wins, as in the reference's loop over the phases
            pct = (it - self.boundary) / (self.total_step - self.boundary)
            return _cos_anneal(self.lr_max, self.low_lr / 1e4, pct), _cos_anneal(self.moms[1], self.moms[0], pct)
        pct = it / self.boundary
        return _cos_anneal(self.low_lr, self.lr_max, pct), _cos_anneal(self.moms[0], self.moms[1], pct)

    def step(self, it):
        lr, mom = self.values(it)
        _set_lr(self.optimizer, lr)
        _set_mom(self.optimizer, mom)


def build_scheduler(optimizer, total_iters_each_epoch, total_epochs, last_epoch, optim_cfg):
    """-> (scheduler, None): the reference returns a pair whose second member (a warm-up scheduler) it never builds."""
    kind = optim_cfg.get('SCHEDULER', None)
    if kind is None:
        return OneCycle(optimizer, total_iters_each_epoch * total_epochs, optim_cfg.LR, list(optim_cfg.MOMS), optim_cfg.DIV_FACTOR,
                        optim_cfg.PCT_START), None
    if kind == 'step':
        return torch.optim.lr_scheduler.StepLR(optimizer, step_size=optim_cfg.STEP_SIZE, gamma=optim_cfg.GAMMA), None
    raise NotImplementedError("OPTIMIZATION.SCHEDULER: %r (absent for OneCycle, or 'step')" % (kind,))
