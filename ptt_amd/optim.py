"""Gradient clipping + Adam of the training step (reference tools/train_utils/train_utils.py:47-51:
`clip_grad_norm_(model.parameters(), GRAD_NORM_CLIP); optimizer.step()` with the optimizer of
tools/train_utils/optimization/__init__.py:12-14) as TWO launches over a device table of all parameters
(ptt_adam_clip_step_f32, ptt_amd/csrc/step_ops.hip) instead of torch's ~25 multi-tensor launches.

ClipAdam IS a torch.optim.Adam: same constructor, same param_groups, same state keys ('step', 'exp_avg', 'exp_avg_sq'), so
state_dict() / load_state_dict() interchange with the stock optimizer and LR schedulers drive it unchanged. Only step() differs:
`step(max_norm=10.0)` clips and updates in one pass. Whatever the table does not take (several param groups with different
hyper-parameters are fine; amsgrad / maximize / non-float32 / CPU parameters are not) runs on the stock path.

ClipAdamW and ClipSGD are the same for torch.optim.AdamW and torch.optim.SGD (the other OPTIMIZER values of
tools/train_utils/optimization/__init__.py:15-35) on ptt_optim_clip_step_f32: rows of ALL parameter groups in one table under
one norm, the hyper-parameters an array with one entry per group — so the reference's two-group `adam_onecycle` optimizer, whose
schedule moves lr and beta1 on every step, keeps the two-launch step and its captured form."""
import ctypes
import math

import torch

from . import _lib, ops


def _bump_versions(params):
    """The launch updated the parameters through raw pointers: tell autograd (saved-tensor checks) and every cache keyed on
    `_version` (train_ops.packed: the MFMA weight packs) that they changed, as an in-place torch op would have."""
    try:
        torch._C._autograd._unsafe_set_version_counter(params, [p._version + 1 for p in params])
    except (AttributeError, TypeError):
        torch._foreach_add_(params, 0.0)             # older torch: a real (multi-tensor) in-place op


def _on_table(params):
    """float32, contiguous, dense, on ONE HIP device, gradients included: what a device table of raw pointers can address."""
    return len(params) > 0 and all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and p.grad.dtype == torch.float32
                                   and not p.grad.is_sparse and p.grad.is_contiguous() and p.device == params[0].device for p in params)


class ClipAdam(torch.optim.Adam):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, foreach=True)
        self._tables = {}                 # group index -> (ids of the parameters in the table, ops.AdamTable)
        self.last_norm = None             # the total gradient norm of the last clipped step: a (1,) device tensor
        self._ring = None                 # ops.AdamHyperRing of the captured form of the step
        self._graph = None                # (group, params, table, step counters) pinned by prepare_graph_step()

    def _fusable(self, group, params):
        return (not group['amsgrad'] and not group.get('maximize', False) and not group.get('capturable', False)
                and not group.get('differentiable', False) and _on_table(params))

    @torch.no_grad()
    def step(self, closure=None, max_norm=None):
        """max_norm: clip the global gradient norm first (torch.nn.utils.clip_grad_norm_ over ALL parameters of the optimizer)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        groups = [(gi, g, [p for p in g['params'] if p.grad is not None]) for gi, g in enumerate(self.param_groups)]
        one_table = len(groups) == 1 and self._fusable(groups[0][1], groups[0][2])
        if not one_table:
            # several groups share one norm: clip with torch, then update every group that qualifies without clipping
            if max_norm is not None:
                self.last_norm = torch.nn.utils.clip_grad_norm_([p for _, _, ps in groups for p in ps], max_norm)
            max_norm = None
        for gi, group, params in groups:
            if not params:
                continue
            if not self._fusable(group, params):
                self._stock_group(group)
                continue
            for p in params:
                st = self.state[p]
                if len(st) == 0:
                    st['step'] = torch.tensor(0.0, dtype=torch.float32)
                    st['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
            steps = [self.state[p]['step'] for p in params]
            if any(s.is_cuda for s in steps):
                self._stock_group(group)
                continue
            torch._foreach_add_(steps, 1)
            t = float(steps[0])
            if float(steps[-1]) != t:
                raise RuntimeError("ClipAdam: parameters of one group at different step counts")
            key = tuple((id(p), p.data_ptr()) for p in params)      # a moved parameter (model.to(...), p.data = ...) rebuilds the table
            cached = self._tables.get(gi)
            if cached is None or cached[0] != key:
                cached = (key, ops.AdamTable(params, [self.state[p]['exp_avg'] for p in params], [self.state[p]['exp_avg_sq'] for p in params]))
                self._tables[gi] = cached
            beta1, beta2 = group['betas']
            lr = float(group['lr'])
            norm = cached[1].step([p.grad for p in params], beta1, beta2, group['eps'], lr / (1.0 - beta1 ** t), math.sqrt(1.0 - beta2 ** t),
                                  group['weight_decay'], max_norm if max_norm is not None else 0.0)
            if max_norm is not None:
                self.last_norm = norm
            _bump_versions(params)
        return loss

    # ------------------------------------------------------------------ the step in two halves, for a captured training step
    def _graph_table(self):
        """(group, params, AdamTable) when the whole optimizer is ONE table that has already stepped eagerly (state, table and
        gradient addresses exist) — the precondition of the captured form; None otherwise."""
        if len(self.param_groups) != 1:
            return None
        group = self.param_groups[0]
        params = [p for p in group['params'] if p.grad is not None]
        cached = self._tables.get(0)
        if not params or cached is None or not self._fusable(group, params):
            return None
        if cached[0] != tuple((id(p), p.data_ptr()) for p in params) or not cached[1].check_grads_in_place([p.grad for p in params]):
            return None
        return group, params, cached[1]

    def prepare_graph_step(self):
        """Before a capture: checks the one-table state and pins it (the per-step halves below do no checking of their own — they
        run once per replay). False when the optimizer cannot take the captured form (it then steps eagerly)."""
        hit = self._graph_table()
        if hit is None:
            self._graph = None
            return False
        group, params, table = hit
        if self._ring is None:
            self._ring = ops.AdamHyperRing(table.device)
        self._graph = (group, params, table, [self.state[p]['step'] for p in params])
        return True

    def begin_graph_step(self, max_norm=None):
        """Host half of a captured step, BEFORE the replay: the step counters advance and this step's hyper-parameters (the lr of
        the moment, the bias corrections) go to the device struct the recorded launches read."""
        group, params, table, steps = self._graph
        torch._foreach_add_(steps, 1)
        t = float(steps[0])
        beta1, beta2 = group['betas']
        self._ring.upload(table.hyper(beta1, beta2, group['eps'], float(group['lr']) / (1.0 - beta1 ** t), math.sqrt(1.0 - beta2 ** t),
                                      group['weight_decay'], max_norm if max_norm is not None else 0.0))

    def record_graph_step(self, max_norm=None):
        """Device half: the two launches, reading the device struct (called while the stream is capturing)."""
        table = self._graph[2]
        norm = table.step_device_hyper(self._ring.dev, clip=max_norm is not None)
        if max_norm is not None:
            self.last_norm = norm

    def end_graph_step(self):
        """Host half AFTER the replay was queued: the parameters changed under autograd's feet, and a torch LRScheduler attached
        to this optimizer must see that a step happened (it tracks calls of step(), which a replay never makes)."""
        _bump_versions(self._graph[1])
        self._opt_called = True

    def _stock_group(self, group):
        saved = self.param_groups
        try:
            self.param_groups = [group]
            torch.optim.Adam.step(self)
        finally:
            self.param_groups = saved

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._graph = None
        self._tables = {}                 # the moments are new tensors


class _GroupTableStep(object):
    """step() and the four-call capture protocol of ClipAdamW / ClipSGD: every parameter group in ONE ops.OptimTable under one
    norm. The subclass says which group the table takes (_group_fusable), makes a parameter's state (_init_state -> the two state
    tensors of its row; True when it made them), advances a group by one step and returns its hyper-parameter entry (_advance),
    and names its stock class (_stock)."""

    def _init_table_step(self):
        self._table = None                # (key, ops.OptimTable)
        self.last_norm = None             # the total gradient norm of the last clipped step: a (1,) device tensor
        self._ring = None                 # ops.AdamHyperRing holding one OptimHyper per group
        self._graph = None                # (params, table, groups) pinned by prepare_graph_step()

    def _rows(self):
        """[(group index, parameter)] of every parameter that has a gradient, in param_groups order."""
        return [(gi, p) for gi, g in enumerate(self.param_groups) for p in g['params'] if p.grad is not None]

    def _fusable(self, rows):
        from ._lib import PTT_OPTIM_MAX_GROUPS
        return (len(self.param_groups) <= PTT_OPTIM_MAX_GROUPS and _on_table([p for _, p in rows])
                and all(self._group_fusable(g) for g in self.param_groups))

    def _key(self, rows):
        return tuple((gi, id(p), p.data_ptr()) + tuple(id(t) for t in self._state_tensors(p)) for gi, p in rows)

    def _build(self, rows):
        """(table of `rows`, groups on their first step). State is created here where it is missing; the table is cached until
        a parameter or a state tensor moves."""
        total, made = {}, {}
        for gi, p in rows:
            total[gi] = total.get(gi, 0) + 1
            if self._init_state(self.param_groups[gi], p):
                made[gi] = made.get(gi, 0) + 1
        fresh = {gi for gi, n in made.items() if n == total[gi]}      # groups on their first step: ALL their state is new
        key = self._key(rows)
        if self._table is None or self._table[0] != key:
            st = [self._state_tensors(p) for _, p in rows]
            self._table = (key, ops.OptimTable([p for _, p in rows], [a for a, _ in st], [b for _, b in st], [gi for gi, _ in rows],
                                               len(self.param_groups)))
            self._graph = None
        return self._table[1], fresh

    @torch.no_grad()
    def step(self, closure=None, max_norm=None):
        """max_norm: clip the global gradient norm first (torch.nn.utils.clip_grad_norm_ over ALL parameters of the optimizer)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        rows = self._rows()
        if not rows:
            return loss
        if not self._fusable(rows):
            if max_norm is not None:
                self.last_norm = torch.nn.utils.clip_grad_norm_([p for _, p in rows], max_norm)
            self._stock.step(self)
            return loss
        table, fresh = self._build(rows)
        hypers = [self._advance(gi, g, [p for k, p in rows if k == gi], gi in fresh) for gi, g in enumerate(self.param_groups)]
        norm = table.step([p.grad for _, p in rows], hypers, max_norm if max_norm is not None else 0.0)
        if max_norm is not None:
            self.last_norm = norm
        _bump_versions([p for _, p in rows])
        return loss

    # ------------------------------------------------------------------ the step in two halves, for a captured training step
    def prepare_graph_step(self):
        """Before a capture: True when every group is in the ONE table that has already stepped eagerly (state, table and gradient
        addresses exist); pins that state. False: the optimizer steps eagerly."""
        self._graph = None
        rows = self._rows()
        if not rows or self._table is None or not self._fusable(rows):
            return False
        key, table = self._table
        if any(self._needs_state(self.param_groups[gi]) and self._state_tensors(p)[0] is None for gi, p in rows):
            return False
        if key != self._key(rows) or not table.check_grads_in_place([p.grad for _, p in rows]):
            return False
        if self._ring is None or self._ring.dev.numel() != ctypes.sizeof(_lib.OptimHyper) * table.n_groups:
            self._ring = ops.AdamHyperRing(table.device, nbytes=ctypes.sizeof(_lib.OptimHyper) * table.n_groups)
        params = [p for _, p in rows]
        self._graph = (params, table, [[p for k, p in rows if k == gi] for gi in range(len(self.param_groups))])
        return True

    def begin_graph_step(self, max_norm=None):
        """Host half of a captured step, BEFORE the replay: every group advances and its hyper-parameters of the moment (lr, betas
        or momentum, weight decay as a scheduler left them; the bias corrections) go to the device array the recorded launches
        read. max_norm is fixed by record_graph_step()."""
        _, table, per_group = self._graph
        self._ring.upload(table.hyper_array([self._advance(gi, g, per_group[gi], False) for gi, g in enumerate(self.param_groups)]))

    def record_graph_step(self, max_norm=None):
        """Device half: the two launches, reading the device array (called while the stream is capturing)."""
        norm = self._graph[1].step_device_hyper(self._ring.dev, max_norm if max_norm is not None else 0.0)
        if max_norm is not None:
            self.last_norm = norm

    def end_graph_step(self):
        """Host half AFTER the replay was queued (see ClipAdam.end_graph_step)."""
        _bump_versions(self._graph[0])
        self._opt_called = True

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._graph = None
        self._table = None                # the state tensors are new


class ClipAdamW(_GroupTableStep, torch.optim.AdamW):
    """torch.optim.AdamW (decoupled weight decay: p *= 1 - lr wd, then Adam) with clip_grad_norm_ folded into step(). With
    `betas=(0.9, 0.99)` and two groups it is what the reference's OptimWrapper(true_wd=True) over Adam computes
    (optimization.build_optimizer, 'adam_onecycle')."""
    _stock = torch.optim.AdamW

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, foreach=True)
        self._init_table_step()

    def _group_fusable(self, group):
        return (not group['amsgrad'] and not group.get('maximize', False) and not group.get('capturable', False)
                and not group.get('differentiable', False) and not torch.is_tensor(group['lr']))

    def _needs_state(self, group):
        return True

    def _state_tensors(self, p):
        st = self.state.get(p)
        return (st['exp_avg'], st['exp_avg_sq']) if st else (None, None)

    def _init_state(self, group, p):
        st = self.state[p]
        if len(st) == 0:
            st['step'] = torch.tensor(0.0, dtype=torch.float32)
            st['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
            return True
        if st['step'].is_cuda:
            st['step'] = st['step'].cpu()     # a capturable optimizer's state_dict: the table's step counters live on the host
        return False

    def _advance(self, gi, group, params, fresh):
        if not params:                                      # a group without gradients: its entry is never read
            return ops.OptimTable.hyper("adamw", 0.0)
        steps = [self.state[p]['step'] for p in params]
        torch._foreach_add_(steps, 1)
        t = float(steps[0])
        if float(steps[-1]) != t:
            raise RuntimeError("ClipAdamW: parameters of one group at different step counts")
        return ops.OptimTable.hyper("adamw", group['lr'], t, group['betas'], group['eps'], group['weight_decay'])


class ClipSGD(_GroupTableStep, torch.optim.SGD):
    """torch.optim.SGD (momentum, L2 weight decay; no dampening, no nesterov on the table) with clip_grad_norm_ folded into step()."""
    _stock = torch.optim.SGD

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False):
        super().__init__(params, lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov, foreach=True)
        self._init_table_step()

    def _group_fusable(self, group):
        return (not group['nesterov'] and group['dampening'] == 0 and not group.get('maximize', False)
                and not group.get('differentiable', False) and not torch.is_tensor(group['lr']))

    def _needs_state(self, group):
        return group['momentum'] != 0

    def _state_tensors(self, p):
        return (self.state.get(p, {}).get('momentum_buffer'), None)

    def _init_state(self, group, p):
        if group['momentum'] == 0 or self.state[p].get('momentum_buffer') is not None:
            return False
        # torch makes the buffer a clone of the first gradient; the launch writes exactly that into it (first_step)
        self.state[p]['momentum_buffer'] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return True

    def _advance(self, gi, group, params, fresh):
        if group['momentum'] != 0 and any(self.state[p].get('momentum_buffer') is None for p in params):
            raise RuntimeError("ClipSGD: momentum switched on under a captured step; step eagerly once first")
        return ops.OptimTable.hyper("sgd", group['lr'], weight_decay=group['weight_decay'], momentum=group['momentum'], first_step=fresh)
