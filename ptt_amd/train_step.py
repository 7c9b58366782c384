"""Data-parallel training step of the full tracker (BASELINE.json configs[3]): one process per GPU, the batch
sharded across ranks, ONE gradient all-reduce per step (4 903 113 fp32 values = 19.6 MB) over RCCL/xGMI.

On a HIP device the gradients of a step live in ONE flat buffer (train_ops.GradSink: every `.grad` is a view of it, filled by
one finishing launch after the backward pass) and the all-reduce is one collective over that buffer — what
DistributedDataParallel does with its single 25-MB bucket (all 19.6 MB become ready with the LAST gradient of the backward
pass, so there is nothing for it to overlap), without the bucket copies and the per-parameter hooks. `reducer="ddp"` (and
every CPU run: the gloo tests) wraps the model in DistributedDataParallel instead.

What it stands in for in the reference: tools/train_tracking.py:158-159 (the DistributedDataParallel wrap — dead
code there because :63 forces dist_train=False, so the reference's `--launcher pytorch` runs N unsynchronised
replicas) and tools/train_utils/train_utils.py:47-51 (model_func -> loss.backward() -> clip_grad_norm_(10) ->
optimizer.step()), with the optimiser of tools/cfgs/kitti_models/ptt.yaml:129-133 (Adam, lr 1e-3, betas 0.5/0.999,
eps 1e-6; ptt/optimization/__init__.py:12-14).

On a HIP device with the flat reducer the step is CAPTURED after `graph_warmup` eager steps and replayed as hipGraphs from then
on (`graph=None`, the default; `graph=False` keeps every step eager): forward + backward + the gradient-finishing launch as one
graph, clip + Adam as a second, the all-reduce issued eagerly between the two (no collective is ever captured: the first run
with more than one RCCL rank is the driver's, and a captured collective is the one thing that could not be tried here). Without
a collective the two are ONE graph. Queuing a step then costs the host two replays instead of ~415 launches through Python and
autograd (12.4 ms -> well under a millisecond), so that eight ranks no longer need eight busy cores and small per-GPU batches
become device-bound. The replayed step is bit-identical to the eager one (tests/test_train_graph_gpu.py).

The same class runs on `gloo` + CPU tensors in the tests (world_size 2) — there the HIP index ops are replaced by
the tests' oracle, because the product ops refuse CPU tensors.
"""
import os
import warnings

import numpy as np
import torch
import torch.distributed as dist

from . import synth
from .optim import ClipAdam, _bump_versions

GRAD_ELEMS = 4903113            # parameters of the shipped PTT model


def synthetic_train_batch(seed, B, device, NS=1024, NT=512, K_s=200, K_t=100):
    """A training batch shaped like KittiTrackingDataset.get_train_items' default-collated output
    (ptt/datasets/kitti/kitti_dataset_tracking.py:60-107): search (B,NS,3), template (B,NT,3), cls_label (B,NS),
    reg_label (B,4). K_s = 200 unique points: nuScenes-Car sparsity. Seeded numpy, so every box
    and backend sees the same numbers."""
    s, t = synth.frames(seed, B, NS, NT, K_s=K_s, K_t=K_t)
    rs = np.random.RandomState(seed + 7919)
    cls = (rs.random_sample((B, NS)) > 0.7).astype(np.float32)
    reg = (rs.standard_normal((B, 4)) * 0.3).astype(np.float32)
    to = lambda a: torch.from_numpy(a).to(device)
    return {'search_points': to(s), 'template_points': to(t), 'batch_size': B, 'cls_label': to(cls), 'reg_label': to(reg)}


def broadcast_module_state(module, buffers_only=False, src=0):
    """Parameters (unless buffers_only) and buffers of `module` on every rank := rank `src`'s, one broadcast per dtype over a
    flattened copy. No-op without a process group of more than one rank."""
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return
    with torch.no_grad():
        tensors = ([] if buffers_only else [p.data for p in module.parameters()]) + [b.data for b in module.buffers()]
        by_type = {}
        for t in tensors:
            by_type.setdefault(t.dtype, []).append(t)
        for ts in by_type.values():
            flat = torch.cat([t.reshape(-1) for t in ts])
            dist.broadcast(flat, src=src)
            off = 0
            for t in ts:
                t.copy_(flat[off:off + t.numel()].view_as(t))
                off += t.numel()
    if not buffers_only:
        from . import train_ops
        train_ops.invalidate_packed()                     # written through .data: the version counters did not move


class _CapturedStep(object):
    """The hipGraphs of one training step for one batch shape, with the static tensors they read and write."""

    def __init__(self, batch):
        self.static = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()}
        self.signature = self._signature(batch)
        self.first, self.second = torch.cuda.CUDAGraph(), None
        self.loss, self.tables, self.optimizer_state, self.packs = None, None, None, None
        self.loss_values = None           # with a ledger: the one-launch losses' (8,) buffer the recorded append reads
        self.ledger = False               # the recorded launches end with the ledger's append
        self.bn_buffers = []              # running statistics the recorded launches update through raw pointers

    @staticmethod
    def _signature(batch):
        return tuple(sorted((k, tuple(v.shape), str(v.dtype), str(v.device)) if torch.is_tensor(v) else (k, v) for k, v in batch.items()))

    def accepts(self, batch):
        return self._signature(batch) == self.signature

    def valid(self, trainer):
        return trainer.optimizer._graph is not None and trainer.optimizer._graph is self.optimizer_state

    def load(self, batch):
        """The batch into the static tensors the graphs read, always copied (one call, four device-to-device copies under 1 MB).
        Neither (data_ptr, _version) nor the tensor's identity tells a new batch from the last one: a batch moved to the device
        after the previous one was freed gets its block back with a fresh version counter, and a raw-pointer writer refills a
        buffer without moving it."""
        keys = [k for k, v in batch.items() if torch.is_tensor(v)]
        torch._foreach_copy_([self.static[k] for k in keys], [batch[k] for k in keys], non_blocking=True)


class DataParallelTrainer(object):
    """model (+ DDP when a process group with more than one rank is initialised) + Adam + gradient clipping.

        trainer = DataParallelTrainer(build_network(...).to(dev).train(), dev)
        loss = trainer.step(batch)          # forward, backward (all-reduce inside), clip, Adam
    """

    def __init__(self, model, device, lr=1e-3, betas=(0.5, 0.999), eps=1e-6, clip=10.0, bucket_cap_mb=25, sync_bn=False, force_ddp=False,
                 reducer=None, graph=None, graph_warmup=3, optimizer=None, scheduler=None, ledger=None):
        """graph: None = replay the step as hipGraphs where that is possible (HIP device, flat reducer, no SyncBatchNorm exchange;
        anything else steps eagerly), True = the same but raise where it is not possible, False = always eager. graph_warmup:
        eager steps before the capture (the plans, tables and workspaces of a step are built by them).
        force_ddp: reduce the gradients over the process group whenever one is initialised, a ONE-rank group included (the
        all-reduce then runs on the device with one participant: how a one-GPU box exercises the multi-GPU code).
        reducer: "flat" (HIP devices, the default there) = train_ops.GradSink + one all-reduce over its buffer; "ddp" =
        DistributedDataParallel (the default, and the only choice, off the HIP device).
        optimizer: None = ClipAdam(lr, betas, eps); otherwise an optimizer instance over the model's parameters or a callable
        model -> optimizer (ptt_amd.optimization.build_optimizer gives the ones of a config's OPTIMIZATION block). One without
        the capture protocol of ptt_amd.optim (a stock torch optimizer) steps eagerly after `clip_grad_norm_`.
        scheduler: an object whose .step(it) is called with the running iteration count at the top of every step(), before the
        optimizer's host half reads lr / betas / momentum (tools/train_utils/train_utils.py:26-27).
        ledger: None = nothing changes; a ptt_amd.fit.StepLedger = every step appends one row (the five loss values of the one-launch
        losses and the gradient norm) to it with one single-wave launch behind the optimizer's update — in the captured step a node
        of the graph, so a per-step loss curve costs no host read. `ledger_fed` turns False (with one warning) where that is not
        possible: a CPU device, or a tracker that took the heads' own losses."""
        self.device = torch.device(device)
        self.world = dist.get_world_size() if (dist.is_available() and dist.is_initialized()) else 1
        collective = self.world > 1 or (force_ddp and dist.is_available() and dist.is_initialized())
        if reducer is None:
            reducer = "flat" if self.device.type == 'cuda' else "ddp"
        if reducer not in ("flat", "ddp") or (reducer == "flat" and self.device.type != 'cuda'):
            raise ValueError("reducer: 'flat' (HIP device) or 'ddp'")
        self.reducer = reducer
        self.collective = collective          # no_sync() switches this off for a scope
        self._collective_cfg = collective     # what the trainer was built with (what a capture records)
        self.ddp = collective and reducer == "ddp"
        if sync_bn and self.world > 1:
            # tools/train_tracking.py:133-134 (--sync_bn). The SharedMLP stages keep running on the hand-written row
            # kernels: their statistics are exchanged as 2C + 1 float64 sums per layer (ptt_amd/train_ops.py)
            model = torch.nn.SyncBatchNorm.convert_sync_batchnorm(model)
        self.tracker = model
        if self.ddp:
            ids = [self.device.index] if self.device.type == 'cuda' else None
            # bucket_cap_mb 25 > 19.6 MB: the whole gradient is one bucket, one all-reduce per step; for a message
            # this small RCCL's direct algorithms over the 7 xGMI links beat a ring
            self.model = torch.nn.parallel.DistributedDataParallel(model, device_ids=ids, bucket_cap_mb=bucket_cap_mb)
        else:
            self.model = model
        # torch.optim.Adam with clip_grad_norm_ folded into step(): two launches on a HIP device, the stock path elsewhere
        if optimizer is None:
            self.optimizer = ClipAdam(self.model.parameters(), lr=lr, betas=betas, eps=eps)
        elif isinstance(optimizer, torch.optim.Optimizer):
            self.optimizer = optimizer
        else:
            self.optimizer = optimizer(self.model)
        self.scheduler = scheduler
        self.epoch_scheduler = None       # from_optim_cfg: a per-epoch schedule ('step'), stepped by the caller's loop (ptt_amd.fit.fit)
        self.iteration = 0                # steps taken: what scheduler.step() is called with
        self._fused_clip = hasattr(self.optimizer, "prepare_graph_step")      # ptt_amd.optim: step(max_norm=...) clips
        self.clip = clip
        self.sink = None
        if reducer == "flat":
            from .train_ops import GradSink
            self.sink = GradSink(list(self.model.parameters()), self.device)
            if self.world > 1:
                self.sync_replicas()
        can_graph = reducer == "flat" and not (sync_bn and self.world > 1)
        if graph and not can_graph:
            raise ValueError("graph=True needs the flat reducer on a HIP device and no SyncBatchNorm exchange inside the step")
        if graph and not self._fused_clip:
            raise ValueError("graph=True needs an optimizer of ptt_amd.optim (the capture protocol); this one steps eagerly")
        self.graph_mode = can_graph and self._fused_clip and graph is not False and os.environ.get("PTT_TRAIN_GRAPH", "1") != "0"
        self.graph_warmup = max(1, int(graph_warmup))
        self.eager_steps = 0
        self.captured = None              # _CapturedStep once the step has been captured
        self.graph_steps = 0
        self._capture_misses = 0
        self.ledger = ledger
        self.ledger_fed = ledger is not None and self.device.type == 'cuda'
        self.tb_dict = None               # the tb_dict of the last EAGER forward pass (a replay has none: None then)
        self._loss_values = None          # with a ledger: the one-launch losses' device values of the step being run or recorded

    def sync_replicas(self, buffers_only=False):
        """Every parameter and buffer (BatchNorm running statistics, num_batches_tracked) takes rank 0's value — what
        DistributedDataParallel does at construction, and for the buffers before every forward pass. The flat reducer calls it once
        at construction, so that ranks which built their models under different seeds still train ONE model; afterwards the
        parameters stay equal by construction (same averaged gradients, same update), while the running statistics are PER RANK
        (each rank's own shard of the batches, as in the reference's unsynchronised `--launcher pytorch` replicas): call
        sync_replicas(buffers_only=True) before evaluating or checkpointing from a rank other than 0 if that matters."""
        broadcast_module_state(self.tracker, buffers_only)

    def _local_forward_backward(self, batch):
        """This rank's loss and gradients, finished into the sink's flat buffer (flat reducer only)."""
        ret, tb_dict, _ = self.model(dict(batch))
        self.tb_dict = tb_dict
        self._note_loss_values(tb_dict)
        loss = ret['loss'] if ret['loss'].dim() == 0 else ret['loss'].mean()
        with self.sink.collecting():
            loss.backward()
        self.sink.flush()
        return loss

    def _note_loss_values(self, tb_dict):
        """With a ledger: the device tensor behind the tb_dict's train_ops.LossValues numbers (held here so that its memory
        outlives the backward pass — inside a capture it is what the recorded append reads on every replay); None where the
        tracker took the heads' own losses."""
        if self.ledger is None:
            return
        owner = getattr(next(iter(tb_dict.values()), None), "owner", None) if isinstance(tb_dict, dict) else None
        values = getattr(owner, "device_values", None)
        self._loss_values = values if (torch.is_tensor(values) and values.is_cuda and values.dtype == torch.float32) else None

    def _ledger_norm(self, norm):
        return norm.reshape(-1) if (torch.is_tensor(norm) and norm.is_cuda and norm.dtype == torch.float32 and norm.numel() == 1) else None

    def _ledger_unfed(self):
        if self.ledger_fed:
            self.ledger_fed = False
            warnings.warn("DataParallelTrainer: the step ledger cannot be fed (no one-launch loss values on a HIP device); "
                          "read loss.item() per step instead")

    def _reduce(self):
        # the mean over ranks, as DistributedDataParallel forms it: one all-reduce of the whole gradient
        dist.all_reduce(self.sink.flat)

    def forward_backward(self, batch):
        """loss.mean() and its gradients (averaged over ranks); no optimiser step."""
        if self.sink is None:
            ret, tb_dict, _ = self.model(dict(batch))
            self.tb_dict = tb_dict
            self._note_loss_values(tb_dict)
            loss = ret['loss'] if ret['loss'].dim() == 0 else ret['loss'].mean()
            self.optimizer.zero_grad(set_to_none=True)
            loss.backward()
            return loss
        loss = self._local_forward_backward(batch)
        if self.collective:
            self._reduce()
            if self.world > 1:
                self.sink.flat.mul_(1.0 / self.world)
        return loss

    def step(self, batch):
        """One training step; returns the loss (a 0-dim device tensor — in graph mode the SAME tensor every step, holding the
        latest step's value once the device gets there)."""
        if self.scheduler is not None:
            self.scheduler.step(self.iteration)
        self.iteration += 1
        if self.graph_mode:
            if self.captured is not None and not self.captured.valid(self):
                self.captured = None                          # e.g. optimizer.load_state_dict(): new moment tensors
            if self.captured is None and self.eager_steps >= self.graph_warmup:
                self._capture(batch)
            if self.captured is not None and self.captured.accepts(batch):
                return self._replay(batch)
        loss = self.forward_backward(batch)
        norm = None
        if self._fused_clip:
            self.optimizer.step(max_norm=self.clip if self.clip else None)
            norm = self.optimizer.last_norm if self.clip else None
        else:
            if self.clip:
                norm = torch.nn.utils.clip_grad_norm_(self.model.parameters(), self.clip)
            self.optimizer.step()
        if self.ledger is not None:
            if self.ledger_fed and self._loss_values is not None:
                self.ledger.append(self._loss_values, self._ledger_norm(norm))
            else:
                self._ledger_unfed()
            self._loss_values = None
        self.tracker.update_global_step()
        self.eager_steps += 1
        return loss

    @classmethod
    def from_optim_cfg(cls, model, device, optim_cfg, total_iters_each_epoch, total_epochs, **kw):
        """The trainer of a config's OPTIMIZATION block: build_optimizer / build_scheduler of ptt_amd.optimization and
        GRAD_NORM_CLIP (tools/train_tracking.py:161-167 with train_utils.py:26-51). kw: the other constructor arguments."""
        from .optimization import build_optimizer, build_scheduler
        trainer = cls(model, device, clip=optim_cfg.get('GRAD_NORM_CLIP', 10.0), optimizer=lambda m: build_optimizer(m, optim_cfg), **kw)
        sched, _ = build_scheduler(trainer.optimizer, total_iters_each_epoch, total_epochs, -1, optim_cfg)
        # OneCycle (no SCHEDULER key) is stepped per iteration, by step(); a 'step' schedule per EPOCH, by the caller's loop
        # (train_utils.py:116-117): trainer.epoch_scheduler.step() after each epoch
        trainer.scheduler, trainer.epoch_scheduler = (sched, None) if optim_cfg.get('SCHEDULER', None) is None else (None, sched)
        return trainer

    # ------------------------------------------------------------------------------------------------ the captured step
    def _capture(self, batch):
        """Records the step for batches shaped like `batch` (other shapes keep stepping eagerly). Nothing is executed here: the
        caller replays. A capture that fails turns graph mode off (with a warning) and the trainer continues eagerly."""
        from . import ops, train_ops
        if not self.optimizer.prepare_graph_step():
            # e.g. right after optimizer.load_state_dict(): the next eager step rebuilds the optimizer's table, then this succeeds
            self._capture_misses += 1
            if self._capture_misses > 3:
                self.graph_mode = False
                warnings.warn("DataParallelTrainer: the optimizer is not in the one-table state a captured step needs; stepping eagerly")
            return
        self._capture_misses = 0
        clip = self.clip if self.clip else None
        cap = _CapturedStep(batch)
        try:
            # what the recorded launches read besides tensors of the step itself is built NOW, eagerly, and belongs to the capture:
            # the finishing launch's job table and the weight-packing launch's table (nothing the eager code touches afterwards)
            self.sink.plan.prepare_capture()
            cap.packs = train_ops.PackCapture(list(self.model.parameters()), self.device)
            torch.cuda.synchronize(self.device)
            # capture_error_mode "thread_local": calls other threads make while this one records (RCCL's watchdog polling its events,
            # a data loader pinning memory) neither fail nor invalidate the capture; the autograd thread's launches are recorded all the
            # same — capturing is a property of the stream
            with cap.packs, torch.cuda.graph(cap.first, capture_error_mode="thread_local"):
                cap.loss = self._local_forward_backward(cap.static)
                cap.loss_values = self._loss_values
                if not self._collective_cfg:
                    self.optimizer.record_graph_step(clip)
                    self._record_ledger(cap, clip)
            if self._collective_cfg:
                cap.second = torch.cuda.CUDAGraph()
                with cap.packs, torch.cuda.graph(cap.second, pool=cap.first.pool(), capture_error_mode="thread_local"):
                    if self.world > 1:
                        self.sink.flat.mul_(1.0 / self.world)
                    self.optimizer.record_graph_step(clip)
                    self._record_ledger(cap, clip)
            cap.tables = ops.finish_capture_uploads()
        except Exception as e:                                # noqa: BLE001 — whatever the runtime refuses, the eager step still works
            ops.finish_capture_uploads()
            self.graph_mode = False
            warnings.warn("DataParallelTrainer: capturing the training step failed (%s: %s); stepping eagerly" % (type(e).__name__, e))
            return
        cap.optimizer_state = self.optimizer._graph
        cap.bn_buffers = [t for m in self.tracker.modules()
                          if isinstance(m, torch.nn.modules.batchnorm._BatchNorm) and m.training and m.track_running_stats
                          for t in (m.running_mean, m.running_var, m.num_batches_tracked) if t is not None]
        self.captured = cap

    def _record_ledger(self, cap, clip):
        """The ledger's append as a node of the graph being recorded, behind the optimizer's update (the row needs its norm)."""
        if self.ledger is not None and self.ledger_fed and cap.loss_values is not None:
            self.ledger.record(cap.loss_values, self._ledger_norm(self.optimizer.last_norm) if clip is not None else None)
            cap.ledger = True

    def _replay(self, batch):
        cap = self.captured
        self.tb_dict = None
        cap.load(batch)
        self.optimizer.begin_graph_step(self.clip if self.clip else None)
        cap.first.replay()
        if cap.second is not None:
            if self.collective:                               # False inside no_sync(): a timing scope — the 1 / world scaling stays
                self._reduce()
            cap.second.replay()
        self.optimizer.end_graph_step()
        # the replay moved the running statistics through raw pointers; the eval-mode parameter caches key on their versions
        _bump_versions(cap.bn_buffers)
        if self.ledger is not None:
            if cap.ledger:
                self.ledger.replayed()
            else:
                self._ledger_unfed()
        self.tracker.update_global_step()
        self.graph_steps += 1
        return cap.loss

    def no_sync(self):
        """Steps inside this scope keep their gradients local (DistributedDataParallel.no_sync(), or the flat reducer's
        all-reduce skipped): what bench.py times to see how much of the all-reduce a step does not hide."""
        if self.ddp:
            return self.model.no_sync()
        trainer = self

        class _Scope(object):
            def __enter__(self):
                self.was, trainer.collective = trainer.collective, False

            def __exit__(self, *exc):
                trainer.collective = self.was
        return _Scope()

    def grad_bytes_allreduced(self):
        """Bytes of gradient one step hands to the bucket all-reduce (0 without DDP): every parameter that requires a gradient."""
        if not self.collective:
            return 0
        return sum(p.numel() * p.element_size() for p in self.model.parameters() if p.requires_grad)

    def ranks_seen(self):
        """All-reduce of ones: how many ranks actually take part in the collective."""
        if not self.collective:
            return 1
        one = torch.ones(1, device=self.device)
        dist.all_reduce(one)
        return int(one.item())
