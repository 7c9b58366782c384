"""fit(): the reference's training driver (tools/train_utils/train_utils.py:train_model with tools/train_tracking.py:139-165) on
this project's parts — epochs over a TrainBatchFeeder, DataParallelTrainer.step per batch, the per-epoch 'step' schedule,
checkpoint save / rotate / auto-resume under the reference's file names and keys, TRAIN.WITH_EVAL through PackedTrackletRunner +
eval_metrics.evaluate, and loss / lr logging under the reference's tensorboard names.

What cannot be transcribed is the logging: the reference calls loss.item() and reads four tb_dict values on EVERY step
(train_utils.py:54-70), i.e. it waits for the device once per step. The captured training step returns the same 0-dim tensor
every step and its loss buffer is overwritten by the next replay, so reading it per step would give back the 0.3 ms of host time
the replay was built for. StepLedger is the answer: the step itself appends [total, seed cls, seed reg, proposal cls, proposal
reg, gradient norm] to a ring in device memory with one single-wave launch (ptt_step_ledger_f32, a node of the step's hipGraph),
and fit() fetches the ring with ONE copy every `log_interval` steps. Every step's values still reach the logger, each under its
own iteration number — later, not fewer.
"""
import glob
import os
import warnings

import numpy as np
import torch
import torch.distributed as dist

LEDGER_COLS = 6
COLUMNS = ('loss', 'centroids_cls_loss', 'centroids_reg_loss', 'boxes_cls_loss', 'boxes_reg_loss', 'grad_norm')
CHECKPOINT_KEYS = ('epoch', 'it', 'model_state', 'optimizer_state', 'version')


# --------------------------------------------------------------------------------------------------------------- the ledger
def unwrap_ring(ring, appended, fetched):
    """The rows of a (capacity, C) ring that were appended after the first `fetched` ones, oldest first: row k lives in slot
    k % capacity. -> (rows (n, C), dropped): dropped = how many of the appended - fetched pending rows were overwritten before
    this call (the pending rows beyond the ring's capacity; the oldest ones)."""
    ring = np.asarray(ring)
    capacity = ring.shape[0]
    appended, fetched = int(appended), int(fetched)
    if fetched > appended or fetched < 0:
        raise ValueError("unwrap_ring: fetched=%d outside 0..appended=%d" % (fetched, appended))
    pending = appended - fetched
    dropped = max(0, pending - capacity)
    k = np.arange(appended - (pending - dropped), appended, dtype=np.int64)
    return ring[k % capacity].copy(), dropped


class StepLedger(object):
    """A ring of the last `capacity` training steps' scalars and running statistics over all of them, in device memory.

        ledger = StepLedger(dev)
        trainer = DataParallelTrainer(model, dev, ledger=ledger)       # every step appends its row: no host read
        ...
        rows, dropped = ledger.fetch()                                 # (n, 6) float32 since the last fetch, oldest first

    Row = COLUMNS. State on the device: int64 appended, int64 non_finite (rows holding an inf / NaN), float64 sum[6] over the
    finite rows in append order. Ring and state are ONE buffer, so a fetch is one device-to-host copy."""

    def __init__(self, device, capacity=1024):
        from . import ops                                              # loads the library: a ledger exists on a HIP device only
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise ValueError("StepLedger lives on a HIP device; on the CPU fit() reads loss.item() per step")
        self.capacity = int(capacity)
        if self.capacity < 1:
            raise ValueError("StepLedger: capacity must be >= 1, got %d" % self.capacity)
        self._ops = ops
        # 8 state words of 8 bytes (appended, non_finite, sum[6]), then the ring: int32 words, viewed as what each part is
        self.buf = torch.zeros((16 + self.capacity * LEDGER_COLS,), dtype=torch.int32, device=self.device)
        state = self.buf[:16]
        self.counts = state[:4].view(torch.int64)
        self.sums = state[4:].view(torch.float64)
        self.ring = self.buf[16:].view(torch.float32).view(self.capacity, LEDGER_COLS)
        self.queued = 0                   # appends enqueued over the ledger's life (the host's count; no device read)
        self.fetched = 0                  # rows returned or reported dropped by fetch()
        self._reset_at = 0

    def record(self, loss_values, norm):
        """The launch alone: what a capture records (nothing runs, nothing is counted; every replay is reported by replayed())."""
        self._ops.step_ledger(loss_values, norm, self.ring, self.counts, self.sums)

    def replayed(self, n=1):
        self.queued += n

    def append(self, loss_values, norm=None):
        """One launch on the current stream: loss_values = the (8,) buffer of the one-launch losses (its first five floats are
        read), norm = the optimizer's (1,) norm tensor or None."""
        self.record(loss_values, norm)
        self.queued += 1

    def _host(self):
        host = self.buf.cpu().numpy()                                   # THE copy (it waits for the appends enqueued so far)
        counts = host[:4].view(np.int64)
        return int(counts[0]), int(counts[1]), host[4:16].view(np.float64).copy(), host[16:].view(np.float32).reshape(self.capacity, LEDGER_COLS)

    def fetch(self):
        """-> (rows (n, 6) float32, dropped): the rows appended since the last fetch in append order; dropped = rows that were
        overwritten before this fetch (more than `capacity` were pending)."""
        appended, _, _, ring = self._host()
        rows, dropped = unwrap_ring(ring, appended, self.fetched)
        self.fetched = appended
        return rows, dropped

    def summary(self):
        """{'steps', 'non_finite', 'mean'} since the last reset(): mean = float64 sums over the finite rows / their number, by
        column name (NaN where there was no finite row)."""
        appended, bad, sums, _ = self._host()
        steps = appended - self._reset_at
        finite = steps - bad
        with np.errstate(invalid='ignore', divide='ignore'):
            mean = sums / np.float64(finite) if finite > 0 else np.full(LEDGER_COLS, np.nan)
        return {'steps': steps, 'non_finite': bad, 'mean': dict(zip(COLUMNS, (float(m) for m in mean)))}

    def reset(self):
        """Zero the sums and the non-finite counter (an enqueued memset, ordered with the appends); `appended` keeps running."""
        self.buf[2:16].zero_()
        self._reset_at = self.queued


# ------------------------------------------------------------------------------------------------------------- checkpoints
def checkpoint_state(model=None, optimizer=None, epoch=None, it=None):
    """train_utils.py:160-169, key for key."""
    optim_state = optimizer.state_dict() if optimizer is not None else None
    model_state = None
    if model is not None:
        if isinstance(model, torch.nn.parallel.DistributedDataParallel):
            model_state = type(model.module.state_dict())((k, v.cpu()) for k, v in model.module.state_dict().items())
        else:
            model_state = model.state_dict()
    return {'epoch': epoch, 'it': it, 'model_state': model_state, 'optimizer_state': optim_state, 'version': 'none'}


def save_checkpoint(state, filename='checkpoint'):
    """train_utils.py:172-180: `filename` without its extension; -> the path written."""
    filename = '{}.pth'.format(filename)
    torch.save(state, filename)
    return filename


def _by_mtime(pattern):
    files = glob.glob(pattern)
    files.sort(key=os.path.getmtime)
    return files


def latest_checkpoint(ckpt_dir):
    """The newest `*checkpoint_epoch_*.pth` of a directory by modification time (train_tracking.py:149-155), or None."""
    files = _by_mtime(os.path.join(str(ckpt_dir), '*checkpoint_epoch_*.pth'))
    return files[-1] if files else None


def rotate_checkpoints(ckpt_dir, max_ckpt_save_num):
    """Before a save (train_utils.py:122-127): with max_ckpt_save_num or more files present, the oldest by modification time
    go, so that the directory holds max_ckpt_save_num once the new one is written. -> the removed paths."""
    files = _by_mtime(os.path.join(str(ckpt_dir), 'checkpoint_epoch_*.pth'))
    gone = files[:len(files) - max_ckpt_save_num + 1] if len(files) >= max_ckpt_save_num else []
    for f in gone:
        os.remove(f)
    return gone


class _Quiet(object):
    def info(self, *a, **k):
        pass

    warning = info


def resume(trainer, ckpt_dir_or_file, logger=None):
    """Model, optimizer and counters from a checkpoint file, or from the newest one of a directory (nothing there: (0, 0) and
    nothing changes). trainer.iteration = it, which is all a OneCycle schedule goes by; a per-epoch 'step' schedule is built
    anew over the loaded param_groups (their `lr` and `initial_lr` are the straight run's), as the reference builds its scheduler
    after the load (train_tracking.py:139-165). -> (it, start_epoch)."""
    path = str(ckpt_dir_or_file)
    if os.path.isdir(path):
        path = latest_checkpoint(path)
        if path is None:
            return 0, 0
    it, epoch = trainer.tracker.load_params_with_optimizer(path, to_cpu=trainer.device.type == 'cpu', optimizer=trainer.optimizer,
                                                           logger=logger or _Quiet())
    it, epoch = int(it), int(epoch)
    trainer.iteration = it
    old = trainer.epoch_scheduler
    if isinstance(old, torch.optim.lr_scheduler.StepLR):
        trainer.epoch_scheduler = torch.optim.lr_scheduler.StepLR(trainer.optimizer, step_size=old.step_size, gamma=old.gamma)
    return it, epoch


# ----------------------------------------------------------------------------------------------------------------- WITH_EVAL
def eval_due(with_eval, trained_epoch):
    """train_utils.py:135-137 over a TRAIN.WITH_EVAL section (a mapping with ENABLE, START_EPOCH, INTERVAL; None: never)."""
    if not with_eval:
        return False
    return bool(with_eval['ENABLE'] and trained_epoch >= with_eval['START_EPOCH'] and trained_epoch % with_eval['INTERVAL'] == 0)


def runner_args(data_cfg, test_cfg):
    """PackedTrackletRunner's keyword arguments from a DATA_CONFIG and a TEST section."""
    from .train_feed import TrainBatchPlan
    a = TrainBatchPlan.config_args(data_cfg)
    get = lambda key, default: test_cfg[key] if (test_cfg is not None and key in test_cfg) else default
    out = {k: a[k] for k in ('search_size', 'template_size', 'search_offset', 'search_scale', 'model_offset', 'model_scale', 'use_z')}
    out.update(shape_aggregation=get('SHAPE_AGGREGATION', 'firstandprevious'), ref_box=get('REF_BOX', 'previous_result'))
    return out


def make_evaluator(tracklets, data_cfg, test_cfg=None, slots=48):
    """evaluator(model, epoch) -> {'epoch', 'success', 'precision', 'frames'} over the validation `tracklets`: a
    PackedTrackletRunner (built at the first call, kept: its model graph is captured again when the weights changed) with
    TEST.SHAPE_AGGREGATION / REF_BOX and DATA_CONFIG's sizes and offsets, scored by eval_metrics.evaluate under REF_COOR."""
    tracklets = list(tracklets)
    args = runner_args(data_cfg, test_cfg)
    ref_coord = data_cfg['REF_COOR'] if 'REF_COOR' in data_cfg else 'lidar'
    state = {}

    def evaluator(model, epoch):
        from . import eval_metrics
        from .packed_runner import PackedTrackletRunner
        device = next(model.parameters()).device
        if state.get('model') is not model:
            state['model'], state['runner'] = model, PackedTrackletRunner(model, device, slots=slots, **args)
        res = eval_metrics.evaluate(state['runner'].run(tracklets), tracklets, ref_coord=ref_coord, device=device)
        return {'epoch': epoch, 'success': float(res['success']), 'precision': float(res['precision']), 'frames': int(np.sum(res['frames']))}
    return evaluator


# ----------------------------------------------------------------------------------------------------------------------- fit
def _rank(rank):
    if rank is not None:
        return int(rank)
    return dist.get_rank() if (dist.is_available() and dist.is_initialized()) else 0


def _current_lr(optimizer):
    try:                                                    # train_utils.py:29-32
        return float(optimizer.lr)
    except AttributeError:
        return float(optimizer.param_groups[0]['lr'])


def fit(trainer, feeder, total_epochs, ckpt_dir, start_epoch=0, start_iter=0, ckpt_save_interval=1, max_ckpt_save_num=50, with_eval=None,
        evaluator=None, logger=None, tb_log=None, log_interval=100, rank=None, on_non_finite='warn'):
    """Epochs start_epoch .. total_epochs - 1 of `trainer` over `feeder` (anything with set_epoch, __len__ and iteration).

    Per epoch: feeder.set_epoch(e); trainer.step(batch) per batch; a per-epoch 'step' schedule (trainer.epoch_scheduler) is stepped
    with the explicit epoch (train_utils.py:116-117); on rank 0 every ckpt_save_interval-th epoch is saved as
    ckpt_dir/checkpoint_epoch_<e + 1>.pth after the oldest files beyond max_ckpt_save_num were removed; `with_eval` (the
    TRAIN.WITH_EVAL section) decides whether evaluator(model, e + 1) runs on rank 0, under eval() and no_grad(), the model going
    back to train() afterwards.

    Logging: with a StepLedger on the trainer the steps' values are fetched every log_interval steps, at the end of an epoch and
    whenever the ring is full — never per step; without one (CPU, a stock loss path) loss.item() is read per step as the
    reference does. Either way tb_log.add_scalar receives train/loss, meta_data/learning_rate, train/<the four tb_dict keys> and
    train/grad_norm for EVERY step under that step's iteration number (start_iter counts on from a resumed run's `it`).
    on_non_finite: 'warn' (the reference trains on), 'raise' (FloatingPointError when the values are looked at — with a ledger
    that is the next fetch, not the step itself) or 'ignore'.

    -> one record per epoch: {'epoch' (trained epochs, 1-based as in the file name), 'loss' (mean over the epoch's finite steps),
    'lr' (of its last step), 'steps', 'non_finite', 'checkpoint' (path or None), 'eval' (the evaluator's dict or None)}."""
    if on_non_finite not in ('warn', 'raise', 'ignore'):
        raise ValueError("on_non_finite: 'warn', 'raise' or 'ignore'")
    rank = _rank(rank)
    log = logger or _Quiet()
    ledger = trainer.ledger
    if ledger is not None:
        ledger.fetch()                                      # rows of steps taken before this call are not this run's
    if trainer.iteration != start_iter:
        trainer.iteration = int(start_iter)
    it = int(start_iter)
    pending = []                                            # (iteration, lr) of the steps whose rows are still on the device
    stats = {}

    def emit(step_it, lr, row, given):
        """One step's values to the meters and the logger. row: 6 floats; given: which of them exist."""
        bad = any(g and not np.isfinite(v) for v, g in zip(row, given))
        stats['steps'] += 1
        if bad:
            stats['non_finite'] += 1
            msg = "fit: non-finite training values at iteration %d: %s" % (step_it, dict((c, float(v)) for c, v, g in zip(COLUMNS, row, given) if g))
            if on_non_finite == 'raise':
                raise FloatingPointError(msg)
            if on_non_finite == 'warn':
                log.warning(msg)
                warnings.warn(msg)
        else:
            stats['sum'] += np.float64(row[0])
        if tb_log is not None and rank == 0:
            tb_log.add_scalar('train/loss', float(row[0]), step_it)
            tb_log.add_scalar('meta_data/learning_rate', lr, step_it)
            for c, v, g in zip(COLUMNS[1:], row[1:], given[1:]):
                if g:
                    tb_log.add_scalar('train/' + c, float(v), step_it)

    def flush():
        if not pending:
            return
        rows, dropped = ledger.fetch()
        assert dropped == 0 and len(rows) == len(pending), (dropped, len(rows), len(pending))
        for (step_it, lr), row in zip(pending, rows):
            emit(step_it, lr, row, (True,) * LEDGER_COLS)
        del pending[:]

    records = []
    for epoch in range(int(start_epoch), int(total_epochs)):
        feeder.set_epoch(epoch)
        stats.update(steps=0, non_finite=0, sum=np.float64(0.0))
        if ledger is not None:
            ledger.reset()
        lr = _current_lr(trainer.optimizer)
        for batch in feeder:
            queued = ledger.queued if ledger is not None else 0
            loss = trainer.step(batch)
            lr = _current_lr(trainer.optimizer)             # after the step: a per-iteration schedule moved it at its top
            if ledger is not None and ledger.queued == queued + 1:
                pending.append((it, lr))
                if len(pending) >= ledger.capacity or (it + 1) % log_interval == 0:
                    flush()
            else:
                if ledger is not None:
                    flush()
                tb = trainer.tb_dict if isinstance(getattr(trainer, 'tb_dict', None), dict) else {}
                row = [float(loss.detach().item())] +[float(tb[c]) if c in tb else np.nan for c in COLUMNS[1:5]] + [np.nan]
                emit(it, lr, row, [True] + [c in tb for c in COLUMNS[1:5]] + [False])
            it += 1
        if ledger is not None:
            flush()
        finite = stats['steps'] - stats['non_finite']
        mean = float(stats['sum'] / np.float64(finite)) if finite > 0 else float('nan')
        if ledger is not None and trainer.ledger_fed and stats['steps']:
            s = ledger.summary()                            # the device's own count and float64 sums: what the rows add up to
            assert s['steps'] == stats['steps'] and s['non_finite'] == stats['non_finite'], (s, stats)
            mean = s['mean']['loss']
        if trainer.epoch_scheduler is not None:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")             # torch calls the epoch argument deprecated; it is the reference's call
                trainer.epoch_scheduler.step(epoch)
        trained = epoch + 1
        record = {'epoch': trained, 'loss': mean, 'lr': lr, 'steps': stats['steps'], 'non_finite': stats['non_finite'], 'checkpoint': None, 'eval': None}
        log.info('epoch %d: %d steps, mean loss %.6f, lr %.3e, %d non-finite' % (trained, stats['steps'], mean, lr, stats['non_finite']))
        if trained % ckpt_save_interval == 0 and rank == 0:
            os.makedirs(str(ckpt_dir), exist_ok=True)
            rotate_checkpoints(ckpt_dir, max_ckpt_save_num)
            record['checkpoint'] = save_checkpoint(checkpoint_state(trainer.tracker, trainer.optimizer, trained, it),
                                                   filename=os.path.join(str(ckpt_dir), 'checkpoint_epoch_%d' % trained))
        if evaluator is not None and eval_due(with_eval, trained) and rank == 0:
            log.info('**********************Eval %d Start**********************' % trained)
            model = trainer.tracker
            model.eval()
            try:
                with torch.no_grad():
                    record['eval'] = evaluator(model, trained)
            finally:
                model.train()
            log.info('**********************Eval %d Over: %s**********************' % (trained, record['eval']))
        records.append(record)
    return records


def from_config(cfg, train_tracklets, device, ckpt_dir, val_tracklets=None, model=None, slots=48, ledger_capacity=1024, feeder_args=None,
                trainer_args=None, **fit_args):
    """The training run of a reference YAML as ptt_amd.config reads it: the feeder of DATA_CONFIG, the trainer of OPTIMIZATION
    (BATCH_SIZE_PER_GPU, NUM_EPOCHS, its optimizer / scheduler / GRAD_NORM_CLIP) with a StepLedger, the evaluator of TEST over
    `val_tracklets` when TRAIN.WITH_EVAL.ENABLE, resumed from the newest checkpoint of `ckpt_dir` if there is one
    (train_tracking.py:104-192). -> run(**more fit() arguments) -> fit()'s records; run.trainer / run.feeder / run.evaluator /
    run.start are what it was built from. model: the tracker to train (default: build_network(cfg.MODEL) on `device`)."""
    from .config import StubDataset
    from .models import build_network
    from .train_feed import TrainBatchFeeder
    from .train_step import DataParallelTrainer
    device = torch.device(device)
    opt = cfg['OPTIMIZATION']
    if model is None:
        names = cfg['CLASS_NAMES'] if 'CLASS_NAMES' in cfg else ['Car']
        names = [names] if isinstance(names, str) else list(names)
        model = build_network(cfg['MODEL'], len(names), StubDataset(training=True, class_names=names)).to(device)
    model.train()
    feeder = TrainBatchFeeder.from_config(train_tracklets, device, cfg['DATA_CONFIG'], opt['BATCH_SIZE_PER_GPU'], **(feeder_args or {}))
    trainer = DataParallelTrainer.from_optim_cfg(model, device, opt, len(feeder), opt['NUM_EPOCHS'],
                                                 ledger=StepLedger(device, ledger_capacity), **(trainer_args or {}))
    with_eval = cfg['TRAIN']['WITH_EVAL'] if ('TRAIN' in cfg and 'WITH_EVAL' in cfg['TRAIN']) else None
    evaluator = None
    if val_tracklets is not None and with_eval and with_eval['ENABLE']:
        evaluator = make_evaluator(val_tracklets, cfg['DATA_CONFIG'], cfg['TEST'] if 'TEST' in cfg else None, slots)
    it, start_epoch = resume(trainer, ckpt_dir, fit_args.get('logger')) if os.path.isdir(str(ckpt_dir)) else (0, 0)

    def run(**more):
        kw = dict(start_epoch=start_epoch, start_iter=it, with_eval=with_eval, evaluator=evaluator)
        kw.update(fit_args)
        kw.update(more)
        return fit(trainer, feeder, opt['NUM_EPOCHS'], ckpt_dir, **kw)
    run.trainer, run.feeder, run.evaluator, run.start = trainer, feeder, evaluator, (it, start_epoch)
    return run


def from_kitti(cfg, device, ckpt_dir, root=None, missing='origin', **kw):
    """from_config on a KITTI tracking directory (cfg.DATA_CONFIG.DATA_PATH, or `root`): the training tracklets are read from the
    files of DATA_SPLIT.train and preloaded by LIDAR_CROP_OFFSET, the validation tracklets — only when TRAIN.WITH_EVAL.ENABLE —
    are the whole scans of DATA_SPLIT.test (datasets/kitti/kitti_scenes.kitti_tracklets). Everything else, `kw` included, is
    from_config's. -> its run; run.train_scenes / run.val_scenes are the two KittiTrackingScenes (val_scenes None without
    evaluation)."""
    from .datasets.kitti import kitti_tracklets
    names = cfg['CLASS_NAMES'] if 'CLASS_NAMES' in cfg else 'Car'
    data_cfg = cfg['DATA_CONFIG']
    train = kitti_tracklets(data_cfg, names, True, device, root=root, missing=missing)
    with_eval = cfg['TRAIN']['WITH_EVAL'] if ('TRAIN' in cfg and 'WITH_EVAL' in cfg['TRAIN']) else None
    val = kitti_tracklets(data_cfg, names, False, device, root=root, missing=missing) if with_eval and with_eval['ENABLE'] else None
    run = from_config(cfg, train.tracklets(), device, ckpt_dir, val_tracklets=None if val is None else val.tracklets(), **kw)
    run.train_scenes, run.val_scenes = train, val
    return run
