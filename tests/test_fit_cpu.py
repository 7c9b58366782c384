"""ptt_amd.fit without a device: checkpoint rotation and the newest checkpoint by modification time, the WITH_EVAL predicate, the
ring unwrap of StepLedger.fetch, and fit() itself on the CPU — the stock path that reads loss.item() per step — with its records,
its tensorboard scalars and the identity of a resumed run with the straight one."""
import os

import numpy as np
import pytest
import torch

from ptt_amd import fit as F


def test_abi_and_exports():
    from ptt_amd import _lib
    assert _lib.ABI_VERSION >= 36
    assert "ptt_step_ledger_f32" in _lib.EXPORTS
    assert _lib.DEFINES["PTT_LEDGER_COLS"] == F.LEDGER_COLS == len(F.COLUMNS) == 6


def _touch(path, mtime):
    with open(path, "wb") as fh:
        fh.write(b"x")
    os.utime(path, (mtime, mtime))


def test_rotation_and_latest_checkpoint_go_by_mtime(tmp_path):
    d = str(tmp_path)
    assert F.latest_checkpoint(d) is None and F.rotate_checkpoints(d, 2) == []
    # written out of epoch order: epoch 3 is the OLDEST file, epoch 1 the newest
    for epoch, mtime in ((3, 1000), (2, 2000), (4, 3000), (1, 4000)):
        _touch(os.path.join(d, "checkpoint_epoch_%d.pth" % epoch), mtime)
    _touch(os.path.join(d, "best_checkpoint_epoch_9.pth"), 3500)          # matches the resume glob, not the rotation's
    _touch(os.path.join(d, "checkpoint_epoch_5.txt"), 9000)
    assert os.path.basename(F.latest_checkpoint(d)) == "checkpoint_epoch_1.pth"
    assert F.rotate_checkpoints(d, 50) == []
    gone = F.rotate_checkpoints(d, 3)                                     # 4 present, room for one more within 3: two go
    assert [os.path.basename(g) for g in gone] == ["checkpoint_epoch_3.pth", "checkpoint_epoch_2.pth"]
    assert sorted(os.listdir(d)) == ["best_checkpoint_epoch_9.pth", "checkpoint_epoch_1.pth", "checkpoint_epoch_4.pth", "checkpoint_epoch_5.txt"]
    os.utime(os.path.join(d, "best_checkpoint_epoch_9.pth"), (5000, 5000))
    assert os.path.basename(F.latest_checkpoint(d)) == "best_checkpoint_epoch_9.pth"
    gone = F.rotate_checkpoints(d, 1)
    assert [os.path.basename(g) for g in gone] == ["checkpoint_epoch_4.pth", "checkpoint_epoch_1.pth"]


@pytest.mark.parametrize("cfg", [dict(ENABLE=True, START_EPOCH=3, INTERVAL=1), dict(ENABLE=True, START_EPOCH=2, INTERVAL=2),
                                 dict(ENABLE=False, START_EPOCH=1, INTERVAL=1)])
def test_with_eval_predicate(cfg):
    from ptt_amd.config import EasyDict
    for trained_epoch in range(1, 7):
        # tools/train_utils/train_utils.py:135-137
        ref = cfg["ENABLE"] and trained_epoch >= cfg["START_EPOCH"] and trained_epoch % cfg["INTERVAL"] == 0
        assert F.eval_due(cfg, trained_epoch) is bool(ref)
        assert F.eval_due(EasyDict(cfg), trained_epoch) is bool(ref)
    assert F.eval_due(None, 3) is False


def test_ring_unwrap():
    """Capacity 4, rows numbered by their first column; 3, then 2, then 6 appends (the cases of tests/test_step_ledger_gpu.py)."""
    cap, ring, appended, fetched = 4, np.full((4, 6), -1.0, np.float32), 0, 0
    for n, dropped in ((3, 0), (2, 0), (6, 2), (0, 0), (4, 0), (9, 5)):
        for _ in range(n):
            ring[appended % cap] = np.arange(6) + 10 * appended
            appended += 1
        rows, d = F.unwrap_ring(ring, appended, fetched)
        kept = n - dropped
        assert d == dropped and rows.shape == (kept, 6)
        assert rows[:, 0].tolist() == [10.0 * k for k in range(appended - kept, appended)]
        assert all(np.array_equal(r, np.arange(6) + r[0]) for r in rows)
        fetched = appended
    with pytest.raises(ValueError):
        F.unwrap_ring(ring, 3, 4)


def test_checkpoint_keys_are_the_references(tmp_path):
    m = torch.nn.Linear(3, 2)
    opt = torch.optim.Adam(m.parameters())
    state = F.checkpoint_state(m, opt, 4, 44)
    assert tuple(state) == F.CHECKPOINT_KEYS == ('epoch', 'it', 'model_state', 'optimizer_state', 'version')
    path = F.save_checkpoint(state, str(tmp_path / "checkpoint_epoch_4"))
    assert path.endswith("checkpoint_epoch_4.pth") and F.latest_checkpoint(str(tmp_path)) == path
    back = torch.load(path)
    assert set(back) == set(F.CHECKPOINT_KEYS) and back['epoch'] == 4 and back['it'] == 44 and back['version'] == 'none'


# ------------------------------------------------------------------------------------------------- fit() on the CPU, stock path
class _Tb(object):
    def __init__(self):
        self.calls = []

    def add_scalar(self, name, value, it):
        self.calls.append((name, float(value), int(it)))

    def series(self, name):
        return [(it, v) for n, v, it in self.calls if n == name]


class _ListFeed(object):
    """A list-backed loader: epoch e serves its batches rotated by e (so a wrong set_epoch shows)."""

    def __init__(self, batches):
        self.batches, self.epoch = batches, 0

    def set_epoch(self, epoch):
        self.epoch = epoch

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        k = self.epoch % len(self.batches)
        return iter(self.batches[k:] + self.batches[:k])


OPTIM = dict(OPTIMIZER='adam', LR=0.001, WEIGHT_DECAY=0, BETAS=[0.5, 0.999], EPS=1e-6, SCHEDULER='step', STEP_SIZE=1, GAMMA=0.5, GRAD_NORM_CLIP=10)


def _trainer(seed):
    from ptt_amd.config import EasyDict, StubDataset, ptt_model_cfg
    from ptt_amd.models import build_network
    from ptt_amd.train_step import DataParallelTrainer
    from tests.util import fill_state_dict_
    model = fill_state_dict_(build_network(ptt_model_cfg(), 1, StubDataset(training=True)), seed).train()
    return DataParallelTrainer.from_optim_cfg(model, "cpu", EasyDict(OPTIM), 2, 2)


def _equal_state(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


def _equal_optim(a, b):
    assert a['state'].keys() == b['state'].keys()
    for k in a['state']:
        for name, v in a['state'][k].items():
            assert torch.equal(torch.as_tensor(v), torch.as_tensor(b['state'][k][name])), (k, name)
    assert [g['lr'] for g in a['param_groups']] == [g['lr'] for g in b['param_groups']]
    assert [g.get('initial_lr') for g in a['param_groups']] == [g.get('initial_lr') for g in b['param_groups']]


def test_fit_on_the_cpu_records_scalars_and_resume(tmp_path, monkeypatch):
    from ptt_amd.train_step import synthetic_train_batch
    from tests.test_ddp_cpu import _oracle_index_ops
    _oracle_index_ops(monkeypatch.setattr)
    torch.set_num_threads(min(8, torch.get_num_threads()))
    batches = [synthetic_train_batch(seed, 2, "cpu") for seed in (300, 301)]
    straight_dir, split_dir = str(tmp_path / "straight"), str(tmp_path / "split")

    tb = _Tb()
    t = _trainer(7)
    assert t.ledger is None and t.epoch_scheduler is not None
    records = F.fit(t, _ListFeed(batches), 2, straight_dir, tb_log=tb, log_interval=3)
    assert [r['epoch'] for r in records] == [1, 2] and all(r['steps'] == 2 and r['non_finite'] == 0 for r in records)
    assert [os.path.basename(r['checkpoint']) for r in records] == ["checkpoint_epoch_1.pth", "checkpoint_epoch_2.pth"]
    assert all(r['eval'] is None for r in records)
    # 'step' with STEP_SIZE 1, GAMMA 0.5, stepped with the explicit epoch: epochs 0 and 1 run at LR, the file of epoch 2 holds LR / 2
    assert [r['lr'] for r in records] == [0.001, 0.001]
    loss = tb.series('train/loss')
    assert [it for it, _ in loss] == [0, 1, 2, 3] and all(np.isfinite(v) for _, v in loss)
    assert tb.series('meta_data/learning_rate') == [(k, 0.001) for k in range(4)]
    for key in ('centroids_cls_loss', 'centroids_reg_loss', 'boxes_cls_loss', 'boxes_reg_loss'):
        assert [it for it, _ in tb.series('train/' + key)] == [0, 1, 2, 3], key
    assert tb.series('train/grad_norm') == []                              # the stock path has no norm to report
    for r, span in zip(records, ((0, 2), (2, 4))):
        mean = np.float64(0.0)
        for _, v in loss[span[0]:span[1]]:
            mean += np.float64(v)
        assert r['loss'] == float(mean / np.float64(2))
    assert t.iteration == 4 and int(t.tracker.global_step) == 4

    # the split run: one epoch; a model built from another seed, a new trainer and feed; resume; the second epoch
    first = F.fit(_trainer(7), _ListFeed(batches), 1, split_dir)
    assert first[0]['loss'] == records[0]['loss']
    t2 = _trainer(99)
    it, start_epoch = F.resume(t2, split_dir)
    assert (it, start_epoch) == (2, 1) and t2.iteration == 2
    tb2 = _Tb()
    second = F.fit(t2, _ListFeed(batches), 2, split_dir, start_epoch=start_epoch, start_iter=it, tb_log=tb2)
    assert len(second) == 1 and second[0]['epoch'] == 2 and second[0]['loss'] == records[1]['loss']
    assert tb2.series('train/loss') == loss[2:]
    a = torch.load(os.path.join(straight_dir, "checkpoint_epoch_2.pth"))
    b = torch.load(os.path.join(split_dir, "checkpoint_epoch_2.pth"))
    assert set(a) == set(b) == set(F.CHECKPOINT_KEYS) and a['epoch'] == b['epoch'] == 2 and a['it'] == b['it'] == 4
    _equal_state(a['model_state'], b['model_state'])
    _equal_optim(a['optimizer_state'], b['optimizer_state'])
    assert [g['lr'] for g in a['optimizer_state']['param_groups']] == [0.0005]
    # nothing to resume: an empty directory changes nothing
    empty = tmp_path / "empty"
    empty.mkdir()
    assert F.resume(t2, str(empty)) == (0, 0) and t2.iteration == 4
