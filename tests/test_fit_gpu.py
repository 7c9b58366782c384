"""ptt_amd.fit on the device: fit() over a TrainBatchFeeder with the step ledger inside the captured training step, against
trainers stepped by hand; exact resume; checkpoint rotation and WITH_EVAL; the collective branch on a one-rank group. The full
tracker at batch_size 4, spare 2, one candidate per frame: 6 batches per epoch, so graph_warmup = 3 puts eager steps, the capture
and replays inside epoch 0. Every comparison is bit identity."""
import importlib.util
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 5
TB_KEYS = ('centroids_cls_loss', 'centroids_reg_loss', 'boxes_cls_loss', 'boxes_reg_loss')
ADAM_STEP = dict(OPTIMIZER='adam', LR=0.001, WEIGHT_DECAY=0, BETAS=[0.5, 0.999], EPS=1e-6, SCHEDULER='step', STEP_SIZE=1, GAMMA=0.5,
                 GRAD_NORM_CLIP=10)
ONECYCLE = dict(OPTIMIZER='adam_onecycle', LR=0.003, WEIGHT_DECAY=0.01, MOMS=[0.95, 0.85], DIV_FACTOR=10, PCT_START=0.4, GRAD_NORM_CLIP=10)


@pytest.fixture(scope="module")
def tracklets():
    from ptt_amd import synth
    return [synth.tracklet(seed, 6, n_obj=(100, 300), n_bg=(300, 800)) for seed in range(4)]


class _Tb(object):
    def __init__(self):
        self.calls = []

    def add_scalar(self, name, value, it):
        self.calls.append((name, float(value), int(it)))

    def series(self, name):
        return [(it, v) for n, v, it in self.calls if n == name]


def _feeder(trks, dev):
    from ptt_amd.train_feed import TrainBatchFeeder
    f = TrainBatchFeeder(trks, dev, batch_size=4, spare=2, candidates_per_frame=1, seed=SEED)
    assert len(f) == 6
    return f


def _model(dev, seed=1):
    from ptt_amd.config import StubDataset, ptt_model_cfg
    from ptt_amd.models import build_network
    torch.manual_seed(seed)
    return build_network(ptt_model_cfg(), 1, StubDataset(training=True)).to(dev).train()


def _ledger(dev):
    from ptt_amd.fit import StepLedger
    return StepLedger(dev, capacity=32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _assert_same_model(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    assert sa.keys() == sb.keys()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


def _assert_same_optim(a, b, groups=True):
    a = a if isinstance(a, dict) else a.state_dict()
    b = b if isinstance(b, dict) else b.state_dict()
    assert a['state'].keys() == b['state'].keys() and len(a['state']) > 100
    for k in a['state']:
        assert a['state'][k].keys() == b['state'][k].keys()
        for name, v in a['state'][k].items():
            assert torch.equal(torch.as_tensor(v).cpu(), torch.as_tensor(b['state'][k][name]).cpu()), (k, name)
    if groups:
        for ga, gb in zip(a['param_groups'], b['param_groups']):
            assert ga['lr'] == gb['lr'] and ga.get('initial_lr') == gb.get('initial_lr') and ga.get('betas') == gb.get('betas')


def test_the_ledger_holds_every_steps_values(dev, tracklets, tmp_path):
    from ptt_amd.fit import fit
    from ptt_amd.train_step import DataParallelTrainer
    # the twin: stepped by hand, eagerly, reading the device after every step — what fit() with the ledger never does
    twin = DataParallelTrainer(_model(dev), dev, graph=False)
    f = _feeder(tracklets, dev)
    f.set_epoch(0)
    want = []
    for batch in f:
        loss = twin.step(batch)
        values = next(iter(twin.tb_dict.values())).owner.device_values
        torch.cuda.synchronize()
        row = np.concatenate([values[:5].cpu().numpy(), twin.optimizer.last_norm.cpu().numpy().reshape(1)])
        assert _bits(np.array([float(loss.detach())]))[0] == _bits(row)[0]      # column 0 is the loss the step returned
        want.append(row)
    want = np.stack(want)
    assert want.shape == (6, 6) and np.isfinite(want).all()

    tb = _Tb()
    graphed = DataParallelTrainer(_model(dev), dev, graph=True, ledger=_ledger(dev))
    records = fit(graphed, _feeder(tracklets, dev), 1, str(tmp_path / "a"), tb_log=tb)
    torch.cuda.synchronize()
    assert graphed.graph_steps == 3 and graphed.eager_steps == 3 and graphed.ledger_fed
    assert graphed.captured.ledger and graphed.captured.second is None and graphed.captured.loss_values is not None
    got = graphed.ledger.ring[:6].cpu().numpy()
    assert np.array_equal(_bits(got), _bits(want)), (got, want)             # all 6 x 6 values
    assert graphed.ledger.counts.cpu().tolist() == [6, 0]
    _assert_same_model(graphed.tracker, twin.tracker)
    _assert_same_optim(graphed.optimizer, twin.optimizer)
    # the scalars: the reference's names, each under the iteration numbers 0 .. 5 with the ledger's values
    names = ['train/loss'] + ['train/' + k for k in TB_KEYS] + ['train/grad_norm']
    for c, name in enumerate(names):
        assert tb.series(name) == [(k, float(want[k, c])) for k in range(6)], name
    assert tb.series('meta_data/learning_rate') == [(k, 1e-3) for k in range(6)]
    assert {n for n, _, _ in tb.calls} == set(names) | {'meta_data/learning_rate'}
    r = records[0]
    mean = np.float64(0.0)
    for v in want[:, 0]:
        mean += np.float64(v)
    assert r['epoch'] == 1 and r['steps'] == 6 and r['non_finite'] == 0 and r['loss'] == float(mean / np.float64(6)) and r['lr'] == 1e-3
    assert os.path.basename(r['checkpoint']) == "checkpoint_epoch_1.pth" and r['eval'] is None

    # ledger=None: the same final state (and fit() then reads loss.item() per step)
    tb3 = _Tb()
    plain = DataParallelTrainer(_model(dev), dev, graph=True)
    fit(plain, _feeder(tracklets, dev), 1, str(tmp_path / "b"), tb_log=tb3)
    assert plain.graph_steps == 3 and plain.ledger is None
    _assert_same_model(plain.tracker, twin.tracker)
    _assert_same_optim(plain.optimizer, twin.optimizer)
    assert tb3.series('train/loss') == tb.series('train/loss')


@pytest.mark.parametrize("optim", [ADAM_STEP, ONECYCLE], ids=["adam_step", "adam_onecycle"])
def test_resume_is_exact(dev, tracklets, tmp_path, optim):
    from ptt_amd.config import EasyDict
    from ptt_amd.fit import CHECKPOINT_KEYS, fit, resume
    from ptt_amd.train_step import DataParallelTrainer

    def trainer(seed):
        return DataParallelTrainer.from_optim_cfg(_model(dev, seed), dev, EasyDict(optim), 6, 2, ledger=_ledger(dev))

    straight_dir, split_dir = str(tmp_path / "straight"), str(tmp_path / "split")
    straight = trainer(1)
    records = fit(straight, _feeder(tracklets, dev), 2, straight_dir)
    torch.cuda.synchronize()
    assert [r['steps'] for r in records] == [6, 6] and straight.graph_steps == 9
    rows = straight.ledger.ring[:12].cpu().numpy()
    assert np.isfinite(rows).all()

    fit(trainer(1), _feeder(tracklets, dev), 1, split_dir)
    again = trainer(77)                                                     # another model, a new trainer, a new feeder
    it, start_epoch = resume(again, split_dir)
    assert (it, start_epoch) == (6, 1) and again.iteration == 6
    second = fit(again, _feeder(tracklets, dev), 2, split_dir, start_epoch=start_epoch, start_iter=it)
    torch.cuda.synchronize()
    assert len(second) == 1 and second[0]['epoch'] == 2 and again.graph_steps == 3
    assert np.array_equal(_bits(again.ledger.ring[:6].cpu().numpy()), _bits(rows[6:]))      # epoch 1's rows
    assert second[0]['loss'] == records[1]['loss'] and second[0]['lr'] == records[1]['lr']

    a = torch.load(os.path.join(straight_dir, "checkpoint_epoch_2.pth"))
    b = torch.load(os.path.join(split_dir, "checkpoint_epoch_2.pth"))
    assert set(a) == set(b) == set(CHECKPOINT_KEYS) == {'epoch', 'it', 'model_state', 'optimizer_state', 'version'}
    assert a['epoch'] == b['epoch'] == 2 and a['it'] == b['it'] == 12
    assert a['model_state'].keys() == b['model_state'].keys()
    for k in a['model_state']:
        assert torch.equal(a['model_state'][k], b['model_state'][k]), k
    _assert_same_optim(a['optimizer_state'], b['optimizer_state'])
    if optim is ADAM_STEP:
        # StepLR.step(epoch) after epochs 0 and 1: the file of epoch 1 still holds LR, that of epoch 2 LR / 2
        assert torch.load(os.path.join(split_dir, "checkpoint_epoch_1.pth"))['optimizer_state']['param_groups'][0]['lr'] == 1e-3
        assert [g['lr'] for g in b['optimizer_state']['param_groups']] == [5e-4]
        assert records[1]['lr'] == 1e-3
    else:
        assert len(b['optimizer_state']['param_groups']) == 2 and records[1]['lr'] != records[0]['lr']


def test_rotation_and_with_eval(dev, tracklets, tmp_path):
    from ptt_amd import synth
    from ptt_amd.eval_metrics import evaluate
    from ptt_amd.fit import fit, make_evaluator, runner_args
    from ptt_amd.packed_runner import PackedTrackletRunner
    from ptt_amd.train_step import DataParallelTrainer
    val = [synth.tracklet(seed, 4, n_obj=(100, 300), n_bg=(300, 800)) for seed in (10, 11)]
    data_cfg = dict(REF_COOR='lidar', SEARCH_INPUT_SIZE=1024, TEMPLATE_INPUT_SIZE=512, SEARCH_BB_OFFSET=0.0, SEARCH_BB_SCALE=1.25,
                    MODEL_BB_OFFSET=0.0, MODEL_BB_SCALE=1.25, USE_Z_AXIS=True)
    test_cfg = dict(SHAPE_AGGREGATION='firstandprevious', REF_BOX='previous_result')
    inner, calls = make_evaluator(val, data_cfg, test_cfg, slots=2), []

    def evaluator(model, epoch):
        assert not model.training and not torch.is_grad_enabled()
        calls.append(epoch)
        return inner(model, epoch)

    with_dir, without_dir = str(tmp_path / "with"), str(tmp_path / "without")
    a = DataParallelTrainer(_model(dev), dev, ledger=_ledger(dev))
    records = fit(a, _feeder(tracklets, dev), 3, with_dir, max_ckpt_save_num=2, with_eval=dict(ENABLE=True, START_EPOCH=2, INTERVAL=1),
                  evaluator=evaluator)
    assert sorted(os.listdir(with_dir)) == ["checkpoint_epoch_2.pth", "checkpoint_epoch_3.pth"]
    assert calls == [2, 3] and [r['eval'] is not None for r in records] == [False, True, True]
    assert records[0]['checkpoint'].endswith("checkpoint_epoch_1.pth") and a.tracker.training
    for r in records[1:]:
        fresh = _model(dev, seed=50 + r['epoch'])
        fresh.load_state_dict(torch.load(r['checkpoint'])['model_state'])
        fresh.eval()
        with torch.no_grad():
            res = evaluate(PackedTrackletRunner(fresh, dev, slots=2, **runner_args(data_cfg, test_cfg)).run(val), val, ref_coord='lidar')
        assert r['eval']['epoch'] == r['epoch'] and r['eval']['frames'] == 8
        assert r['eval']['success'] == float(res['success']) and r['eval']['precision'] == float(res['precision']), (r['eval'], res['success'], res['precision'])
    # evaluation did not perturb training: the same three epochs without it
    b = DataParallelTrainer(_model(dev), dev, ledger=_ledger(dev))
    plain = fit(b, _feeder(tracklets, dev), 3, without_dir, max_ckpt_save_num=2)
    torch.cuda.synchronize()
    assert [r['loss'] for r in plain] == [r['loss'] for r in records]
    _assert_same_model(a.tracker, b.tracker)                                # weights and BatchNorm buffers
    _assert_same_optim(a.optimizer, b.optimizer)
    assert np.array_equal(_bits(a.ledger.ring[:18].cpu().numpy()), _bits(b.ledger.ring[:18].cpu().numpy()))


def test_the_collective_branch_on_one_rank(dev):
    """scripts/fit_one_rank_check.py in a child process with its own time limit (a one-rank nccl group, force_ddp=True: the append
    sits in the second graph) against the same epoch here without a group."""
    spec = importlib.util.spec_from_file_location("fit_one_rank_check", os.path.join(ROOT, "scripts", "fit_one_rank_check.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(ROOT, "scripts", "fit_one_rank_check.py")], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=600, cwd=ROOT, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    child = json.loads(lines[0])
    here = mod.one_epoch(dev, force_ddp=False)
    assert child["backend"] == "nccl" and child["world"] == 1 and child["ranks_seen"] == 1 and child["collective"] and not here["collective"]
    assert child["two_graphs"] and not here["two_graphs"] and child["ledger_in_graph"] and here["ledger_in_graph"]
    assert child["graph_steps"] == here["graph_steps"] == 3 and child["steps"] == here["steps"] == 6 and child["ledger_fed"]
    assert child["rows_bits"] == here["rows_bits"] and len(child["rows_bits"]) == 6
    assert child["digest"] == here["digest"] and child["mean_loss"] == here["mean_loss"] and child["non_finite"] == 0
