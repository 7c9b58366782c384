"""What the product reuses across calls — the captured training step, the captured inference graphs, the eval-mode caches of
packed / folded weights — against a fresh eager computation of the CURRENT state, after that state changed underneath it:

* the reference's training loop moves every batch to the device anew (tools/train_utils/train_utils.py:38-44,
  load_data_to_gpu): the freed batch's blocks come back with fresh version counters, and a raw-pointer writer refills a buffer
  without moving its counter — the replayed step must train on the new batch all the same;
* repeated checkpoint evaluation (load_state_dict) and training between evaluations (WITH_EVAL) change the weights a
  captured inference graph was recorded with — its next replay must compute with the new ones (or refuse, where a batch is in
  flight);
* a replayed training step moves the BatchNorm running statistics through raw pointers — the eval-mode caches keyed on
  (data_ptr, _version) must see them move, frozen layers included.

The bars are the existing suite's: bit-identity between graph and eager (tests/test_train_graph_gpu.py, test_hot_path_gpu.py),
box for box between tracklet runners (test_tracking_gpu.py)."""
import numpy as np
import pytest
import torch

from ptt_amd import synth

pytestmark = pytest.mark.gpu

OUT_KEYS = ('search_inds', 'template_inds', 'cosine_feats', 'pred_centroids_votes', 'pred_box_center', 'pred_box_data')


# ------------------------------------------------------------------ training: the batch the replay trains on
def _trainer(dev, graph, freeze=None, weights=None, **kw):
    from ptt_amd.config import StubDataset, ptt_model_cfg
    from ptt_amd.models import build_network
    from ptt_amd.train_step import DataParallelTrainer
    torch.manual_seed(1)
    model = build_network(ptt_model_cfg(), 1, StubDataset(training=True))
    if weights is not None:
        model.load_state_dict(weights)
    model = model.to(dev).train()
    if freeze is not None:
        getattr(model, freeze).requires_grad_(False)
    return DataParallelTrainer(model, dev, graph=graph, **kw)


def _same_state(a, b):
    from tests.test_train_graph_gpu import _same_state as same       # the bar of the captured-step tests
    return same(a, b)


def _numpy_batch(seed, B=4):
    """synthetic_train_batch's arrays before they are moved to the device: what the reference's data loader hands over."""
    from ptt_amd.train_step import synthetic_train_batch
    cpu = synthetic_train_batch(seed, B, torch.device('cpu'))
    return {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in cpu.items()}


def _reloaded_pass(dev, graph, n):
    """The reference's loop: `batch = next(dataloader_iter); load_data_to_gpu(batch)` — the previous device batch is freed
    before the next one is allocated, at the same size."""
    from ptt_amd.models import load_data_to_gpu
    tr = _trainer(dev, graph)
    losses, ptrs = [], []
    for k in range(n):
        batch = _numpy_batch(200 + k)
        load_data_to_gpu(batch, dev)
        losses.append(tr.step(batch).detach().clone())
        ptrs.append(batch['search_points'].data_ptr())
    torch.cuda.synchronize()
    return tr, losses, ptrs


def _refilled_pass(dev, graph, n):
    """One device batch, refilled in place each step through .data: new contents, same storage, same version counter — what a
    raw-pointer writer (this project's crop kernels) leaves behind."""
    from ptt_amd.models import load_data_to_gpu
    tr = _trainer(dev, graph)
    batch = load_data_to_gpu(_numpy_batch(300), dev)
    losses = []
    for k in range(n):
        src = _numpy_batch(300 + k)
        for key, v in batch.items():
            if torch.is_tensor(v):
                v.data.copy_(torch.from_numpy(src[key]))
        losses.append(tr.step(batch).detach().clone())
    torch.cuda.synchronize()
    return tr, losses


def _assert_twins(graphed, eager, lg, le, n):
    assert graphed.graph_steps == n - graphed.graph_warmup and graphed.captured is not None and eager.captured is None
    for k, (a, b) in enumerate(zip(le, lg)):
        assert torch.equal(a, b) and bool(torch.isfinite(b)), (k, float(a), float(b))
    assert len(set(float(x) for x in le)) == n                       # every step saw another batch
    bad = _same_state(eager, graphed)
    assert not bad, bad


def test_replayed_step_trains_on_each_reloaded_batch(dev):
    """Graphed and eager trainer in two passes from one seed (the eager twin does not disturb the graphed pass's allocations),
    fed the reference's way: every step's loss and the final state bit-identical — and the batch's device address DID repeat
    across replayed steps, so that a copy skipped on (data_ptr, _version) would have trained on a stale batch."""
    n = 8
    graphed, lg, ptrs = _reloaded_pass(dev, True, n)
    replayed = ptrs[graphed.graph_warmup:]
    assert len(set(replayed)) < len(replayed), ptrs
    eager, le, _ = _reloaded_pass(dev, False, n)
    _assert_twins(graphed, eager, lg, le, n)


def test_replayed_step_trains_on_a_batch_refilled_in_place(dev):
    n = 8
    graphed, lg = _refilled_pass(dev, True, n)
    eager, le = _refilled_pass(dev, False, n)
    _assert_twins(graphed, eager, lg, le, n)


# ------------------------------------------------------------------ inference graphs after the tracker changed
def _weights(seed):
    """The state of a tracker randomised with `seed` (a checkpoint, as far as the graphs can tell), on the host."""
    from ptt_amd.config import StubDataset, ptt_model_cfg
    from ptt_amd.hot_path import randomize_
    from ptt_amd.models import build_network
    tracker = randomize_(build_network(ptt_model_cfg(), 1, StubDataset()), seed=seed)
    with torch.no_grad():                                  # small regression outputs, as a trained model's are:
        tracker.box_voting_head.refine_layer[-1].conv.weight.mul_(0.05)      # keeps the boxes on their objects
        tracker.box_voting_head.refine_layer[-1].conv.bias.mul_(0.05)
    return tracker.state_dict()


def _tracker(dev, seed):
    from ptt_amd.config import StubDataset, ptt_model_cfg
    from ptt_amd.models import build_network
    tracker = build_network(ptt_model_cfg(), 1, StubDataset())
    tracker.load_state_dict(_weights(seed))
    return tracker.to(dev).eval()


def _frames(dev, seed, B=2, NS=1024, NT=512):
    return tuple(torch.from_numpy(a).to(dev) for a in synth.frames(seed, B, NS, NT))


def _eager(tracker, s, t):
    with torch.no_grad():
        o = tracker({'search_points': s, 'template_points': t, 'batch_size': s.shape[0]})
    return {k: o[k].clone() for k in OUT_KEYS}


def _assert_outputs_equal(got, ref):
    for k in OUT_KEYS:
        assert torch.equal(got[k], ref[k]), k


def test_graphed_tracker_replays_the_weights_it_now_has(dev):
    """GraphedHotPath over the whole tracker: replay == eager with weights a; after load_state_dict(weights b) the next replay
    == eager with weights b (no eager call in between: the weights' version counters are what tells); after weights c and an
    eager forward that rebuilt every cache (the graph's packed buffers are freed) the replay == that forward."""
    from ptt_amd.hot_path import GraphedHotPath, TrackerThroughput
    tracker = _tracker(dev, 2)
    s, t = _frames(dev, 31)
    g = GraphedHotPath(TrackerThroughput(tracker), s, t)
    replay = lambda: {k: v.clone() for k, v in g(s, t).items() if k in OUT_KEYS}
    got_a = replay()
    _assert_outputs_equal(got_a, _eager(tracker, s, t))
    tracker.load_state_dict(_weights(5))
    got_b = replay()
    _assert_outputs_equal(got_b, _eager(tracker, s, t))
    assert not torch.equal(got_a['pred_box_data'], got_b['pred_box_data'])
    tracker.load_state_dict(_weights(6))
    ref_c = _eager(tracker, s, t)
    _assert_outputs_equal(replay(), ref_c)
    assert g.captures == 3


def _tracklets(lengths, base=100):
    return [synth.tracklet(base + k, T) for k, T in enumerate(lengths)]


def _assert_same_boxes(got, ref, tracklets):
    assert len(got) == len(ref) == len(tracklets)
    for a, b, (clouds, _) in zip(got, ref, tracklets):
        assert len(a) == len(b) == len(clouds)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x[0], y[0])
            np.testing.assert_array_equal(x[2], y[2])


def _moved(a, b):
    return any(not np.array_equal(x[0], y[0]) for ra, rb in zip(a, b) for x, y in zip(ra, rb))


RUNNER_CASES = [(1, [6]), (6, [4, 3, 5, 2, 4])]     # the frame graph of a handful of tracklets; GraphedHotPath beyond it


@pytest.mark.parametrize("batch,lengths", RUNNER_CASES)
def test_tracklet_runner_after_a_checkpoint_is_loaded(dev, batch, lengths):
    """The reference's repeated checkpoint evaluation: run with weights a, load_state_dict(weights b), run again — box for box
    what a runner built for weights b returns."""
    from ptt_amd.tracklet_runner import TrackletRunner
    tracker = _tracker(dev, 2)
    tracklets = _tracklets(lengths)
    runner = TrackletRunner(tracker, dev, batch=batch)
    got_a = runner.run(tracklets)
    tracker.load_state_dict(_weights(7))
    got_b = runner.run(tracklets)
    _assert_same_boxes(got_b, TrackletRunner(tracker, dev, batch=batch).run(tracklets), tracklets)
    assert _moved(got_a, got_b)


@pytest.mark.parametrize("batch,lengths", RUNNER_CASES)
def test_tracklet_runner_after_training_between_evaluations(dev, batch, lengths):
    """WITH_EVAL: run, a few training steps on the same tracker (eager warm-up, capture, replays), eval(), run again — box for
    box what a runner built after the training returns."""
    from ptt_amd.train_step import synthetic_train_batch
    from ptt_amd.tracklet_runner import TrackletRunner
    tr = _trainer(dev, None, weights=_weights(4))
    tracker = tr.tracker.eval()
    tracklets = _tracklets(lengths, base=600)
    runner = TrackletRunner(tracker, dev, batch=batch)
    got_a = runner.run(tracklets)
    tracker.train()
    batches = [synthetic_train_batch(700 + k, 4, dev) for k in range(2)]
    for k in range(5):
        tr.step(batches[k % 2])
    assert tr.graph_steps == 2
    tracker.eval()
    got_b = runner.run(tracklets)
    _assert_same_boxes(got_b, TrackletRunner(tracker, dev, batch=batch).run(tracklets), tracklets)
    assert _moved(got_a, got_b)


@pytest.mark.parametrize("batch,lengths", RUNNER_CASES)
def test_tracklet_runner_after_train_eval_and_allocator_churn(dev, batch, lengths):
    """No weight change: train(); eval() drops the SA modules' caches, an eager forward at another input size rebuilds them
    elsewhere and reuses the freed blocks — the next run returns the very same boxes."""
    from ptt_amd.tracklet_runner import TrackletRunner
    tracker = _tracker(dev, 3)
    tracklets = _tracklets(lengths, base=800)
    runner = TrackletRunner(tracker, dev, batch=batch)
    got_a = runner.run(tracklets)
    tracker.train()
    tracker.eval()
    _eager(tracker, *_frames(dev, 41, B=3, NS=2048, NT=1024))
    _assert_same_boxes(runner.run(tracklets), got_a, tracklets)


def test_pipelined_and_interleaved_graphs_refuse_changed_weights(dev):
    """A batch is in flight in these graphs (sampled by the old capture): after a weight change the next call raises instead
    of replaying — over the whole tracker and over the hot-path module."""
    from ptt_amd.hot_path import FrameHotPath, InterleavedHotPath, PipelinedHotPath, TrackerThroughput, kitti_model_cfg, randomize_
    tracker = _tracker(dev, 2)
    s, t = _frames(dev, 51)
    p = PipelinedHotPath(TrackerThroughput(tracker), s, t)
    p(s, t)
    tracker.load_state_dict(_weights(8))
    with pytest.raises(RuntimeError, match="changed"):
        p(s, t)
    model = randomize_(FrameHotPath(kitti_model_cfg()), seed=9).to(dev).eval()
    q = InterleavedHotPath(model, s, t, ways=2)
    q(s, t)
    q(s, t)
    model.load_state_dict(randomize_(FrameHotPath(kitti_model_cfg()), seed=10).state_dict())
    with pytest.raises(RuntimeError, match="changed"):
        q(s, t)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ train and eval on one model
@pytest.mark.parametrize("freeze", [None, "box_voting_head"])
def test_eval_between_replayed_training_steps_sees_the_trained_state(dev, freeze):
    """The reference's WITH_EVAL flow on one model: a captured training step (warm-up, capture, 2 replays), eval() and a
    forward, train() and 3 more replays, another eval forward — each equal, bit for bit, to a fresh model that loaded the
    trainer's state_dict. With a frozen head its BatchNorm layers still move their running statistics in training mode, and
    nothing but those statistics' version counters tells the eval caches that they moved."""
    from ptt_amd.config import StubDataset, ptt_model_cfg
    from ptt_amd.models import build_network
    from ptt_amd.train_step import synthetic_train_batch
    tr = _trainer(dev, True, freeze=freeze)
    batches = [synthetic_train_batch(900 + k, 4, dev) for k in range(2)]
    s, t = _frames(dev, 61)

    def evaluate():
        fresh = build_network(ptt_model_cfg(), 1, StubDataset(training=True)).to(dev)
        fresh.load_state_dict(tr.tracker.state_dict())
        got = _eager(tr.tracker.eval(), s, t)
        ref = _eager(fresh.eval(), s, t)
        torch.cuda.synchronize()
        _assert_outputs_equal(got, ref)
        tr.tracker.train()
        return got

    for k in range(5):
        tr.step(batches[k % 2])
    assert tr.graph_steps == 2
    first = evaluate()
    for k in range(3):
        tr.step(batches[k % 2])
    assert tr.graph_steps == 5 and tr.eager_steps == 3
    second = evaluate()
    assert not torch.equal(first['pred_box_data'], second['pred_box_data'])
