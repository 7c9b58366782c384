"""TrackletRunner in every SHAPE_AGGREGATION x REF_BOX mode against the restated loop (tests/tracking_modes_ref.py, pinned to the
reference by G18) driving the same tracker; the SHAPE_AGGREGATION = all store (append crops, growth, graph warm-up); the mirror
module's get_model + regularize_pc on G18's `all` frames; resampling of store-sized clouds."""
import functools
import os

import numpy as np
import pytest
import torch

from ptt_amd import ops, synth
from ptt_amd.datasets.kitti import box_math as bm
from tests import tracking_modes_ref as TM

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPES = ("firstandprevious", "first", "previous", "all")
REFS = ("previous_result", "previous_gt", "current_gt")


@functools.lru_cache(maxsize=None)
def _tracker(dev, steady=False):
    """steady: the last vote and refine layers output zeros, so every vote is its seed and every proposal is a point of the search
    cloud with angle 0 (random weights move a box by metres to tens of metres per frame)."""
    from ptt_amd.config import StubDataset, ptt_model_cfg
    from ptt_amd.hot_path import randomize_
    from ptt_amd.models import build_network
    tracker = randomize_(build_network(ptt_model_cfg(), 1, StubDataset()), seed=2).to(dev).eval()
    with torch.no_grad():
        if steady:
            for layer in (tracker.centroid_voting_head.vote_layer[-1], tracker.box_voting_head.refine_layer[-1]):
                for prm in layer.parameters():
                    prm.zero_()
        else:                                              # small regression outputs, as a trained model's are
            tracker.box_voting_head.refine_layer[-1].conv.weight.mul_(0.05)
            tracker.box_voting_head.refine_layer[-1].conv.bias.mul_(0.05)
    return tracker


def _empty_first(seed, n):
    """A tracklet whose frame-0 cloud lies far from its box: the first-frame crop is empty (first: an all-zero template that is
    never resampled, so the generator position comes from the search alone)."""
    clouds, boxes = synth.tracklet(seed, n)
    clouds[0] = np.ascontiguousarray(clouds[0] + np.array([[40.0], [0.0], [0.0]], np.float32))
    return clouds, boxes


def _long(seed, n=30):
    """A 30-frame tracklet of dense objects in dense clutter confined to +-3 m around them (large crops while a box stays near)."""
    clouds, boxes = synth.tracklet(seed, n, n_obj=(600, 900), n_bg=(1, 2))
    rs = np.random.RandomState(seed)
    for i, (center, _, _) in enumerate(boxes):
        clutter = rs.uniform(-1, 1, (3, 1500)) * np.array([[3.0], [3.0], [1.0]]) + center[:, None]
        clouds[i] = np.ascontiguousarray(np.concatenate([clouds[i], clutter.astype(np.float32)], 1))
    return clouds, boxes


def _compact(seed, n=30):
    """Every cloud a dense ball of +-0.4 m around its ground-truth centre: with REF_BOX current_gt and the steady tracker each result
    lies within 0.4 m of its ground truth, so every template crop keeps its whole cloud and the store's total is the sum of the
    cloud sizes — it outgrows its first capacity (the largest cloud) several times, whatever the random weights."""
    _, boxes = synth.tracklet(seed, n)
    rs = np.random.RandomState(seed)
    clouds = [np.ascontiguousarray((rs.uniform(-0.4, 0.4, (3, rs.randint(600, 1400))) + c[:, None]).astype(np.float32))
              for c, _, _ in boxes]
    return clouds, boxes


def _tracklets(shape):
    ts = [synth.tracklet(100, 6), synth.tracklet(101, 4), _empty_first(102, 5), synth.tracklet(103, 3)]
    return ts + [_long(104)] if shape == "all" else ts


@functools.lru_cache(maxsize=None)
def _expected(dev, shape, ref):
    """The restated loop, one frame at a time through the tracker, for every tracklet of _tracklets(shape)."""
    from oracle import tracking_ref as TR
    tracker = _tracker(dev)

    def infer(search, template):
        with torch.no_grad():
            out = tracker({'search_points': torch.from_numpy(np.ascontiguousarray(search)).to(dev),
                           'template_points': torch.from_numpy(np.ascontiguousarray(template)).to(dev), 'batch_size': 1})
        return out['pred_box_data'][0].cpu().numpy()
    return [TM.track_modes(clouds, [TR.RefBox(*b) for b in boxes], infer, shape, ref, use_z=True)
            for clouds, boxes in _tracklets(shape)]


def _check(got, expected, tracklets, tol):
    assert len(got) == len(expected) == len(tracklets)
    n_moved = 0
    for (clouds, _), res, (ref, _) in zip(tracklets, got, expected):
        assert len(res) == len(ref) == len(clouds)
        for i, (r, o) in enumerate(zip(res, ref)):
            # a box that has run far from its object (random weights; a negative offset is never redrawn) moves by metres per
            # frame, and the 1e-5-level differences of the many-frame model kernels grow with it: the tolerance scales with the distance
            np.testing.assert_allclose(r[0], o.center, rtol=0, atol=tol * max(1.0, float(np.abs(o.center).max())),
                                       err_msg="frame %d centre" % i)
            np.testing.assert_array_equal(r[1], o.wlh, err_msg="frame %d wlh" % i)
            np.testing.assert_allclose(bm.q_rotation_matrix(r[2]), o.rotation_matrix, rtol=0, atol=tol)
            n_moved += int(i > 0 and float(np.abs(r[0] - res[0][0]).max()) > 1e-6)
    assert n_moved > 0


@pytest.mark.parametrize("ref", REFS)
@pytest.mark.parametrize("shape", SHAPES)
def test_runner_one_graph_path_equals_the_restated_loop(dev, shape, ref):
    """Batch 1 (the reference's own mode): every frame one hipGraph replay. Every result box equal to the restated loop's (the
    model's inputs are bit-identical, the float64 box update agrees to 1e-9); a gt-referenced result carries the gt box's wlh."""
    from ptt_amd.tracklet_runner import TrackletRunner
    tracklets = _tracklets(shape)
    runner = TrackletRunner(_tracker(dev), dev, batch=1, shape_aggregation=shape, ref_box=ref)
    _check(runner.run(tracklets), _expected(dev, shape, ref), tracklets, 1e-9)


@pytest.mark.parametrize("shape,ref", [(s, "previous_result") for s in SHAPES] + [("all", "previous_gt"), ("all", "current_gt")])
@pytest.mark.parametrize("path", ["upload", "eager"])
def test_runner_other_paths_equal_the_restated_loop(dev, shape, ref, path):
    """Batch 6 (the crop table uploaded, the best proposal selected on the device; the many-frame model kernels order their sums
    differently from the one-frame chain: 1e-4) and use_graph=False at batch 2 (crops by value, eager model)."""
    from ptt_amd.tracklet_runner import TrackletRunner
    tracklets = _tracklets(shape)
    batch, graph = (6, True) if path == "upload" else (2, False)
    runner = TrackletRunner(_tracker(dev), dev, batch=batch, use_graph=graph, shape_aggregation=shape, ref_box=ref)
    tol = 1e-9 if 2 * batch <= ops.CROP_JOBS_BY_VALUE_MAX else 1e-4
    _check(runner.run(tracklets), _expected(dev, shape, ref), tracklets, tol)


def _growths(clouds, frames):
    """How often the store must grow: TrackletRunner's rule (_reserve_store) replayed on the restated loop's totals — the store starts
    at the largest cloud; before frame i appends cloud i - 1 it must hold total + that cloud's points, else it grows to
    max(that, twice its capacity); after frame i its total is the model-point count of frame i's template (get_model over 0..i-1)."""
    cap, total, n = max(c.shape[1] for c in clouds), 0, 0
    for i in range(1, len(clouds)):
        need = total + clouds[i - 1].shape[1]
        if need > cap:
            cap, n = max(need, 2 * cap), n + 1
        total = frames[i - 1]["n_model"]
    return n, cap


@pytest.mark.parametrize("batch", [1, 6])
def test_all_store_grows_without_dropping_a_point(dev, batch):
    """A 30-frame `all` store starts at its largest cloud and has to grow (_compact): the growth rule replayed on the restated loop's
    totals (_growths) asks for at least two growths. The runner counts its own (store_growths) and must have grown exactly as often,
    to the same capacity; the boxes of every frame — which depend on every stored point through the template — equal the restated
    loop's. A second run() starts from an empty store, keeps the capacity and gives the same boxes."""
    from oracle import tracking_ref as TR
    from ptt_amd.tracklet_runner import TrackletRunner
    long_only = [_compact(104)]
    tracker = _tracker(dev, True)

    def infer(search, template):
        with torch.no_grad():
            out = tracker({'search_points': torch.from_numpy(np.ascontiguousarray(search)).to(dev),
                           'template_points': torch.from_numpy(np.ascontiguousarray(template)).to(dev), 'batch_size': 1})
        return out['pred_box_data'][0].cpu().numpy()
    clouds, boxes = long_only[0]
    expected = [TM.track_modes(clouds, [TR.RefBox(*b) for b in boxes], infer, "all", "current_gt", use_z=True)]
    want, cap = _growths(long_only[0][0], expected[0][1])
    assert want >= 2
    runner = TrackletRunner(tracker, dev, batch=batch, shape_aggregation="all", ref_box="current_gt")
    got = runner.run(long_only)
    assert runner.store_growths == want and runner.store.shape[1] == cap
    tol = 1e-9 if 2 * batch <= ops.CROP_JOBS_BY_VALUE_MAX else 1e-4
    _check(got, expected, long_only, tol)
    again = runner.run(long_only)
    assert runner.store_growths == want
    for a, b in zip(got[0], again[0]):
        np.testing.assert_array_equal(a[0], b[0])


def test_overlapped_runners_in_all_mode_give_the_same_boxes(dev):
    """run_overlapped (two runners, their groups alternating on two streams) in SHAPE_AGGREGATION = all == one runner."""
    from ptt_amd.tracklet_runner import TrackletRunner, run_overlapped
    tracker = _tracker(dev, True)
    tracklets = [synth.tracklet(500 + k, T) for k, T in enumerate([5, 3, 6, 4, 2, 5, 1])] + [_long(510, 12)]
    single = TrackletRunner(tracker, dev, batch=3, shape_aggregation="all").run(tracklets)
    both = run_overlapped([TrackletRunner(tracker, dev, batch=2, shape_aggregation="all"),
                           TrackletRunner(tracker, dev, batch=2, shape_aggregation="all")], tracklets)
    assert len(both) == len(single) == len(tracklets)
    for a, b, (clouds, _) in zip(single, both, tracklets):
        assert len(a) == len(b) == len(clouds)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x[0], y[0])
            np.testing.assert_array_equal(x[2], y[2])


def test_G18_mirror_get_model_of_all_frames_equals_the_reference(dev):
    """ptt.datasets.kitti.kitti_tracking_utils (device-backed mirror): get_model over every earlier (cloud, result box) pair — up
    to six clouds, more than PTT_MAX_SEGMENTS — then regularize_pc == G18's `all` templates (the reference's), bit for bit."""
    import ptt.datasets.kitti.kitti_tracking_utils as ku
    from ptt.datasets.kitti.kitti_tracking_utils import Box, Quaternion
    g = np.load(os.path.join(GOLD, "G18_tracking_modes.npz"))
    size = int(g["sizes"][1])
    box = lambda a: Box(a[0:3], a[3:6], Quaternion(array=a[6:10]))
    n = 0
    for t in range(int(g["n_tracklets"])):
        L = int(g["n_frames_%d" % t])
        pcs = [ku.PointCloud(g["cloud_%d_%d" % (t, i)]) for i in range(L)]
        for ref in g["refs"]:
            results = [box(g["gt_%d_0" % t])] + [box(g["res_%d_all_%s_%d" % (t, ref, i)]) for i in range(1, L)]
            for i in range(1, L):
                key = "%d_all_%s_%d" % (t, ref, i)
                model = ku.get_model(pcs[:i], results[:i], offset=0.0, scale=1.25)
                assert model.nbr_points() == int(g["nmodel_" + key]), key
                np.testing.assert_array_equal(ku.regularize_pc(model, size, istrain=False).cpu().numpy(), g["template_" + key],
                                              err_msg=key)
                n += i > 4
    assert n > 0


@pytest.mark.parametrize("n", [70000, 300000])
def test_resampling_index_stream_is_numpys_for_store_sizes(dev, n):
    """A long tracklet's `all` store holds tens to hundreds of thousands of points: the resampling still picks
    np.random.randint(0, n, 512) after np.random.seed(1) (regularize_pc:349-353)."""
    import ptt.datasets.kitti.kitti_tracking_utils as ku
    pts = np.zeros((3, n), np.float32)
    pts[0] = np.arange(n)
    got = ku.regularize_pc(ku.PointCloud(pts), 512, istrain=False).cpu().numpy()
    np.random.seed(1)
    want = np.random.randint(low=0, high=n, size=512, dtype=np.int64)
    np.testing.assert_array_equal(got[:, 0].astype(np.int64), want)
