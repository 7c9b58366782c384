"""ptt_box_overlap_f64 / ptt_amd.eval_metrics on the device against the float64 checker tests/box_overlap_ref.py (pinned by
tests/test_eval_metrics_cpu.py): hand-made families of box pairs and a seeded random set under both coordinate conventions and
both dims, the Success / Precision curves fed with the device's values, argument errors, and TrackletRunner -> evaluate end to end.

Tolerance: 1e-9 absolute on overlap and accuracy. Both sides are float64 and follow the same algorithm; two DIFFERENT float64
algorithms for the intersection area disagreed by 4e-13 m^2 on such pairs, so 1e-9 leaves three orders of margin and is still far
below what a wrong vertex would cause. What the reference makes exact is compared exactly: 1.0 from the equality shortcut, 0.0 for
disjoint or vertically separated pairs, 0.0 accuracy for identical centres."""
import functools

import numpy as np
import pytest
import torch

from ptt_amd import eval_metrics as E, ops, synth
from tests import box_overlap_ref as R

pytestmark = pytest.mark.gpu
COORDS = ("camera", "lidar")
TOL = 1e-9
K = 64                      # pairs per family
BLOCK = 256                 # box_overlap_kernel's workgroup: n = BLOCK + 1 is one pair into the second one


def _quat(coord):
    return R.q_camera if coord == "camera" else R.q_lidar


def _mk(coord, plane, up, wlh, ang):
    """A box from footprint-plane quantities: `plane` = the centre on (x, z) for camera, (x, y) for lidar; `up` the third."""
    centre = [plane[0], up, plane[1]] if coord == "camera" else [plane[0], plane[1], up]
    return R.box_row(centre, wlh, _quat(coord)(ang))


def _base(rs, coord):
    plane, up = rs.uniform(-38.0, 38.0, 2), rs.uniform(-3.0, 3.0)
    wlh = rs.uniform([1.2, 2.0, 1.2], [2.2, 5.0, 2.2])
    ang = rs.uniform(-np.pi, np.pi)
    return plane, up, wlh, ang


def _along(ang, d_len, d_wid):
    """A footprint-plane offset of d_len along the box's length and d_wid along its width. The length runs along the first
    footprint axis at angle 0; a positive camera angle (about +y) turns it towards -z, a positive lidar yaw towards +y."""
    return np.array([np.cos(ang) * d_len - np.sin(ang) * d_wid, np.sin(ang) * d_len + np.cos(ang) * d_wid])


def _in_plane(coord, ang, d_len, d_wid):
    off = _along(ang, d_len, d_wid)
    return np.array([off[0], -off[1]]) if coord == "camera" else off


@functools.lru_cache(maxsize=None)
def _families(coord):
    """{name: (gt (K,10), pred (K,10))}, seeded."""
    rs = np.random.RandomState(11 if coord == "camera" else 12)
    fam = {}

    def build(name, fn):
        pairs = [fn(k) for k in range(K)]
        fam[name] = (np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]))

    def identical(k):
        a = _mk(coord, *_base(rs, coord))
        return a, a.copy()

    def within_allclose(k):
        a = _mk(coord, *_base(rs, coord))
        b = a.copy()
        b[k % 3] += 1e-7
        return a, b

    def outside_allclose(k):
        a = _mk(coord, *_base(rs, coord))
        b = a.copy()
        b[0] += 1e-3                                         # > 1e-8 + 1e-5 * 38
        return a, b

    def asymmetric_allclose(k):
        # 0.001000015 apart at 100 m: inside the bound taken from the larger centre (1e-8 + 1e-5 * 100.001000015 = 0.00100002),
        # outside the one taken from 100.0 (0.00100001) — np.allclose judges against its SECOND argument, the result box
        plane, up, wlh, ang = _base(rs, coord)
        lo, hi = _mk(coord, (100.0, plane[1]), up, wlh, ang), _mk(coord, (100.001000015, plane[1]), up, wlh, ang)
        return (lo, hi) if k % 2 == 0 else (hi, lo)

    def negated_quaternion(k):
        a = _mk(coord, *_base(rs, coord))
        b = a.copy()
        b[6:10] = -b[6:10]
        return a, b

    def parallel_shift(k):
        plane, up, wlh, ang = _base(rs, coord)
        d_len = rs.uniform(-0.8, 0.8) * wlh[1]
        d_wid = 0.0 if k % 2 == 0 else rs.uniform(-0.8, 0.8) * wlh[0]        # even: two edges of each box on one line
        return _mk(coord, plane, up, wlh, ang), _mk(coord, plane + _in_plane(coord, ang, d_len, d_wid), up, wlh, ang)

    def quarter_turns(k):
        plane, up, wlh, ang = _base(rs, coord)
        b = _mk(coord, plane + rs.uniform(-0.3, 0.3, 2), up + rs.uniform(-0.1, 0.1), wlh * rs.uniform(0.9, 1.1, 3), ang + (k % 4) * np.pi / 2)
        return _mk(coord, plane, up, wlh, ang), b

    def inside(k):
        plane, up, wlh, ang = _base(rs, coord)
        m = min(wlh[0], wlh[1])
        small = np.array([0.3 * m, 0.3 * m, 0.5 * wlh[2]])
        a, b = _mk(coord, plane, up, wlh, ang), _mk(coord, plane + rs.uniform(-0.1, 0.1, 2) * m, up, small, rs.uniform(-np.pi, np.pi))
        return (a, b) if k % 2 == 0 else (b, a)

    def shared_edge(k):
        plane, up, wlh, ang = _base(rs, coord)
        d = (wlh[1], 0.0) if k % 2 == 0 else (0.0, wlh[0])
        return _mk(coord, plane, up, wlh, ang), _mk(coord, plane + _in_plane(coord, ang, *d), up, wlh, ang)

    def disjoint(k):
        plane, up, wlh, ang = _base(rs, coord)
        t = rs.uniform(-np.pi, np.pi)
        far = (wlh[0] + wlh[1] + 1.0 + 6.0 * rs.rand()) * np.array([np.cos(t), np.sin(t)])
        return _mk(coord, plane, up, wlh, ang), _mk(coord, plane + far, up, wlh * rs.uniform(0.8, 1.2, 3), rs.uniform(-np.pi, np.pi))

    def vertical(k):
        # the height term reads component 1 of the centres under both conventions: more than both heights apart there
        a = _mk(coord, *_base(rs, coord))
        b = a.copy()
        b[3:6] *= rs.uniform(0.9, 1.1, 3)
        b[1] += (a[5] + b[5] + 0.1 + rs.rand()) * (1 if k % 2 else -1)
        return a, b

    def roll_pitch(k):
        plane, up, wlh, ang = _base(rs, coord)
        tilt = lambda: R.q_mul(R.q_axis(0, rs.normal(0, 0.2)), R.q_axis(1, rs.normal(0, 0.2)))
        a, b = _mk(coord, plane, up, wlh, ang), _mk(coord, plane + rs.normal(0, 0.5, 2), up + rs.normal(0, 0.1), wlh * rs.uniform(0.8, 1.2, 3),
                                                   ang + rs.normal(0, 0.3))
        a[6:10], b[6:10] = R.q_mul(a[6:10], tilt()), R.q_mul(b[6:10], tilt())
        return a, b

    for fn in (identical, within_allclose, outside_allclose, asymmetric_allclose, negated_quaternion, parallel_shift, quarter_turns,
               inside, shared_edge, disjoint, vertical, roll_pitch):
        build(fn.__name__, fn)
    return fam


@functools.lru_cache(maxsize=None)
def _family_expected(coord, dims):
    return {name: R.overlaps(gt, pred, coord, dims) for name, (gt, pred) in _families(coord).items()}


@functools.lru_cache(maxsize=None)
def _random(coord):
    return R.random_pairs(21 if coord == "camera" else 22, 4099, coord)


@functools.lru_cache(maxsize=None)
def _random_expected(coord, dims, n):
    gt, pred = _random(coord)
    return R.overlaps(gt[:n], pred[:n], coord, dims)


def _device_values(dev, gt, pred, coord, dims):
    ov, acc = ops.box_overlap(torch.from_numpy(np.ascontiguousarray(gt)).to(dev), torch.from_numpy(np.ascontiguousarray(pred)).to(dev), coord, dims)
    return ov.cpu().numpy(), acc.cpu().numpy()


def _close(name, got, want, gt, pred, zeros_exact=True):
    """Within TOL of the checker, and exactly equal where the reference makes the value exact: 1.0 where the equality shortcut
    applies (decided on the boxes — a geometric value that happens to round to 1.0 is not pinned), 0.0 where the checker finds no
    intersection or no common height (zeros_exact), 0.0 accuracy for identical centres."""
    (g_ov, g_acc), (w_ov, w_acc) = got, want
    assert g_ov.shape == w_ov.shape and g_acc.shape == w_acc.shape and g_ov.dtype == g_acc.dtype == np.float64
    d_ov, d_acc = float(np.abs(g_ov - w_ov).max()), float(np.abs(g_acc - w_acc).max())
    print("%s: n %d, worst |overlap - checker| %.3g, worst |accuracy - checker| %.3g" % (name, len(w_ov), d_ov, d_acc))
    assert d_ov <= TOL and d_acc <= TOL, (name, d_ov, d_acc)
    same = np.array([R.boxes_equal(a, b) for a, b in zip(gt, pred)], bool)
    np.testing.assert_array_equal(w_ov[same], 1.0, err_msg=name)
    np.testing.assert_array_equal(g_ov[same], 1.0, err_msg=name)
    if zeros_exact:
        np.testing.assert_array_equal(g_ov[w_ov == 0.0], 0.0, err_msg=name)
    np.testing.assert_array_equal(g_acc[w_acc == 0.0], 0.0, err_msg=name)


@pytest.mark.parametrize("dims", [2, 3])
@pytest.mark.parametrize("coord", COORDS)
def test_families_equal_the_checker(dev, coord, dims):
    fams, wants = _families(coord), _family_expected(coord, dims)
    got = {name: _device_values(dev, gt, pred, coord, dims) for name, (gt, pred) in fams.items()}
    for name in fams:
        # a shared edge is 0 within the tolerance, not by construction: an intersection of rounding-error area is legitimate
        _close("%s %s dims %d" % (name, coord, dims), got[name], wants[name], *fams[name], zeros_exact=name != "shared_edge")
    ov = {name: g[0] for name, g in got.items()}
    acc = {name: g[1] for name, g in got.items()}
    want = {name: w[0] for name, w in wants.items()}
    # what each family is there for — asserted on the checker too, so that a family cannot quietly miss its point
    for o in (ov, want):
        np.testing.assert_array_equal(o["identical"], 1.0)
        np.testing.assert_array_equal(o["within_allclose"], 1.0)
        assert np.all(o["outside_allclose"] < 1.0) and np.all(o["outside_allclose"] > 0.99)
        np.testing.assert_array_equal(o["asymmetric_allclose"][0::2], 1.0)
        assert np.all(o["asymmetric_allclose"][1::2] < 1.0) and np.all(o["asymmetric_allclose"][1::2] > 0.99)
        assert np.all(np.abs(o["negated_quaternion"] - 1.0) <= TOL)
        assert np.all(np.abs(o["shared_edge"]) <= TOL)
        np.testing.assert_array_equal(o["disjoint"], 0.0)
        # (under lidar the dims-3 height term reads y, which these shifts move: some pairs are 0 there by the reference's quirk)
        assert np.all(o["parallel_shift"] < 1.0) and (dims == 3 or np.all(o["parallel_shift"] > 0.0))
        assert np.all(o["roll_pitch"] >= 0.0) and np.all(o["roll_pitch"] < 1.0) and np.mean(o["roll_pitch"] > 0.05) > 0.5
        if dims == 3:
            np.testing.assert_array_equal(o["vertical"], 0.0)
    np.testing.assert_array_equal(acc["identical"], 0.0)
    np.testing.assert_array_equal(acc["negated_quaternion"], 0.0)
    if dims == 2:
        # closed forms: the footprint of the inner box over that of the outer one; a box against itself moved along its axes
        gt, pred = fams["inside"]
        small, large = np.minimum(gt[:, 3] * gt[:, 4], pred[:, 3] * pred[:, 4]), np.maximum(gt[:, 3] * gt[:, 4], pred[:, 3] * pred[:, 4])
        np.testing.assert_allclose(ov["inside"], small / large, rtol=0, atol=TOL)
    if dims == 3 or coord == "camera":
        # touching boxes are a box length (even pairs) or width (odd pairs) apart. Not so for lidar with dims 2: the shift lies in
        # (x, y) and estimateAccuracy's dims-2 norm reads components 0 and 2
        gt, _ = fams["shared_edge"]
        apart = np.where(np.arange(K) % 2 == 0, gt[:, 4], gt[:, 3])
        np.testing.assert_allclose(acc["shared_edge"], apart, rtol=0, atol=TOL)


@pytest.mark.parametrize("n,dims", [(1, 3), (BLOCK + 1, 3), (BLOCK + 1, 2), (4099, 3), (4099, 2)])
@pytest.mark.parametrize("coord", COORDS)
def test_random_pairs_equal_the_checker(dev, coord, n, dims):
    """Seeded perturbed pairs — centre offset N(0, 0.6 m), yaw offset N(0, 0.3 rad), sizes scaled by U(0.8, 1.2), centres within
    +-40 m — at one pair, one pair past a workgroup and several workgroups with a ragged tail."""
    gt, pred = _random(coord)
    assert np.abs(gt[:, 0:3]).max() <= 40.0 and np.abs(pred[:, 0:3]).max() <= 40.0
    got = _device_values(dev, gt[:n], pred[:n], coord, dims)
    want = _random_expected(coord, dims, n)
    _close("random %s n %d dims %d" % (coord, n, dims), got, want, gt[:n], pred[:n])
    if n == 4099:
        assert want[0].mean() > 0.15 and np.mean(want[0] > 0) > 0.8             # the set is about overlapping boxes


@pytest.mark.parametrize("coord", COORDS)
def test_curves_from_device_values_equal_the_checkers(dev, coord):
    """Success / Precision fed with the device's values == the checker's classes fed with the checker's values: the curves exactly,
    as counts, the averages within 1e-9. Pairs whose checker value lies within 1e-6 of a threshold are left out on both sides (a
    1e-9 difference may legitimately move them across); exact 0 and exact 1 stay in. At most 1 % may be left out."""
    gt, pred = _random(coord)
    g_ov, g_acc = _device_values(dev, gt, pred, coord, 3)
    w_ov, w_acc = _random_expected(coord, 3, 4099)
    ref_s, ref_p = R.Success(), R.Precision()
    near = lambda v, x: np.abs(v[:, None] - x[None, :]).min(1) < 1e-6
    keep_ov = ~near(w_ov, ref_s.Xaxis) | (w_ov == 0.0) | (w_ov == 1.0)
    keep_acc = ~near(w_acc, ref_p.Xaxis) | (w_acc == 0.0)
    print("left out: %d overlaps, %d accuracies of %d" % ((~keep_ov).sum(), (~keep_acc).sum(), len(w_ov)))
    assert (~keep_ov).mean() <= 0.01 and (~keep_acc).mean() <= 0.01
    s, p = E.Success(), E.Precision()
    s.extend(g_ov[keep_ov])
    p.extend(g_acc[keep_acc])
    for v in w_ov[keep_ov]:
        ref_s.add_overlap(v)
    for v in w_acc[keep_acc]:
        ref_p.add_accuracy(v)
    assert s.count == ref_s.count and p.count == ref_p.count
    np.testing.assert_array_equal(np.rint(s.value * s.count).astype(np.int64), ref_s.counts)
    np.testing.assert_array_equal(np.rint(p.value * p.count).astype(np.int64), ref_p.counts)
    np.testing.assert_array_equal(s.value, ref_s.value)
    np.testing.assert_array_equal(p.value, ref_p.value)
    assert abs(s.average - ref_s.average) <= 1e-9 and abs(p.average - ref_p.average) <= 1e-9
    assert 0 < s.average < 100 and 0 < p.average < 100


def test_argument_errors_and_the_empty_launch(dev):
    gt, pred = _random("lidar")
    g, p = torch.from_numpy(gt[:4].copy()), torch.from_numpy(pred[:4].copy())
    with pytest.raises(RuntimeError):
        ops.box_overlap(g, p, "lidar")                                          # CPU tensors
    g, p = g.to(dev), p.to(dev)
    with pytest.raises(RuntimeError):
        ops.box_overlap(g, p.cpu(), "lidar")
    with pytest.raises(RuntimeError):
        ops.box_overlap(g.float(), p.float(), "lidar")
    with pytest.raises(RuntimeError):
        ops.box_overlap(g, p[:3], "lidar")
    for dims in (0, 1, 4):
        with pytest.raises(RuntimeError, match="PTT_EINVAL"):
            ops.box_overlap(g, p, "lidar", dims)
    for coord in (-1, 2):
        with pytest.raises(RuntimeError, match="PTT_EINVAL"):
            ops.box_overlap(g, p, coord)
    with pytest.raises(ValueError):
        ops.box_overlap(g, p, "radar")
    ov, acc = ops.box_overlap(g[:0], p[:0], "camera")
    assert tuple(ov.shape) == tuple(acc.shape) == (0,) and ov.dtype == torch.float64
    ov, acc = E.overlaps([], [], "lidar")
    assert ov.shape == acc.shape == (0,) and ov.dtype == acc.dtype == np.float64
    # the constants of the C ABI and any letter case, as the reference's `.lower()`
    want = ops.box_overlap(g, p, "lidar")[0].cpu().numpy()
    np.testing.assert_array_equal(ops.box_overlap(g, p, "LiDAR")[0].cpu().numpy(), want)
    np.testing.assert_array_equal(ops.box_overlap(g, p, ops.REF_COORDS["lidar"])[0].cpu().numpy(), want)
    assert not np.array_equal(ops.box_overlap(g, p, "Camera")[0].cpu().numpy(), want)


def test_single_pair_functions_take_boxes_and_tuples(dev):
    """estimateOverlap / estimateAccuracy with the reference's signatures and defaults (dim = 2, camera / dim = 3): the mirror's Box
    objects or the runner's (center, wlh, quat[, score]) tuples -> Python floats."""
    from ptt_amd.datasets.kitti.kitti_tracking_utils import Box, Quaternion
    gt, pred = _random("camera")
    a, b = gt[5], pred[5]
    box = lambda r: Box(r[0:3], r[3:6], Quaternion(array=r[6:10]))
    tup = lambda r: (r[0:3], r[3:6], r[6:10], 0.5)
    for dim in (2, 3):
        want_ov, want_acc = R.estimateOverlap(a, b, dim, "camera"), R.estimateAccuracy(a, b, dim)
        for fa, fb in ((box, box), (tup, tup), (box, tup)):
            ov, acc = E.estimateOverlap(fa(a), fb(b), dim, "Camera"), E.estimateAccuracy(fa(a), fb(b), dim)
            assert type(ov) is float and type(acc) is float
            assert abs(ov - want_ov) <= TOL and abs(acc - want_acc) <= TOL
    assert abs(E.estimateOverlap(box(a), box(b)) - R.estimateOverlap(a, b, 2, "camera")) <= TOL          # the defaults
    assert abs(E.estimateAccuracy(box(a), box(b)) - R.estimateAccuracy(a, b, 3)) <= TOL
    assert E.estimateOverlap(box(a), box(a)) == 1.0 and E.estimateAccuracy(tup(a), box(a)) == 0.0


@functools.lru_cache(maxsize=None)
def _tracker(dev):
    """A seeded, randomised tracker with small regression outputs, as a trained model's are (random weights alone move a box by
    metres per frame)."""
    from ptt_amd.config import StubDataset, ptt_model_cfg
    from ptt_amd.hot_path import randomize_
    from ptt_amd.models import build_network
    tracker = randomize_(build_network(ptt_model_cfg(), 1, StubDataset()), seed=2).to(dev).eval()
    with torch.no_grad():
        tracker.box_voting_head.refine_layer[-1].conv.weight.mul_(0.05)
        tracker.box_voting_head.refine_layer[-1].conv.bias.mul_(0.05)
    return tracker


def test_evaluate_scores_a_runners_results_end_to_end(dev):
    """Two 6-frame tracklets through TrackletRunner(batch=2), then evaluate(results, tracklets): the per-frame values equal the
    checker applied to the same result boxes, frame 0 (the ground-truth box itself) scores overlap 1.0 and accuracy 0.0 exactly,
    the overall numbers are those of the pooled curves and the per-tracklet ones those of each tracklet's own frames."""
    from ptt_amd.tracklet_runner import TrackletRunner
    tracklets = [synth.tracklet(300, 6), synth.tracklet(301, 6)]
    results = TrackletRunner(_tracker(dev), dev, batch=2).run(tracklets)
    out = E.evaluate(results, tracklets)
    assert [len(r) for r in results] == [6, 6] and out["frames"].tolist() == [6, 6]
    rows = lambda boxes: np.stack([R.box_row(*b[0:3]) for b in boxes])
    gt = np.concatenate([rows(boxes) for _, boxes in tracklets])
    pred = np.concatenate([rows(res) for res in results])
    _close("end to end", (out["overlap"], out["accuracy"]), R.overlaps(gt, pred, "lidar", 3), gt, pred)
    for first in (0, 6):
        assert out["overlap"][first] == 1.0 and out["accuracy"][first] == 0.0
    assert np.any(out["accuracy"] > 0) and np.any(out["overlap"] < 1.0)             # the boxes did move

    def pooled(ov, acc):
        s, p = R.Success(), R.Precision()
        for v in ov:
            s.add_overlap(v)
        for v in acc:
            p.add_accuracy(v)
        return s, p
    s, p = pooled(out["overlap"], out["accuracy"])
    assert abs(out["success"] - s.average) <= 1e-9 and abs(out["precision"] - p.average) <= 1e-9
    np.testing.assert_array_equal(out["success_curve"], s.value)
    np.testing.assert_array_equal(out["precision_curve"], p.value)
    assert out["tracklet_success"].shape == out["tracklet_precision"].shape == (2,)
    for t in range(2):
        s, p = pooled(out["overlap"][6 * t:6 * t + 6], out["accuracy"][6 * t:6 * t + 6])
        assert abs(out["tracklet_success"][t] - s.average) <= 1e-9 and abs(out["tracklet_precision"][t] - p.average) <= 1e-9
