"""Tracking evaluation without a device: (1) the checker tests/box_overlap_ref.py — the reference's estimateOverlap /
estimateAccuracy restated with Sutherland-Hodgman clipping in place of shapely — against closed forms and against an independent
half-space method; (2) what the package declares (C header, ptt_amd.eval_metrics) and the host-side Success / Precision curves
against hand-computed values."""
import os
import re

import numpy as np
import pytest

from tests import box_overlap_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COORDS = ("camera", "lidar")
TRAPZ = getattr(np, "trapz", None) or np.trapezoid          # np.trapz, under the name numpy 2 gives it where it dropped the old one


def _box(coord, plane_xy, up, wlh, ang):
    """A box of one convention from footprint-plane quantities: plane_xy = the centre's two footprint coordinates ((x, z) for
    camera, (x, y) for lidar), up = its remaining coordinate, ang = rotation in the footprint plane. A pure q_y would leave the
    camera footprint (corners 0 1 5 4) degenerate; KITTI's camera boxes carry q_y(ry) * q_x(pi / 2)."""
    if coord == "camera":
        return R.box_row([plane_xy[0], up, plane_xy[1]], wlh, R.q_camera(ang))
    return R.box_row([plane_xy[0], plane_xy[1], up], wlh, R.q_lidar(ang))


# ----------------------------------------------------------------------------- the checker against closed forms
@pytest.mark.parametrize("coord", COORDS)
def test_checker_unit_square_against_itself_turned_45_degrees(coord):
    a = _box(coord, (0.0, 0.0), 0.0, [1, 1, 1], 0.0)
    b = _box(coord, (0.0, 0.0), 0.0, [1, 1, 1], np.pi / 4)
    assert abs(R.intersection_area(a, b, coord) - 2 * (np.sqrt(2) - 1)) < 1e-14          # the regular octagon


@pytest.mark.parametrize("coord", COORDS)
def test_checker_box_against_itself_is_its_footprint(coord):
    a = _box(coord, (3.0, 1.0), -2.0, [2.0, 4.0, 1.5], 0.3)
    assert abs(R.intersection_area(a, a.copy(), coord) - 2.0 * 4.0) < 1e-13
    assert R.estimateOverlap(a, a.copy(), 3, coord) == 1.0 and R.estimateAccuracy(a, a.copy(), 3) == 0.0


@pytest.mark.parametrize("coord", COORDS)
def test_checker_2_by_4_box_shifted_one_metre_along_its_length(coord):
    # at angle 0 the length (wlh[1] = 4) runs along the first footprint axis under both conventions
    a = _box(coord, (0.0, 0.0), 0.0, [2, 4, 1], 0.0)
    b = _box(coord, (1.0, 0.0), 0.0, [2, 4, 1], 0.0)
    assert abs(R.intersection_area(a, b, coord) - 6.0) < 1e-14
    assert abs(R.estimateOverlap(a, b, 2, coord) - 6.0 / 10.0) < 1e-14


@pytest.mark.parametrize("coord", COORDS)
def test_checker_containment_is_small_volume_over_large_volume(coord):
    # the height term reads component 1 of the centre and wlh[2] under BOTH conventions: big spans [0, 2] there, small [0.5, 1.5]
    big = R.box_row([10.0, 2.0, -3.0], [2.0, 4.0, 2.0], (R.q_camera if coord == "camera" else R.q_lidar)(0.4))
    small = R.box_row([10.1, 1.5, -2.9], [1.0, 2.0, 1.0], (R.q_camera if coord == "camera" else R.q_lidar)(0.4))
    if coord == "lidar":                                     # footprint on (x, y): keep y inside big's footprint AND its "height" span
        small[1] = 1.6
    assert abs(R.intersection_area(big, small, coord) - 2.0) < 1e-13
    assert abs(R.estimateOverlap(big, small, 3, coord) - 2.0 / 16.0) < 1e-14
    assert abs(R.estimateOverlap(small, big, 3, coord) - 2.0 / 16.0) < 1e-14


@pytest.mark.parametrize("coord", COORDS)
def test_checker_footprints_overlap_but_ymax_below_ymin_is_exactly_zero(coord):
    # camera: same (x, z), y apart by more than the height. lidar: the "height" term is y too — 0.5 m apart with h = 0.4, while
    # the 2 m wide footprints still overlap
    if coord == "camera":
        a = R.box_row([1.0, 0.0, 5.0], [2, 4, 1.5], R.q_camera(0.2))
        b = R.box_row([1.2, 3.0, 5.1], [2, 4, 1.5], R.q_camera(0.25))
    else:
        a = R.box_row([1.0, 0.0, 5.0], [2, 4, 0.4], R.q_lidar(0.0))
        b = R.box_row([1.2, 0.5, 5.0], [2, 4, 0.4], R.q_lidar(0.0))
    assert R.intersection_area(a, b, coord) > 1.0
    assert R.estimateOverlap(a, b, 3, coord) == 0.0
    assert R.estimateOverlap(a, b, 2, coord) > 0.0


@pytest.mark.parametrize("coord", COORDS)
def test_checker_disjoint_boxes_are_exactly_zero(coord):
    a = _box(coord, (0.0, 0.0), 1.0, [2, 4, 1.5], 0.3)
    for shift, ang in (((10.0, 0.0), 0.3), ((0.0, -7.0), 1.1), ((5.0, 5.0), -0.7)):
        b = _box(coord, shift, 1.0, [2, 4, 1.5], ang)
        assert R.intersection_area(a, b, coord) == 0.0
        assert R.estimateOverlap(a, b, 3, coord) == 0.0 and R.estimateOverlap(a, b, 2, coord) == 0.0


def test_checker_equality_shortcut_is_numpys_asymmetric_allclose():
    a = R.box_row([100.0, 0.0, 0.0], [2, 4, 1.5], R.q_lidar(0.3))
    b = a.copy()
    b[0] += 1e-7
    assert R.estimateOverlap(a, b, 3, "lidar") == 1.0
    b[0] = a[0] + 1e-3                                       # 1e-3 <= 1e-8 + 1e-5 * 100.001: still "equal"
    assert R.estimateOverlap(a, b, 3, "lidar") == 1.0
    # |a - b| <= 1e-8 + 1e-5 * |b| is judged against the SECOND box: 0.0100001 apart passes against 1000.0100001 (bound
    # 0.01000011), not against 1000.0 (bound 0.01000001)
    lo, hi = a.copy(), a.copy()
    lo[0], hi[0] = 1000.0, 1000.0100001
    assert R.boxes_equal(lo, hi) and not R.boxes_equal(hi, lo)
    assert R.estimateOverlap(lo, hi, 3, "lidar") == 1.0 and 0.99 < R.estimateOverlap(hi, lo, 3, "lidar") < 1.0


@pytest.mark.parametrize("coord", COORDS)
def test_checker_agrees_with_the_halfspace_method_on_random_pairs(coord):
    """Seeded perturbed pairs (centres within +-40 m, intersection areas up to ~11 m^2): Sutherland-Hodgman + shoelace against
    scipy's HalfspaceIntersection + ConvexHull within 1e-11 m^2 — the two float64 methods were measured 3.8e-13 apart over 2744 such
    pairs; the margin is about 25 x."""
    gt, pred = R.random_pairs(7, 200, coord)
    worst, n = 0.0, 0
    for a, b in zip(gt, pred):
        pa, pb = R.footprint(a, coord), R.footprint(b, coord)
        other = R.halfspace_area(pa, pb)
        if other is None:
            continue
        worst, n = max(worst, abs(R.clip_area(pa, pb) - other)), n + 1
    print("pairs", n, "worst |clip - halfspace|", worst)
    assert n > 170
    assert worst < 1e-11


# ----------------------------------------------------------------------------- the feature, as far as it shows without a device
def test_header_declares_the_overlap_entry_point_and_its_constants():
    from ptt_amd import _lib
    header = open(os.path.join(ROOT, "include", "ptt_hip.h")).read()
    assert re.search(r"int\s+ptt_box_overlap_f64\s*\(", header)
    assert _lib.DEFINES["PTT_REF_CAMERA"] == 0 and _lib.DEFINES["PTT_REF_LIDAR"] == 1
    import ctypes
    vp, i = ctypes.c_void_p, ctypes.c_int
    assert _lib.PROTOTYPES["ptt_box_overlap_f64"] == (i, [vp, vp, i, i, i, vp, vp, vp])


def test_eval_metrics_exports_the_references_names():
    from ptt_amd import eval_metrics as E
    for name in ("estimateOverlap", "estimateAccuracy", "Success", "Precision", "overlaps", "evaluate"):
        assert callable(getattr(E, name)), name
    import ptt.eval_metrics                                  # the `ptt` alias resolves it too
    assert ptt.eval_metrics.Success.__name__ == "Success"
    for cls, adder in ((E.Success, "add_overlap"), (E.Precision, "add_accuracy")):
        m = cls()
        for attr in (adder, "reset", "extend", "count", "value", "average", "Xaxis"):
            assert hasattr(m, attr), (cls.__name__, attr)


def test_success_and_precision_curves_on_hand_written_lists():
    from ptt_amd.eval_metrics import Precision, Success
    s, p = Success(), Precision()
    assert s.average == 0 and p.average == 0 and s.count == 0 and p.count == 0
    np.testing.assert_array_equal(s.Xaxis, np.linspace(0, 1, 21))
    np.testing.assert_array_equal(p.Xaxis, np.linspace(0, 2, 21))

    s.add_overlap(1.0)
    np.testing.assert_array_equal(s.value, np.ones(21))
    assert abs(s.average - 100.0) < 1e-12
    p.add_accuracy(0.0)
    np.testing.assert_array_equal(p.value, np.ones(21))
    assert abs(p.average - 100.0) < 1e-12

    s.reset()
    assert s.count == 0
    for v in (0.0, 0.5, 1.0):
        s.add_overlap(v)
    x = np.linspace(0, 1, 21)
    # thresholds 0: all three; (0, 0.5]: two (x[10] is exactly 0.5 and >= keeps it); (0.5, 1]: one (1.0 >= x[20] = 1.0)
    want = np.array([3.0] + [2.0] * 10 + [1.0] * 10) / 3
    np.testing.assert_array_equal(s.value, want)
    assert s.average == TRAPZ(want, x=x) * 100 / 1
    assert s.count == 3

    # a value exactly ON a threshold counts: >= for Success, <= for Precision
    s2, p2 = Success(), Precision()
    s2.extend(np.array([x[7]]))
    np.testing.assert_array_equal(s2.value, (np.arange(21) <= 7).astype(float))
    px = np.linspace(0, 2, 21)
    p2.extend([px[7]])
    np.testing.assert_array_equal(p2.value, (np.arange(21) >= 7).astype(float))
    assert p2.average == TRAPZ((np.arange(21) >= 7).astype(float), x=px) * 100 / 2
    # just off the threshold, on the losing side
    s3, p3 = Success(), Precision()
    s3.add_overlap(np.nextafter(x[7], 0.0))
    p3.add_accuracy(np.nextafter(px[7], 3.0))
    np.testing.assert_array_equal(s3.value, (np.arange(21) <= 6).astype(float))
    np.testing.assert_array_equal(p3.value, (np.arange(21) >= 8).astype(float))

    # accuracies beyond the last threshold never count; other curve lengths / ranges as the constructor says
    p4 = Precision(n=5, max_accuracy=4)
    p4.extend([0.5, 2.0, 9.0, 3.9])
    np.testing.assert_array_equal(p4.Xaxis, np.linspace(0, 4, 5))
    np.testing.assert_array_equal(p4.value, np.array([0, 1, 2, 2, 3]) / 4.0)
    assert p4.average == TRAPZ(np.array([0, 1, 2, 2, 3]) / 4.0, x=np.linspace(0, 4, 5)) * 100 / 4


def test_curves_equal_the_checkers_on_a_seeded_list():
    from ptt_amd.eval_metrics import Precision, Success
    rs = np.random.RandomState(3)
    ov = np.concatenate([rs.uniform(0, 1, 200), [0.0, 1.0, 0.35, 0.7]])
    acc = np.concatenate([rs.uniform(0, 3, 200), [0.0, 2.0, 0.4]])
    s, p, rs_, rp = Success(), Precision(), R.Success(), R.Precision()
    s.extend(ov)
    p.extend(acc)
    for v in ov:
        rs_.add_overlap(v)
    for v in acc:
        rp.add_accuracy(v)
    np.testing.assert_array_equal(s.value, rs_.value)
    np.testing.assert_array_equal(p.value, rp.value)
    np.testing.assert_array_equal(np.rint(s.value * s.count), rs_.counts)
    np.testing.assert_array_equal(np.rint(p.value * p.count), rp.counts)
    assert s.average == rs_.average and p.average == rp.average


def test_overlaps_without_a_device_raises():
    import torch
    from ptt_amd import eval_metrics as E, ops
    box = (np.zeros(3), np.ones(3), np.array([1.0, 0, 0, 0]))
    with pytest.raises(RuntimeError):
        ops.box_overlap(torch.zeros(1, 10, dtype=torch.float64), torch.zeros(1, 10, dtype=torch.float64), "lidar")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            E.estimateOverlap(box, box)
