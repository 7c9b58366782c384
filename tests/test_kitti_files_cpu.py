"""ptt_amd.datasets.kitti.kitti_files on the host, against fixture G28 (tests/golden/make_golden_g28.py: the reference's own
KittiTrackingDataset on the tree tests/kitti_tree.py writes): calibration and label parsing, split -> scenes, tracklet grouping,
annotation -> box, the result line; and KittiTrackingScenes' host half (scene order, tables, replay), which needs no device.

Bounds. Camera centre and wlh are the same float64 subtractions as the reference's: equal. A quaternion component is four
products and three sums of magnitudes <= 1 — at most seven roundings of 2^-53: within 2^-50. The lidar centre goes through an
inverse and two matrix products at magnitudes of tens of metres; 1e-9 m is about a million float64 roundings there, so any
correct order of evaluation passes, while a transposed matrix or a dropped R0 is off by centimetres. Observed on the committed
fixture: 0 for the quaternions, 1.8e-15 m for the lidar centre (tests/golden/GOLDEN_REPORT_G28.txt).
"""
import io
import os

import numpy as np
import pytest

from ptt_amd.datasets.kitti import box_math as bm
from ptt_amd.datasets.kitti import kitti_files as kf
from tests import kitti_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_cache = {}


def _g28():
    if "g28" not in _cache:
        _cache["g28"] = dict(np.load(os.path.join(ROOT, "tests", "golden", "G28_kitti_files.npz")))
    return _cache["g28"]


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("kitti")
    kitti_tree.write_tree(str(root), int(_g28()["seed"]))
    return str(root)


def _paths(tree, scene):
    base = os.path.join(tree, "training")
    return os.path.join(base, "calib", scene + ".txt"), os.path.join(base, "label_02", scene + ".txt")


# ------------------------------------------------------------------------------------------------------------------ calib
def test_calib_in_both_spellings(tree, tmp_path):
    calib = kf.read_calib(_paths(tree, "0019")[0])
    assert [a.shape for a in calib] == [(3, 4), (3, 4), (3, 4), (3, 3)] and all(a.dtype == np.float64 for a in calib)
    R, t = calib.V2C[:, :3], calib.V2C[:, 3]
    assert np.array_equal(calib.C2V[:, :3], R.T) and np.allclose(calib.C2V[:, 3], -R.T @ t, rtol=0, atol=1e-15)
    assert np.abs(calib.R0 - np.eye(3)).max() > 1e-4 and np.abs(np.abs(R).max(1) - 1).min() > 1e-6      # neither is an axis permutation
    # the object-detection spelling, keys with and without the colon, in another order, with a date line in between
    text = open(_paths(tree, "0019")[0]).read().splitlines()
    by_key = {l.split()[0]: l.split()[1:] for l in text}
    other = tmp_path / "object.txt"
    other.write_text("calib_time: 09-Jan-2012 13:57:47\nTr_velo_to_cam: %s\nR0_rect: %s\nP2 %s\n"
                     % (" ".join(by_key["Tr_velo_cam"]), " ".join(by_key["R_rect"]), " ".join(by_key["P2:"])))
    again = kf.read_calib(str(other))
    for a, b in zip(calib, again):
        assert np.array_equal(a, b)
    for drop, named in (("R_rect", "R0_rect"), ("Tr_velo_cam", "Tr_velo_to_cam"), ("P2:", "P2")):
        bad = tmp_path / "bad.txt"
        bad.write_text("\n".join(l for l in text if l.split()[0] != drop) + "\n")
        with pytest.raises(ValueError, match=named) as e:
            kf.read_calib(str(bad))
        assert "bad.txt" in str(e.value)
    short = tmp_path / "short.txt"
    short.write_text("\n".join(l if l.split()[0] != "R_rect" else "R_rect 1 0 0 0 1 0" for l in text) + "\n")
    with pytest.raises(ValueError, match="R_rect"):
        kf.read_calib(str(short))


def test_rect_to_velo_inverts_the_chain(tree):
    calib = kf.read_calib(_paths(tree, "0020")[0])
    velo = np.array([[12.5, -3.25, -0.8], [30.0, 8.0, 1.0]])
    rect = (calib.R0 @ (calib.V2C[:, :3] @ velo.T + calib.V2C[:, 3:])).T
    np.testing.assert_allclose(kf.rect_to_velo(calib, rect), velo, rtol=0, atol=1e-12)
    assert kf.rect_to_velo(calib, rect[0]).shape == (1, 3)


# ----------------------------------------------------------------------------------------------------------------- labels
ROW = "3 7 Car 0 1 -1.5 100.0 150.0 200.0 250.0 1.5 1.7 4.2 2.5 1.6 14.0 -1.2"


def test_labels_17_and_18_fields_and_bad_counts(tmp_path):
    p = tmp_path / "0000.txt"
    p.write_text(ROW + "\n" + ROW.replace("3 7 Car", "4 7 Car") + " 0.93\n\n0 -1 DontCare -1 -1 -10 1 2 3 4 -1000 -1000 -1000 -10 -1 -1 -1\n")
    rows = kf.read_labels(str(p))
    assert rows.dtype.names == kf.LABEL_COLUMNS and len(rows.dtype.names) == 17 and len(rows) == 3
    assert rows["frame"].tolist() == [3, 4, 0] and rows["track_id"].tolist() == [7, 7, -1] and rows["type"].tolist() == ["Car", "Car", "DontCare"]
    assert rows["rotation_y"].tolist() == [-1.2, -1.2, -1.0] and rows["height"][0] == 1.5 and rows["z"][1] == 14.0      # the score is not the last column
    for bad in (" ".join(ROW.split()[:16]), ROW + " 0.9 0.1"):
        p.write_text(ROW + "\n" + ROW + "\n" + bad + "\n")
        with pytest.raises(ValueError, match="line 3") as e:
            kf.read_labels(str(p))
        assert "0000.txt" in str(e.value)
    p.write_text(ROW + "\n" + ROW.replace("14.0", "far") + "\n")
    with pytest.raises(ValueError, match="line 2"):
        kf.read_labels(str(p))


def test_a_track_whose_frames_do_not_ascend_is_refused(tmp_path):
    p = tmp_path / "0000.txt"
    p.write_text("\n".join(ROW.replace("3 7 Car", "%d %d Car" % ft) for ft in ((0, 7), (0, 8), (2, 7), (1, 7), (1, 8))) + "\n")
    rows = kf.read_labels(str(p))
    with pytest.raises(ValueError, match="ascending"):
        kf.tracklets_of(rows, "Car")
    groups = kf.tracklets_of(rows[[0, 1, 2, 4]], "Car")
    assert [g["track_id"].tolist() for g in groups] == [[7, 7], [8, 8]] and [g["frame"].tolist() for g in groups] == [[0, 2], [0, 1]]
    assert kf.tracklets_of(rows, "Cyclist") == []


def test_scenes_of_split():
    assert kf.scenes_of_split("train") == list(range(17)) and kf.scenes_of_split("TRAIN_tiny") == [0]
    assert kf.scenes_of_split("val") == [17, 18] and kf.scenes_of_split("test") == [19, 20] and kf.scenes_of_split("test_tiny") == [0]
    assert kf.scenes_of_split("val_tiny") == [3] and kf.scenes_of_split("all") == list(range(21))
    assert kf.scenes_of_split("trainval") == list(range(17))                 # TRAIN is looked for first


# ------------------------------------------------------------------------------------------------------------ against G28
def test_tracklet_grouping_equals_the_reference(tree):
    g = _g28()
    assert g["scenes"].tolist() == list(kitti_tree.SCENES)
    for scene in kitti_tree.SCENES:
        labels = kf.read_labels(_paths(tree, scene)[1])
        assert set(labels["type"].tolist()) == {"Car", "Pedestrian", "DontCare"} and (labels["track_id"][labels["type"] == "DontCare"] == -1).all()
        groups = kf.tracklets_of(labels, "Car")
        assert [int(r["track_id"][0]) for r in groups] == g["tracks_%s" % scene].tolist() == [1, 0]      # first appearance, not id order
        for rows in groups:
            assert rows["frame"].tolist() == g["frames_%s_%d" % (scene, rows["track_id"][0])].tolist()
        assert [r["frame"].tolist() for r in kf.tracklets_of(labels, "Pedestrian")] == [list(range(kitti_tree.FRAMES))]


def test_annotation_box_equals_the_reference(tree):
    g = _g28()
    q_err = c_err = 0.0
    n = 0
    for scene in kitti_tree.SCENES:
        calib = kf.read_calib(_paths(tree, scene)[0])
        for rows in kf.tracklets_of(kf.read_labels(_paths(tree, scene)[1]), "Car"):
            for coor in ("camera", "lidar", "LIDAR"):
                want = g["box_%s_%s_%d" % (coor.lower(), scene, rows["track_id"][0])]
                assert want.shape == (len(rows), 10) and want.dtype == np.float64
                for r, w in zip(rows, want):
                    c, wlh, q = kf.annotation_box(r, calib, coor)
                    assert c.dtype == wlh.dtype == q.dtype == np.float64 and (c.shape, wlh.shape, q.shape) == ((3,), (3,), (4,))
                    assert np.array_equal(wlh, w[3:6]) and wlh.tolist() == [r["width"], r["length"], r["height"]]
                    if coor == "camera":
                        assert np.array_equal(c, w[:3]) and c.tolist() == [r["x"], r["y"] - r["height"] / 2, r["z"]]
                    else:
                        c_err = max(c_err, float(np.abs(c - w[:3]).max()))
                    q_err = max(q_err, float(np.abs(q - w[6:]).max()))
                    n += 1
    print("annotation_box over %d boxes: quaternion max |diff| %.3e, lidar centre max |diff| %.3e m" % (n, q_err, c_err))
    assert n == 3 * 8 * 3 and q_err <= 2.0 ** -50 and c_err <= 1e-9
    with pytest.raises(ValueError, match="ref_coor"):
        kf.annotation_box(rows[0], calib, "ego")


def test_the_fixtures_boxes_hold_their_points(tree):
    """The tree is worth tracking on: every Car box of either frame holds at least 30 points of its scan."""
    g = _g28()
    least = 10 ** 9
    for coor in ("camera", "lidar"):
        for scene in kitti_tree.SCENES:
            for track in g["tracks_%s" % scene]:
                for frame, b in zip(g["frames_%s_%d" % (scene, track)], g["box_%s_%s_%d" % (coor, scene, track)]):
                    if (scene, int(frame)) == kitti_tree.MISSING:
                        continue
                    pts = g["scan_%s_%s_%d" % (coor, scene, frame)].astype(np.float64)
                    local = bm.q_rotation_matrix(b[6:]).T @ (pts - b[:3, None])
                    inside = (np.abs(local) < (b[[4, 3, 5]] / 2)[:, None]).all(0)
                    least = min(least, int(inside.sum()))
                    assert 300 <= pts.shape[1] <= 500
    assert least >= 30, least


def test_write_track_results_reproduces_the_reference_line(tree):
    g = _g28()
    scene, frame, number, track = g["line_info"].tolist()
    assert (scene, int(track), int(frame)) == kitti_tree.LINE_ROW
    rows = [r for r in kf.tracklets_of(kf.read_labels(_paths(tree, scene)[1]), "Car") if r["track_id"][0] == int(track)][0]
    row = rows[rows["frame"] == int(frame)][0]
    box = kf.annotation_box(row, kf.read_calib(_paths(tree, scene)[0]), "lidar")
    fp = io.StringIO()
    kf.write_track_results(fp, scene, int(frame), int(number), box)
    line = str(g["line"])
    assert fp.getvalue() == line and line.endswith("\n") and len(line.split()) == 27 and line.split()[:3] == [scene, frame, number]
    # corner 0 is (+l/2, +w/2, +h/2) from the centre, corner 6 its opposite: the order of corners().transpose()
    v = np.array(line.split()[3:], np.float64).reshape(8, 3)
    np.testing.assert_allclose(v[0] - v[6], box[1][[1, 0, 2]], rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------- KittiTrackingScenes, the host half
def test_scenes_tables_and_order(tree):
    from ptt_amd.datasets.kitti.kitti_scenes import KittiTrackingScenes
    g = _g28()
    ks = KittiTrackingScenes(tree, class_name='Car', split='all', ref_coor='lidar')
    assert ks.scenes == ["0000", "0019", "0020"] and ks.store is None                 # ascending scene number; nothing on a device yet
    assert [(m["scene"], m["track_id"]) for m in ks.meta] == [(s, t) for s in ks.scenes for t in (1, 0)]
    for m, boxes in zip(ks.meta, ks.boxes):
        assert m["frames"] == g["frames_%s_%d" % (m["scene"], m["track_id"])].tolist() and len(m["rows"]) == len(boxes) == len(m["frames"])
        want = g["box_lidar_%s_%d" % (m["scene"], m["track_id"])]
        for b, w in zip(boxes, want):
            assert np.array_equal(b[1], w[3:6]) and np.abs(b[2] - w[6:]).max() <= 2.0 ** -50 and np.abs(b[0] - w[:3]).max() <= 1e-9
    assert KittiTrackingScenes(tree, split='test').scenes == ["0019", "0020"] and KittiTrackingScenes(tree, split='train_tiny').scenes == ["0000"]
    assert KittiTrackingScenes(tree, split='val').meta == []
    assert [m["track_id"] for m in KittiTrackingScenes(tree, class_name='Pedestrian', split='test_tiny').meta] == [2]
    assert ks.frames_of("0019") == [0, 1, 2, 3, 4] and ks.steps_of("0019") == []
    cam = KittiTrackingScenes(tree, split='test', ref_coor='CAMERA')
    (kind, m), = cam.steps_of("0020")
    assert kind == 'affine' and np.array_equal(m, cam.calib["0020"].V2C)
    for kw in (dict(ref_coor='ego'), dict(missing='zeros')):
        with pytest.raises(ValueError):
            KittiTrackingScenes(tree, **kw)


def test_replay_adds_drops_and_splits_a_track_at_a_gap(tree, tmp_path):
    import shutil
    from ptt_amd.datasets.kitti.kitti_scenes import KittiTrackingScenes
    ks = KittiTrackingScenes(tree, split='test', ref_coor='camera')
    steps = list(ks.replay("0019"))
    assert [sorted(a) for _, _, a, _ in steps] == [[1], [0], [], [], []] and [d for _, _, _, d in steps] == [(), (), (), (), (1,)]
    for f, (raw, st, add, drop) in enumerate(steps):
        want = np.fromfile(ks.scan_path("0019", f), np.float32).reshape(-1, 4)
        assert raw.dtype == np.float32 and np.array_equal(raw, want) and st[0][0] == 'affine'
    assert np.array_equal(steps[0][2][1][0], ks.boxes[0][0][0])
    # the missing scan of 0020: one origin row and no step; missing='raise' refuses it when its frame comes up
    raw, st, _, _ = list(ks.replay("0020"))[kitti_tree.MISSING[1]]
    assert raw.shape == (1, 4) and not raw.any() and st == []
    with pytest.raises(FileNotFoundError):
        list(KittiTrackingScenes(tree, split='test', missing='raise').replay("0020"))
    with pytest.raises(KeyError):
        next(ks.replay("0000"))
    # a copy of the tree in which track 0 of 0019 loses its row of frame 3: frames 1, 2, 4
    gap = tmp_path / "gap"
    shutil.copytree(tree, str(gap))
    label = gap / "training" / "label_02" / "0019.txt"
    label.write_text("\n".join(l for l in label.read_text().splitlines() if not l.startswith("3 0 Car")) + "\n")
    kg = KittiTrackingScenes(str(gap), split='test')
    assert kg.meta[1]["frames"] == [1, 2, 4]
    steps = list(kg.replay("0019"))
    assert [list(a) for _, _, a, _ in steps] == [[1], [0], [], [], [(0, 1)]] and [d for _, _, _, d in steps] == [(), (), (), (0,), (1,)]
    assert np.array_equal(steps[4][2][(0, 1)][0], kg.boxes[1][2][0])
