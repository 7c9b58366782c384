"""The KITTI tracking files, read on the host: calibration, label rows, tracklet grouping, annotation -> box, split -> scenes,
and the result line. numpy only; nothing here touches the device (kitti_scenes.py hands the arrays to SceneStore).

Restates what the reference does in KittiTrackingDataset (ptt/datasets/kitti/kitti_dataset_tracking.py:254-296, 315-327, 344-355),
Calibration (ptt/utils/calibration_kitti_tracking.py:6-13, 49-63, 73-92, 129-142) and save_track_results (ptt/utils/file_io.py:55-65,
called from tools/eval_utils/eval_tracking_utils.py:276-280). Fixture G28 (tests/golden/make_golden_g28.py) holds what the
reference's own dataset class gives on a generated tree; tests/test_kitti_files_cpu.py compares these functions with it.

Numbers in the text files are parsed by Python's float(), which rounds correctly; so does the reader the reference uses for the
digits KITTI writes.
"""
import collections

import numpy as np

from . import box_math as bm

LABEL_COLUMNS = ("frame", "track_id", "type", "truncated", "occluded", "alpha", "bbox_left", "bbox_top", "bbox_right", "bbox_bottom",
                 "height", "width", "length", "x", "y", "z", "rotation_y")          # kitti_dataset_tracking.py:281-286
LABEL_DTYPE = np.dtype([(name, 'U32' if name == "type" else (np.int64 if name in ("frame", "track_id") else np.float64))
                        for name in LABEL_COLUMNS])

Calib = collections.namedtuple("Calib", "P2 V2C C2V R0")

# the tracking files' spelling first (calibration_kitti_tracking.py:55-62), then the object-detection one; a trailing colon is dropped
_CALIB_KEYS = {"P2": ("P2",), "V2C": ("Tr_velo_cam", "Tr_velo_to_cam"), "R0": ("R_rect", "R0_rect")}


def read_calib(path):
    """-> Calib(P2 (3,4), V2C (3,4), C2V (3,4), R0 (3,3)), float64. Keys 'P2', 'R_rect' | 'R0_rect', 'Tr_velo_cam' |
    'Tr_velo_to_cam', each with or without a trailing colon; lines that are not numbers are skipped as the reference skips them
    (:90-91). C2V is the rigid inverse [R^T | -R^T t] (:6-13). ValueError names the file and the key that is missing or has the
    wrong number of values."""
    rows = {}
    with open(str(path), 'r') as f:
        for line in f:
            parts = line.split()
            if not parts:
                continue
            try:
                rows[parts[0].rstrip(':')] = np.array([float(v) for v in parts[1:]], np.float64)
            except ValueError:
                pass
    out = {}
    for field, names in _CALIB_KEYS.items():
        found = [n for n in names if n in rows]
        if not found:
            raise ValueError("%s: no %s line" % (path, " / ".join(names)))
        shape = (3, 3) if field == "R0" else (3, 4)
        if rows[found[0]].size != shape[0] * shape[1]:
            raise ValueError("%s: %s has %d values, expected %d" % (path, found[0], rows[found[0]].size, shape[0] * shape[1]))
        out[field] = rows[found[0]].reshape(shape)
    v2c = out["V2C"]
    rot_t = v2c[:, :3].T
    c2v = np.hstack([rot_t, -(rot_t @ v2c[:, 3])[:, None]])
    return Calib(out["P2"], v2c, c2v, out["R0"])


def rect_to_velo(calib, pts):
    """(n, 3) rectified-camera points -> (n, 3) velodyne points: inv(R0), then C2V on the homogeneous points, float64 (:129-142)."""
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    ref = (np.linalg.inv(calib.R0) @ pts.T).T                           # rectified -> reference camera
    return np.hstack([ref, np.ones((len(ref), 1))]) @ calib.C2V.T        # reference camera -> velodyne


def read_labels(path):
    """-> structured array (LABEL_DTYPE) with one row per line of a label_02 file. 17 fields per line; with 18 (a score column, as
    result files carry) the last is ignored. ValueError names the file and the line number for any other count or a field that
    does not parse."""
    rows = []
    with open(str(path), 'r') as f:
        for no, line in enumerate(f, 1):
            parts = line.split()
            if not parts:
                continue
            if len(parts) not in (17, 18):
                raise ValueError("%s line %d: %d fields, expected 17 (or 18 with a score)" % (path, no, len(parts)))
            try:
                rows.append(tuple(p if name == "type" else (int(p) if name in ("frame", "track_id") else float(p))
                                  for name, p in zip(LABEL_COLUMNS, parts)))
            except ValueError:
                raise ValueError("%s line %d: a field is not a number" % (path, no))
    return np.array(rows, LABEL_DTYPE)


def tracklets_of(labels, class_name):
    """The rows of `class_name`, one group per track_id in order of first appearance, rows in file order (:287-295). The frames of
    a group must ascend as they stand (the reference asserts that sorting by frame changes nothing): ValueError otherwise."""
    rows = labels[labels["type"] == class_name]
    groups = []
    for track_id in dict.fromkeys(rows["track_id"].tolist()):
        group = rows[rows["track_id"] == track_id]
        frames = group["frame"].tolist()
        if frames != sorted(frames):
            raise ValueError("track %d of class %s: frames %s are not ascending" % (track_id, class_name, frames))
        groups.append(group)
    return groups


def annotation_box(row, calib, ref_coor):
    """One label row -> (center (3), wlh (3), quaternion (w, x, y, z)), float64, in the frame REF_COOR names (:315-327, 344-355):
      camera   centre (x, y - h/2, z); orientation Q(axis y, ry) . Q(axis x, pi/2)
      lidar    centre rect_to_velo((x, y, z)) with z += h/2; orientation Q(axis z, -(pi/2 + ry))
    wlh = (width, length, height) in both. ValueError for any other ref_coor (compared in upper case, as the reference does)."""
    x, y, z, h = (float(row[k]) for k in ("x", "y", "z", "height"))
    ry = float(row["rotation_y"])
    wlh = np.array([row["width"], row["length"], row["height"]], np.float64)
    frame = str(ref_coor).upper()
    if frame == "CAMERA":
        center = np.array([x, y - h / 2, z], np.float64)
        quat = bm.q_mul(bm.q_from_axis_angle([0.0, 1.0, 0.0], ry), bm.q_from_axis_angle([1.0, 0.0, 0.0], np.pi / 2))
    elif frame == "LIDAR":
        center = rect_to_velo(calib, np.array([x, y, z]).reshape(1, 3))[0]
        center[2] += h / 2
        quat = bm.q_from_axis_angle([0.0, 0.0, 1.0], -(np.pi / 2 + ry))
    else:
        raise ValueError("ref_coor must be camera or lidar, got %r" % (ref_coor,))
    return center, wlh, quat


def scenes_of_split(split):
    """get_scenes (:254-264): the upper-cased split is searched for TRAIN, then VAL, then TEST; with TINY in it the answers are
    [0], [3], [0]; anything else is all 21 scenes."""
    s = str(split).upper()
    tiny = "TINY" in s
    if "TRAIN" in s:
        return [0] if tiny else list(range(0, 17))
    if "VAL" in s:
        return [3] if tiny else list(range(17, 19))
    if "TEST" in s:
        return [0] if tiny else list(range(19, 21))
    return list(range(21))


def write_track_results(fp, scene, frame, tracklet_no, box):
    """One line of the reference's track_result file (file_io.py:55-65): scene, frame and tracklet number, then the box's eight
    corners as corners().transpose() flattened — x y z of corner 0, of corner 1, ... — space-separated, str() of each value.
    box = (center, wlh, quaternion (w, x, y, z))."""
    center, wlh, quat = (np.asarray(v, np.float64).reshape(-1) for v in box)
    corners = bm.corners(center, wlh, bm.q_rotation_matrix(quat))                         # (3, 8)
    values = [scene, frame, tracklet_no] + np.concatenate(corners.transpose(), axis=0).tolist()
    fp.write(" ".join(map(str, values)))
    fp.write("\n")
