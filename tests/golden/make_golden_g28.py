"""Fixture G28 — the reference's own KittiTrackingDataset run on the generated tree of tests/kitti_tree.py (run where the
reference tree is at hand, like make_golden.py; only arrays and one text line are committed).

KittiTrackingDataset (ptt/datasets/kitti/kitti_dataset_tracking.py) is built over write_tree(tmp, SEED) with DATA_SPLIT 'all',
LOAD_FROM_DATABASE False and LIDAR_CROP_OFFSET 10, under REF_COOR camera and lidar, in test mode (whole scans) and in train mode
(get_lidar's preload crop). Recorded:

    scenes                              the scene names
    tracks_<scene>                      track ids of the Car tracklets, in the dataset's order within the scene
    frames_<scene>_<track>              the frames of a tracklet
    box_<coor>_<scene>_<track>          (T, 10) float64: centre, wlh, quaternion elements of get_box per frame
    scan_<coor>_<scene>_<frame>         (3, N) float32: pc.points of a frame in test mode (the missing frame: one origin point)
    crop_<coor>_<scene>_<track>_<frame> (3, n) float32: pc.points in train mode
    line, line_info                     one save_track_results line (ptt/utils/file_io.py:55-65) and its (scene, frame, tracklet
                                        number, track id): the lidar box of kitti_tree.LINE_ROW

The module imports what this container lacks (skimage, tqdm if absent, pyquaternion, easydict): those are registered as stub
modules, pyquaternion as the restated stand-in of make_golden.py; `ptt` and `ptt.datasets` are registered as bare packages over
the reference's directories so that their __init__ (which imports the nuScenes devkit) does not run; torch.cuda.get_device_name
is patched to a name the module's import guard accepts. The scenes come in os.listdir order there; everything is keyed by scene
name, so the order does not enter the file.

Before writing, the script compares ptt_amd.datasets.kitti.kitti_files with what it recorded and reports the observed maxima
(the assertions are the tests' own: tests/test_kitti_files_cpu.py).

    python tests/golden/make_golden_g28.py        # writes tests/golden/G28_kitti_files.npz, and its report line GOLDEN_REPORT_G28.txt
"""
import io
import os
import sys
import tempfile
import types
from pathlib import Path

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests.golden import make_golden as MG          # noqa: E402
from tests import kitti_tree                        # noqa: E402

SEED = 2800
OFFSET = 10


def _package(name, path):
    mod = types.ModuleType(name)
    mod.__path__ = [path]
    sys.modules[name] = mod
    return mod


def _reference_dataset_class():
    EasyDict = MG._install_stubs()                  # pyquaternion stand-in (restated formulas), EasyDict
    _package("ptt", os.path.join(MG.REF, "ptt"))
    _package("ptt.datasets", os.path.join(MG.REF, "ptt", "datasets"))
    sk = types.ModuleType("skimage")
    sk.io = types.ModuleType("skimage.io")
    sys.modules["skimage"], sys.modules["skimage.io"] = sk, sk.io
    try:
        import tqdm                                 # noqa: F401
    except ImportError:
        tq = types.ModuleType("tqdm")
        tq.tqdm = lambda it, *a, **k: it
        sys.modules["tqdm"] = tq
    name = torch.cuda.get_device_name
    torch.cuda.get_device_name = lambda *a, **k: 'GeForce RTX 3090'
    try:
        from ptt.datasets.kitti.kitti_dataset_tracking import KittiTrackingDataset
    finally:
        torch.cuda.get_device_name = name
    from ptt.utils.file_io import save_track_results
    return EasyDict, KittiTrackingDataset, save_track_results


def main():
    EasyDict, Dataset, save_track_results = _reference_dataset_class()
    from ptt_amd.datasets.kitti import kitti_files as kf
    out = {"scenes": np.array(kitti_tree.SCENES), "offset": np.int64(OFFSET), "seed": np.int64(SEED)}
    q_err = c_err = 0.0
    with tempfile.TemporaryDirectory() as tmp:
        info = kitti_tree.write_tree(tmp, SEED)
        for coor in ("camera", "lidar"):
            for training in (False, True):
                cfg = EasyDict(DATA_PATH=tmp, DATA_SPLIT={'train': 'all', 'test': 'all'}, SAMPLED_INTERVAL=1, NUM_CANDIDATES_PERFRAME=4,
                               LIDAR_CROP_OFFSET=OFFSET, LOAD_FROM_DATABASE=False, REF_COOR=coor, POINT_CLOUD_RANGE=[-1, -1, -1, 1, 1, 1])
                ds = Dataset(dataset_cfg=cfg, class_names='Car', training=training, root_path=Path(tmp))
                assert ds.preload_offset == (OFFSET if training else -1)
                tracks = {s: [] for s in kitti_tree.SCENES}
                for k, annos in enumerate(ds.per_sequence_anno):
                    scene, track = annos[0]['scene'], int(annos[0]['track_id'])
                    tracks[scene].append(track)
                    rows, frames = [], []
                    for j in range(len(annos)):
                        d = ds.grab_data(k, j)
                        frame = int(d['anno']['frame'])
                        frames.append(frame)
                        box = d['box']
                        rows.append(np.concatenate([box.center, box.wlh, box.orientation.elements]).astype(np.float64))
                        pts = np.ascontiguousarray(np.asarray(d['pc'].points), np.float32)
                        assert pts.shape[0] == 3
                        key = "crop_%s_%s_%d_%d" % (coor, scene, track, frame) if training else "scan_%s_%s_%d" % (coor, scene, frame)
                        assert key not in out or np.array_equal(out[key].view(np.int32), pts.view(np.int32)), key
                        out[key] = pts
                        if not training and coor == "lidar" and (scene, track, frame) == info["line_row"]:
                            fp = io.StringIO()
                            save_track_results(fp, [d['anno']['scene'], d['anno']['frame'], k], box.corners().transpose())
                            out["line"] = np.array(fp.getvalue())
                            out["line_info"] = np.array([scene, str(frame), str(k), str(track)])
                            assert np.array_equal(box.orientation.elements, [1.0, 0.0, 0.0, 0.0]), box.orientation.elements
                    for key, val in (("frames_%s_%d" % (scene, track), np.array(frames, np.int64)),
                                     ("box_%s_%s_%d" % (coor, scene, track), np.stack(rows))):
                        assert key not in out or np.array_equal(out[key], val), key           # test and train mode agree
                        out[key] = val
                for scene, ids in tracks.items():
                    key = "tracks_%s" % scene
                    assert key not in out or out[key].tolist() == ids
                    out[key] = np.array(ids, np.int64)
        # the repo's readers on the same tree: observed maxima for the report
        base = os.path.join(tmp, "training")
        for scene in kitti_tree.SCENES:
            calib = kf.read_calib(os.path.join(base, "calib", scene + ".txt"))
            for rows in kf.tracklets_of(kf.read_labels(os.path.join(base, "label_02", scene + ".txt")), "Car"):
                for coor in ("camera", "lidar"):
                    want = out["box_%s_%s_%d" % (coor, scene, int(rows["track_id"][0]))]
                    for r, w in zip(rows, want):
                        c, wlh, q = kf.annotation_box(r, calib, coor)
                        q_err = max(q_err, float(np.abs(q - w[6:]).max()))
                        if coor == "lidar":
                            c_err = max(c_err, float(np.abs(c - w[:3]).max()))
    missing = out["scan_camera_%s_%d" % kitti_tree.MISSING]
    assert missing.shape == (3, 1) and not missing.any() and "line" in out
    path = os.path.join(HERE, "G28_kitti_files.npz")
    np.savez_compressed(path, **out)
    n_scans = sum(k.startswith("scan_") for k in out)
    n_crops = sum(k.startswith("crop_") for k in out)
    line = ("G28 KittiTrackingDataset on the generated tree (seed %d): %d scans, %d preload crops (offset %d, %d..%d points), %d bytes; "
            "kitti_files.annotation_box vs reference: quaternion max |diff| %.3e, lidar centre max |diff| %.3e m"
            % (SEED, n_scans, n_crops, OFFSET, min(v.shape[1] for k, v in out.items() if k.startswith("crop_")),
               max(v.shape[1] for k, v in out.items() if k.startswith("crop_")), os.path.getsize(path), q_err, c_err))
    print(line)
    with open(os.path.join(HERE, "GOLDEN_REPORT_G28.txt"), "w") as f:          # a report of its own: GOLDEN_REPORT.txt is left as it is
        f.write(line + "\n")


if __name__ == "__main__":
    main()
