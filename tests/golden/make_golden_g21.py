"""Fixture G21 — the REFERENCE's training samples before resampling (run in the build container against /root/reference, like
make_golden_g16.py; only arrays are committed).

KittiTrackingDataset.get_train_items (ptt/datasets/kitti/kitti_dataset_tracking.py:60-107) maps a dataset index to (tracklet,
frame, augmentation), draws the offsets from numpy's global generator, crops the search area with its labels
(prepare_search_and_label :120-149) and the template (prepare_template_data :151-179), and rejects crops of <= 20 points. G21 =
those quantities for every dataset index of a two-tracklet, six-frame synthetic set, with numpy's global generator put into the
state of np.random.RandomState([seed, epoch, index]) in front of each sample — the per-candidate generator of
ptt_amd.train_feed.

The dataset module itself cannot be imported here (it asks torch for a CUDA device's name at import, :15, and needs pandas /
skimage / mayavi), so the METHODS are taken out of its source text with `ast` and run unchanged on a stand-in `self`:
__len__, get_anno_index, get_aug_index, get_frame_seq_map, prepare_search_and_label, prepare_template_data. They call the
reference's own kitti_tracking_utils, in which two names are wrapped for the run: regularize_pc returns its inputs (the fixture
stops in front of the resampling), get_box_by_offset records the offset array it leaves behind (the offsets as used, after
the redraws of :208-211).

    python tests/golden/make_golden_g21.py        # writes tests/golden/G21_train_items.npz
"""
import ast
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests.golden import make_golden as MG          # noqa: E402

SEED, EPOCH = 11, 3
METHODS = ("__len__", "get_anno_index", "get_aug_index", "get_frame_seq_map", "prepare_search_and_label", "prepare_template_data")


def tracklets():
    """Two tracklets of three frames, a few hundred points each; frame 1 of the second is cut to 14 points (every sample of
    that frame is rejected by the search crop, and the samples of frame 2 see it as their previous frame)."""
    from ptt_amd import synth
    a = synth.tracklet(21, 3, n_obj=(60, 150), n_bg=(150, 300))
    b = synth.tracklet(22, 3, n_obj=(60, 150), n_bg=(150, 300))
    b[0][1] = np.ascontiguousarray(b[0][1][:, :14])
    return [a, b]


def main():
    MG._install_stubs()
    sys.path.insert(0, MG.REF)
    from pyquaternion import Quaternion as PQ
    spec = importlib.util.spec_from_file_location("ref_kitti_tracking_utils", os.path.join(MG.REF, "ptt/datasets/kitti/kitti_tracking_utils.py"))
    ku = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ku)
    used = []
    real_box_by_offset = ku.get_box_by_offset

    def box_by_offset(box, offset, use_z=False):
        out = real_box_by_offset(box, offset, use_z)
        used.append(np.array(offset, np.float64))
        return out

    ku.get_box_by_offset = box_by_offset
    ku.regularize_pc = lambda pc, input_size, ratio=1, label=None, reg=None, istrain=True: pc if label is None else (pc, label, reg)
    tree = ast.parse(open(os.path.join(MG.REF, "ptt/datasets/kitti/kitti_dataset_tracking.py")).read())
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "KittiTrackingDataset"][0]
    cls.body = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in METHODS]
    cls.bases = []
    ns = {"np": np, "utils": ku}
    exec(compile(ast.Module(body=[cls], type_ignores=[]), "kitti_dataset_tracking.py", "exec"), ns)
    ds = ns["KittiTrackingDataset"].__new__(ns["KittiTrackingDataset"])

    trks = tracklets()
    cfg = types.SimpleNamespace(USE_Z_AXIS=True, SEARCH_BB_OFFSET=0.0, SEARCH_BB_SCALE=1.25, MODEL_BB_OFFSET=0.0, MODEL_BB_SCALE=1.25,
                                REFINE_BOX_SIZE=True, SEARCH_INPUT_SIZE=1024, TEMPLATE_INPUT_SIZE=512)
    ds.dataset_cfg, ds.debug, ds.training = cfg, False, True
    ds.num_candidates_perframe, ds.sample_interval = 4, 1
    ds.per_sequence_anno = [[None] * len(c) for c, _ in trks]
    ds.per_frame_anno = [a for seq in ds.per_sequence_anno for a in seq]
    ds.frame_seq_map = ds.get_frame_seq_map()
    frame = lambda t, i: {'pc': ku.PointCloud(trks[t][0][i].copy()), 'box': ku.Box(trks[t][1][i][0], trks[t][1][i][1], PQ(array=trks[t][1][i][2]))}

    out = {"seed": SEED, "epoch": EPOCH, "candidates_per_frame": 4, "len": len(ds), "n_tracklets": len(trks),
           "frame_map": np.array([ds.frame_seq_map[k] for k in range(len(ds.frame_seq_map))], np.int64)}
    for t, (clouds, boxes) in enumerate(trks):
        out["n_frames_%d" % t] = len(clouds)
        for i, c in enumerate(clouds):
            out["cloud_%d_%d" % (t, i)] = c
            out["box_%d_%d" % (t, i)] = np.concatenate(boxes[i])
    # the index arithmetic alone, for two intervals (sample_interval enters __len__ and, in __getitem__ :51, the index)
    for interval in (1, 2):
        ds.sample_interval = interval
        n = len(ds)
        out["len_interval_%d" % interval] = n
        out["anno_interval_%d" % interval] = np.array([ds.get_anno_index(k * interval) for k in range(n)], np.int64)
        out["aug_interval_%d" % interval] = np.array([ds.get_aug_index(k * interval) for k in range(n)], np.int64)
    ds.sample_interval = 1
    n_rejected = 0
    for j in range(len(ds)):
        anno, aug = ds.get_anno_index(j), ds.get_aug_index(j)
        t, i = ds.frame_seq_map[anno]
        np.random.set_state(np.random.RandomState([SEED, EPOCH, j]).get_state())
        del used[:]
        pc, label, reg = ds.prepare_search_and_label(frame(t, i), aug)            # get_train_items :73
        search_ok = not isinstance(pc, bool)
        out["search_offset_%d" % j] = used[0]
        if not search_ok:
            # :75-76 the sample is rejected before its template is drawn; the crop that failed is recomputed for the fixture
            sb = real_box_by_offset(frame(t, i)['box'], used[0].copy(), cfg.USE_Z_AXIS)
            pc, label, reg = ku.crop_center_pc(frame(t, i)['pc'], sb, frame(t, i)['box'], sample_offsets=used[0], offset=0.0, scale=1.25,
                                               refine_box=True)
            assert pc.nbr_points() <= 20
        out["search_%d" % j] = np.asarray(pc.points, np.float32)
        out["label_%d" % j] = np.asarray(label, np.float64)
        out["reg_%d" % j] = np.asarray(reg, np.float64)
        valid = search_ok
        if search_ok:
            tpl = ds.prepare_template_data([frame(t, 0), frame(t, max(i - 1, 0))], aug)     # :85-96
            out["template_offset_%d" % j] = used[1]
            valid = not isinstance(tpl, bool)
            if valid:
                out["template_%d" % j] = np.asarray(tpl.points, np.float32)
        out["valid_%d" % j] = bool(valid)
        n_rejected += not valid
    assert n_rejected >= 1 and n_rejected < len(ds)
    np.savez_compressed(os.path.join(HERE, "G21_train_items.npz"), **out)
    print("G21 written: %d samples, %d rejected" % (len(ds), n_rejected))


if __name__ == "__main__":
    main()
