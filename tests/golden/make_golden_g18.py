"""Fixture G18 — the reference's tracking loop in all twelve TEST modes (SHAPE_AGGREGATION first / previous / firstandprevious /
all x REF_BOX previous_result / previous_gt / current_gt; run in the build container against /root/reference, like
make_golden.py; only arrays are committed).

The REFERENCE's own TrackingEvaluator.prepare_search / prepare_template / post_process (tools/eval_utils/eval_tracking_utils.py:
154-229, 266-274) drive two tracklets frame by frame on the CPU, with the model replaced by a deterministic stand-in defined by
data (tests/tracking_modes_ref.standin_model; one proposal's x offset exceeds the box, so get_box_by_offset redraws from numpy's
global generator): G12's six-frame tracklet, and a seven-frame synthetic one whose ground-truth wlh changes from frame to frame
and whose first-frame crop is empty. Recorded per frame: the ref box, the result box, the model-point count (get_model's
output before resampling) and the search / template clouds. The sizes are 256 / 128 points to keep the file small. Each frame
is also checked here against the repo's restatement (tests/tracking_modes_ref.track_modes).

The reference's evaluator module imports what this container lacks (shapely / skimage through its metrics module and
ptt.utils): those imports are registered as stub modules, the two files are loaded by path, __init__ is skipped, and
torch.Tensor.cuda is the identity while the script runs.

    python tests/golden/make_golden_g18.py        # writes tests/golden/G18_tracking_modes.npz
"""
import copy
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests.golden import make_golden as MG          # noqa: E402

SHAPES = ("firstandprevious", "first", "previous", "all")
REFS = ("previous_result", "previous_gt", "current_gt")
SIZES = dict(SEARCH_BB_OFFSET=0.0, SEARCH_BB_SCALE=1.25, MODEL_BB_OFFSET=0.0, MODEL_BB_SCALE=1.25, SEARCH_INPUT_SIZE=256,
             TEMPLATE_INPUT_SIZE=128)
PARAMS = {"rows": np.arange(16).reshape(4, 4) * 13 % 256, "trows": np.array([0, 31, 64, 127]),
          "gain": np.array([0.5, 0.3, 0.4, 0.2]), "theta": np.array([2.0, -3.0, 5.0, 0.5]),
          "kick": np.array([[0.0, 0.0, 0.0], [6.0, 0.0, 0.0], [0.0, 0.0, 0.05], [0.2, 3.5, 0.0]])}


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def _package(name):
    mod = types.ModuleType(name)
    mod.__path__ = []
    sys.modules[name] = mod
    return mod


def _reference_modules():
    EasyDict = MG._install_stubs()                  # pyquaternion stand-in (restated formulas), EasyDict
    for pkg in ("ptt", "ptt.utils", "ptt.datasets", "ptt.datasets.kitti", "tools", "tools.eval_utils"):
        _package(pkg)
    common = types.ModuleType("ptt.utils.common_utils")
    common.set_manual_seed = lambda seed: np.random.seed(int(seed))      # the numpy part of set_manual_seed (common_utils.py:115-123)
    common.MovingAverage = object
    metrics = types.ModuleType("tools.eval_utils.eval_tracking_metrics")
    metrics.Evaluator = metrics.AverageMeter = object
    for name, mod in (("ptt.utils.common_utils", common), ("ptt.utils.timer_utils", types.ModuleType("ptt.utils.timer_utils")),
                      ("ptt.utils.file_io", types.ModuleType("ptt.utils.file_io")),
                      ("tools.eval_utils.eval_tracking_metrics", metrics)):
        sys.modules[name] = mod
    sys.modules["ptt.utils.file_io"].save_track_results = None
    sys.modules["ptt.utils"].common_utils = common
    ku = _load("ptt.datasets.kitti.kitti_tracking_utils", os.path.join(MG.REF, "ptt/datasets/kitti/kitti_tracking_utils.py"))
    sys.modules["ptt.datasets.kitti"].kitti_tracking_utils = ku
    ev = _load("ref_eval_tracking_utils", os.path.join(MG.REF, "tools/eval_utils/eval_tracking_utils.py"))
    return EasyDict, ku, ev


def synthetic_tracklet():
    """Seven frames; the ground-truth wlh changes every frame; frame 0's cloud lies far from its box (an empty first crop)."""
    from ptt_amd import synth
    clouds, boxes = synth.tracklet(1811, 7, n_obj=(80, 200), n_bg=(150, 400))
    out = []
    for i, (c, wlh, q) in enumerate(boxes):
        out.append((c, wlh * np.array([1.0 + 0.08 * np.sin(i), 1.0 + 0.1 * np.cos(1.3 * i), 1.0 + 0.05 * i]), q))
    clouds[0] = np.ascontiguousarray(clouds[0] + np.array([[40.0], [0.0], [0.0]], np.float32))
    return clouds, out


def main():
    EasyDict, ku, E = _reference_modules()
    from pyquaternion import Quaternion as PQ
    from tests import tracking_modes_ref as TM
    from oracle import tracking_ref as TR
    g12 = np.load(os.path.join(HERE, "G12_tracking_pre_post.npz"))
    T12 = int(g12["n_frames"])
    tracklets = [([g12["cloud_%d" % i] for i in range(T12)], [(g12["gt_center_%d" % i], g12["wlh"], g12["gt_quat_%d" % i])
                                                              for i in range(T12)]), synthetic_tracklet()]
    out = {"n_tracklets": len(tracklets), "shapes": np.array(SHAPES), "refs": np.array(REFS),
           "sizes": np.array([SIZES["SEARCH_INPUT_SIZE"], SIZES["TEMPLATE_INPUT_SIZE"]])}
    out.update({"param_" + k: v for k, v in PARAMS.items()})
    infer = TM.standin_model(PARAMS)
    n_models = []
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        for t, (clouds, boxes) in enumerate(tracklets):
            out["n_frames_%d" % t] = len(clouds)
            for i, (c, (center, wlh, q)) in enumerate(zip(clouds, boxes)):
                out["cloud_%d_%d" % (t, i)] = np.asarray(c, np.float32)
                out["gt_%d_%d" % (t, i)] = np.concatenate([center, wlh, q])
            for shape in SHAPES:
                for ref in REFS:
                    ev = E.TrackingEvaluator.__new__(E.TrackingEvaluator)
                    ev.cfg = EasyDict(TEST={"SHAPE_AGGREGATION": shape, "REF_BOX": ref}, DATA_CONFIG={"USE_Z_AXIS": True})
                    ev.dataset = EasyDict(dataset_cfg=dict(SIZES))
                    PCs = [ku.PointCloud(np.array(c, np.float32)) for c in clouds]
                    BBs = [ku.Box(center, wlh, PQ(array=q)) for center, wlh, q in boxes]
                    ev.ret_dict = {"results_BBs": [BBs[0]], "PCs": PCs, "BBs": BBs}
                    seen = []
                    get_model = ku.get_model

                    def counted(*a, **k):
                        pc = get_model(*a, **k)
                        seen.append(pc.points.shape[1])
                        return pc
                    ku.get_model = counted
                    try:
                        for i in range(1, len(clouds)):
                            ev.ret_dict.update({"this_BB": BBs[i], "this_PC": PCs[i]})
                            ev.prepare_search(i)
                            ev.prepare_template(i)
                            search = ev.ret_dict["candidate_PC"][0].numpy()
                            template = ev.ret_dict["model_PC"][0].numpy()
                            ev.ret_dict["model_output"] = {"pred_box": torch.from_numpy(infer(search[None], template[None]))[None]}
                            ev.post_process()
                            key = "%d_%s_%s_%d" % (t, shape, ref, i)
                            rb, res = ev.ret_dict["ref_BB"], ev.ret_dict["results_BBs"][-1]
                            out["ref_" + key] = np.concatenate([rb.center, rb.wlh, rb.orientation.elements])
                            out["res_" + key] = np.concatenate([res.center, res.wlh, res.orientation.elements])
                            out["search_" + key], out["template_" + key] = search.astype(np.float32), template.astype(np.float32)
                            out["nmodel_" + key] = seen[-1]
                            n_models.append(seen[-1])
                    finally:
                        ku.get_model = get_model
                    # the repo's restatement of the same loop: every frame identical
                    res, frames = TM.track_modes(clouds, [TR.RefBox(*b) for b in boxes], infer, shape, ref, use_z=True,
                                                 search_size=SIZES["SEARCH_INPUT_SIZE"], template_size=SIZES["TEMPLATE_INPUT_SIZE"])
                    for i in range(1, len(clouds)):
                        key = "%d_%s_%s_%d" % (t, shape, ref, i)
                        f, r = frames[i - 1], res[i]
                        assert np.array_equal(f["search"], out["search_" + key]), key
                        assert np.array_equal(f["template"], out["template_" + key]), key
                        assert f["n_model"] == out["nmodel_" + key], key
                        assert np.array_equal(np.concatenate([r.center, r.wlh, r.quat.q]), out["res_" + key]), key
    finally:
        torch.Tensor.cuda = cuda
    np.savez_compressed(os.path.join(HERE, "G18_tracking_modes.npz"), **out)
    print("G18 written: %d tracklets x %d modes, model-point counts %d..%d; restatement == reference bitwise"
          % (len(tracklets), len(SHAPES) * len(REFS), min(n_models), max(n_models)))


if __name__ == "__main__":
    main()
