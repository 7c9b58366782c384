"""TEST INFRASTRUCTURE — the reference's tracking loop with its two TEST settings, restated on oracle.tracking_ref's functions:
the checker of TrackletRunner's modes (tests/test_tracking_modes_gpu.py), itself pinned to the reference's own
TrackingEvaluator.prepare_search / prepare_template / post_process by fixture G18 (tests/test_tracking_modes_cpu.py).

Per tracked frame i >= 1 (tools/eval_utils/eval_tracking_utils.py:154-229, 266-274), results[0] = gt[0]:
  ref box   REF_BOX previous_result: results[i-1]; previous_gt: gt[i-1]; current_gt: gt[i]
  search    crop_center_pc(cloud i, ref box, gt[i]) resampled to the search size
  template  get_model over SHAPE_AGGREGATION's (cloud, RESULT box) pairs — firstandprevious [0, i-1], first [0], previous
            [i-1], all [0 .. i-1] — resampled to the template size
  result    get_box_by_offset(ref box, best proposal, use_z): a copy of the ref box, so it keeps the ref box's wlh
"""
import copy

import numpy as np

from oracle import tracking_ref as TR


def template_frames(shape, i):
    """The frames whose crops make frame i's template, in get_model's order (prepare_template :187-216)."""
    return {"firstandprevious": [0, i - 1], "first": [0], "previous": [i - 1], "all": list(range(i))}[shape]


def ref_box(ref, gt_boxes, results, i):
    return {"previous_result": results[i - 1], "previous_gt": gt_boxes[i - 1], "current_gt": gt_boxes[i]}[ref]


def track_modes(clouds, gt_boxes, infer, shape, ref, use_z=True, search_size=1024, template_size=512, offset=0.0,
                scale=1.25, model_offset=0.0, model_scale=1.25):
    """TrackingEvaluator.test_batch for one tracklet in mode (shape, ref) — canonical names, ptt_amd.tracklet_runner.tracking_modes —
    with `infer(search (1,S,3), template (1,T,3)) -> pred_box_data (P,5)`. Returns (result boxes, per-frame records: ref box,
    search, template, model-point count, score), the result boxes starting with the frame-0 ground-truth box."""
    results = [copy.deepcopy(gt_boxes[0])]
    frames = []
    for i in range(1, len(clouds)):
        rb = ref_box(ref, gt_boxes, results, i)
        cand = TR.crop_center_pc(clouds[i], rb, gt_boxes[i].wlh[1], offset=offset, scale=scale)
        search = TR.regularize_pc(cand, search_size)
        ks = template_frames(shape, i)
        model = TR.get_model([clouds[k] for k in ks], [results[k] for k in ks], offset=model_offset, scale=model_scale)
        template = TR.regularize_pc(model, template_size)
        off, score = TR.post_process(np.asarray(infer(search[None], template[None])))
        results.append(TR.get_box_by_offset(rb, off, use_z))
        frames.append({"ref": rb, "search": search, "template": template, "n_model": model.shape[1], "score": score})
    return results, frames


def standin_model(params):
    """A deterministic stand-in for the tracker, defined by data (fixture G18 carries `params`): proposal k's offset is the
    float64 mean of the search rows rows[k] times gain[k] plus kick[k] (a kick larger than the box sends get_box_by_offset
    down its redraw path, :205-208), its angle theta[k] degrees; its score is a fraction formed from the means of those rows
    and of the template rows trows, so that the template takes part and the winner changes from frame to frame."""
    rows, trows = np.asarray(params["rows"]), np.asarray(params["trows"])
    gain, kick, theta = (np.asarray(params[k], np.float64) for k in ("gain", "kick", "theta"))

    def infer(search, template):
        s, t = np.asarray(search, np.float64)[0], np.asarray(template, np.float64)[0]
        m = s[rows].sum(1) / rows.shape[1]                             # (P, 3): sums of a few rows, in a fixed order
        tm = t[trows].sum(0) / len(trows)
        off = m * gain[:, None] + kick
        score = np.mod(1e3 * (m.sum(1) + tm.sum()) + np.arange(len(rows)) * 0.37, 1.0)
        return np.concatenate([off, theta[:, None], score[:, None]], 1).astype(np.float32)
    return infer
