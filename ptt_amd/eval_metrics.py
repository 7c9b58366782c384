"""Success / Precision of a tracking run — the reference's tools/eval_utils/eval_tracking_metrics.py with the same names
(estimateOverlap, estimateAccuracy, Success, Precision), so that its evaluator can import this module in place of its own.

What differs is where the work happens. The reference intersects two shapely polygons per frame on the host; here every
(ground truth, result) pair of an evaluation goes through ONE launch of ptt_box_overlap_f64 (ptt_amd/csrc/track_ops.hip): the
footprints, their intersection, the overlap and the centre distance in float64 on the device. shapely is not needed. The two
21-point curves are comparisons over a host array and stay on the host, vectorised.

  estimateOverlap / estimateAccuracy   one pair (a launch and a read-back each: the drop-in form)
  overlaps                             any number of pairs: one upload, one launch, one read-back
  Success / Precision                  the reference's accumulators, plus extend() for arrays
  evaluate                             results of TrackletRunner.run / run_overlapped + their tracklets -> the numbers the
                                       reference reports (Success, Precision), overall and per tracklet

There is no CPU fallback: without a HIP device the overlap functions raise.
"""
import numpy as np
import torch

from . import ops

# np.trapz, by the name numpy 2 gives it (the old name warns there)
_trapz = getattr(np, "trapezoid", None) or np.trapz


def _row(box):
    """A box as 10 float64: centre, wlh, quaternion (w, x, y, z). Takes the mirror's Box (ptt.datasets.kitti.kitti_tracking_utils) —
    anything with .center, .wlh and .orientation.elements — or a (center, wlh, quat[, score]) tuple as TrackletRunner.run returns."""
    if hasattr(box, "center"):
        parts = (box.center, box.wlh, box.orientation.elements)
    else:
        parts = box[0:3]
    row = np.concatenate([np.asarray(p, np.float64).reshape(-1) for p in parts])
    if row.shape != (10,):
        raise ValueError("a box is centre (3), wlh (3) and quaternion (4), got %d numbers" % row.size)
    return row


def _device(device):
    if device is not None:
        return torch.device(device)
    if not torch.cuda.is_available():
        raise RuntimeError("ptt_amd.eval_metrics computes overlaps on the HIP device; none is visible (there is no CPU fallback)")
    return torch.device('cuda', torch.cuda.current_device())


def overlaps(gt_boxes, pred_boxes, ref_coord, dim=3, device=None):
    """estimateOverlap(gt, pred, dim, ref_coord) and estimateAccuracy(gt, pred, dim) for every pair of two equally long lists of
    boxes -> (overlap, accuracy), numpy float64 arrays. One upload, one launch, one read-back."""
    if len(gt_boxes) != len(pred_boxes):
        raise ValueError("%d ground-truth boxes against %d result boxes" % (len(gt_boxes), len(pred_boxes)))
    n = len(gt_boxes)
    host = np.empty((2, n, 10), np.float64)
    for k, boxes in enumerate((gt_boxes, pred_boxes)):
        for i, box in enumerate(boxes):
            host[k, i] = _row(box)
    dev = torch.from_numpy(host).to(_device(device))
    out = torch.empty((2, n), dtype=torch.float64, device=dev.device)
    ops.box_overlap(dev[0], dev[1], ref_coord, dim, out=out)
    res = out.cpu().numpy()
    return res[0], res[1]


def estimateOverlap(box_a, box_b, dim=2, ref_coord='camera'):
    """eval_tracking_metrics.py:52-74 for one pair -> float."""
    return float(overlaps([box_a], [box_b], ref_coord, dim)[0][0])


def estimateAccuracy(box_a, box_b, dim=3):
    """eval_tracking_metrics.py:37-42 for one pair -> float (ref_coord plays no part in it)."""
    return float(overlaps([box_a], [box_b], 'camera', dim)[1][0])


class Success(object):
    """eval_tracking_metrics.py:77-113: the share of frames whose overlap is >= each of n thresholds in [0, max_overlap], and
    the area under that curve in per cent."""

    def __init__(self, n=21, max_overlap=1):
        self.max_overlap = max_overlap
        self.Xaxis = np.linspace(0, self.max_overlap, n)
        self.reset()

    def reset(self):
        self.overlaps = []

    def add_overlap(self, val, index=None):
        self.overlaps.append(val)

    def extend(self, values):
        self.overlaps.extend(np.asarray(values, np.float64).reshape(-1).tolist())

    @property
    def count(self):
        return len(self.overlaps)

    @property
    def value(self):
        hits = np.asarray(self.overlaps, np.float64)[None, :] >= self.Xaxis[:, None]
        with np.errstate(invalid='ignore'):                       # an empty meter: 0 / 0, as in the reference
            return hits.sum(1).astype(float) / np.float64(self.count)

    @property
    def average(self):
        if len(self.overlaps) == 0:
            return 0
        return _trapz(self.value, x=self.Xaxis) * 100 / self.max_overlap


class Precision(object):
    """eval_tracking_metrics.py:116-154: the share of frames whose centre distance is <= each of n thresholds in
    [0, max_accuracy] metres, and the area under that curve in per cent."""

    def __init__(self, n=21, max_accuracy=2):
        self.max_accuracy = max_accuracy
        self.Xaxis = np.linspace(0, self.max_accuracy, n)
        self.reset()

    def reset(self):
        self.accuracies = []

    def add_accuracy(self, val, index=None):
        self.accuracies.append(val)

    def extend(self, values):
        self.accuracies.extend(np.asarray(values, np.float64).reshape(-1).tolist())

    @property
    def count(self):
        return len(self.accuracies)

    @property
    def value(self):
        hits = np.asarray(self.accuracies, np.float64)[None, :] <= self.Xaxis[:, None]
        with np.errstate(invalid='ignore'):
            return hits.sum(1).astype(float) / np.float64(self.count)

    @property
    def average(self):
        if len(self.accuracies) == 0:
            return 0
        return _trapz(self.value, x=self.Xaxis) * 100 / self.max_accuracy


def evaluate(results, tracklets, ref_coord='lidar', dim=3, device=None):
    """Success / Precision of a run: `results` is what TrackletRunner.run / run_overlapped returned, `tracklets` what they were
    given ((clouds, ground-truth boxes) per tracklet). Every frame of every tracklet is scored against its ground-truth box,
    frame 0 (whose result IS the ground truth) included, as the reference's test_batch does
    (tools/eval_utils/eval_tracking_utils.py:96-112); all frames share one launch. -> dict:
      success, precision                      over all frames (the reference's Success_main / Precision_main averages)
      success_curve, precision_curve          their 21-point curves
      overlap, accuracy                       per frame, tracklet after tracklet; frames = the tracklets' lengths
      tracklet_success, tracklet_precision    per tracklet (what the reference logs as Success_batch / Precision_batch)"""
    if len(results) != len(tracklets):
        raise ValueError("%d result lists for %d tracklets" % (len(results), len(tracklets)))
    gt, pred, frames = [], [], []
    for t, (res, (_, boxes)) in enumerate(zip(results, tracklets)):
        if len(res) != len(boxes):
            raise ValueError("tracklet %d: %d result boxes for %d frames" % (t, len(res), len(boxes)))
        gt.extend(boxes)
        pred.extend(res)
        frames.append(len(boxes))
    overlap, accuracy = overlaps(gt, pred, ref_coord, dim, device)
    main_s, main_p = Success(), Precision()
    main_s.extend(overlap)
    main_p.extend(accuracy)
    per_s, per_p = np.zeros(len(frames)), np.zeros(len(frames))
    batch_s, batch_p, start = Success(), Precision(), 0
    for t, n in enumerate(frames):
        batch_s.reset()
        batch_p.reset()
        batch_s.extend(overlap[start:start + n])
        batch_p.extend(accuracy[start:start + n])
        per_s[t], per_p[t], start = batch_s.average, batch_p.average, start + n
    return {"success": float(main_s.average), "precision": float(main_p.average),
            "success_curve": main_s.value, "precision_curve": main_p.value,
            "overlap": overlap, "accuracy": accuracy, "frames": np.array(frames, np.int64),
            "tracklet_success": per_s, "tracklet_precision": per_p}
