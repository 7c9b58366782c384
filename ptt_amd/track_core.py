"""TrackCore — one step of the tracking loop at one model width W, shared by the three drivers that advance targets frame by
frame: TrackletRunner (lockstep groups), PackedTrackletRunner (refilled slots) and OnlineTracker (live scans).

    host    the driver writes the cloud fields and float64 crop bounds of 2 W jobs into the core's pinned crop table
    device  enqueue(): table upload, ONE crop launch, ptt_regularize_f32 straight into the model's static input buffers, read-back
            of the draw counts, the model (hipGraph replay, best proposal selected on the device), read-back of the (W,5) result
    host    wait(), then update(): ptt_track_select_update moves the float64 boxes

The core owns every buffer those launches address, and so the one rule for when the resampling table, which holds their addresses,
is built and sent again (ready). The table builders below take addresses and sizes, not tensors: plain numpy.
"""
import numpy as np
import torch

from . import ops
from .hot_path import GraphedHotPath, TrackerThroughput

# the template's segments in get_model's order (prepare_template, eval_tracking_utils.py:187-216): firstandprevious [PC_0, PC_{i-1}],
# first [PC_0], previous [PC_{i-1}] — slot 1 holds frame 0's crop, slot 2 the per-frame crop; all: the store (TrackletRunner._store_tables)
TEMPLATE_SLOTS = {"firstandprevious": (1, 2), "first": (1,), "previous": (2,), "all": ()}


def slot_pointers(crop_out, counts, n, cap):
    """The crop slots of `n` targets — a (n, 3, cap, 3) float32 buffer at address `crop_out`: slot 0 search, 1 first-frame, 2
    previous-frame template segment — and their (n, 3) int32 device counts at `counts` -> (out_ptr, cnt_ptr), both (n, 3) uint64."""
    k = np.arange(n)[:, None] * 3 + np.arange(3)[None]
    return (crop_out + k * (cap * 12)).astype(np.uint64), (counts + k * 4).astype(np.uint64)


def unit_boxes(n):
    """n TRACK_BOX records of a unit box (wlh 1, identity quaternion): what an empty slot holds, never used."""
    boxes = np.zeros(n, ops.TRACK_BOX)
    boxes['wlh'], boxes['quat'][..., 0] = 1.0, 1.0
    return boxes


def resample_table(shape, out_ptr, cnt_ptr, cap, search, template, info, search_size, template_size):
    """The 2 W resampling jobs (job 2w: target w's search cloud, 2w + 1: its template) from the crop slots (slot_pointers) into the
    model inputs at `search` (W, search_size, 3) / `template` (W, template_size, 3), their (n, draws used) pairs into the (W, 2, 2)
    int32 buffer at `info`. They change only when one of those buffers moves."""
    W = len(out_ptr)
    rj = np.zeros(2 * W, ops.REGULARIZE_JOB)
    s, t = rj[0::2], rj[1::2]
    s['seg'][:, 0], s['seg_count'][:, 0], s['seg_capacity'][:, 0] = out_ptr[:, 0], cnt_ptr[:, 0], cap
    s['n_seg'], s['input_size'] = 1, search_size
    s['out'], s['info'] = search + np.arange(W) * (search_size * 3 * 4), info + np.arange(W) * 16
    slots = TEMPLATE_SLOTS[shape]
    for k, slot in enumerate(slots):
        t['seg'][:, k], t['seg_count'][:, k], t['seg_capacity'][:, k] = out_ptr[:, slot], cnt_ptr[:, slot], cap
    t['n_seg'], t['input_size'] = max(1, len(slots)), template_size
    t['out'], t['info'] = template + np.arange(W) * (template_size * 3 * 4), info + np.arange(W) * 16 + 8
    return rj


def main_crop_fields(jobs, out_ptr, cnt_ptr, cap):
    """Clear the crop table `jobs` (2 W main entries, then any admission entries) and write what no tracked frame changes: job 2w,
    the search crop -> slot 0; job 2w + 1, the previous-frame template segment -> slot 2; `cap` points each; nothing appends."""
    jobs[:] = np.zeros((), ops.CROP_JOB)
    jobs['capacity'] = cap
    main = jobs[:2 * len(out_ptr)]
    main['out'][0::2], main['count'][0::2] = out_ptr[:, 0], cnt_ptr[:, 0]
    main['out'][1::2], main['count'][1::2] = out_ptr[:, 2], cnt_ptr[:, 2]


def admission_fields(jobs, slots, out_ptr, cnt_ptr, cap):
    """The first len(slots) entries of `jobs`, cleared and pointed at crop slot 1 of the targets `slots`: the first-frame template
    crop (get_model's first segment, fixed for the target's life) of targets that start on this frame — only of those: an empty job
    would zero a continuing target's count. -> those entries; the caller fills the cloud fields and the bounds (cloud 0 around box
    0 with model_offset / model_scale)."""
    aj = jobs[:len(slots)]
    aj[:] = np.zeros((), ops.CROP_JOB)
    aj['out'], aj['count'], aj['capacity'] = out_ptr[slots, 1], cnt_ptr[slots, 1], cap
    return aj


class _BoxedForward(object):
    """tracker forward + best-proposal selection as ONE capturable callable: (search, template) -> (B,5) rows, the best
    proposal of each frame picked on the device (ptt_select_box_f32) — or, select=False, all (B,P,5) proposals: at a handful of
    tracklets the host takes the arg-max itself from the one read-back it makes anyway (np.argmax, the reference's own
    post_process, eval_tracking_utils.py:267-269): one launch less on a chain where launches are what a frame costs."""

    def __init__(self, tracker, select=True):
        self.fwd, self.select = TrackerThroughput(tracker), select

    def __call__(self, search, template):
        boxes = self.fwd(search, template)['pred_box_data'].contiguous()
        return ops.select_box(boxes) if self.select else boxes


class TrackCore(object):
    def __init__(self, tracker, device, width, search_size=1024, template_size=512, search_offset=0.0, search_scale=1.25,
                 model_offset=0.0, model_scale=1.25, use_z=True, use_graph=True, shape="firstandprevious", admissions=0,
                 few=False, info=None):
        """`tracker`, the sizes / offsets / scales and use_z as TrackletRunner's; `width`: the batch the model runs at; `shape`: one of
        tracklet_runner.SHAPE_AGGREGATIONS. admissions: entries of the crop table behind the 2 * width main jobs, for first-frame
        crops that ride in a step's launch (admission_jobs). few: a handful of targets (2 * width <= ops.CROP_JOBS_BY_VALUE_MAX) —
        the crop table rides in the crop launch's arguments (no upload) and all (width, P, 5) proposals are read back for the host's
        arg-max (_BoxedForward): two launches less per frame. info: a (width, 2, 2) int32 device tensor that takes the resampling's
        (n, draws used) pairs instead of the core's own."""
        self.tracker, dev, W = tracker, torch.device(device), int(width)
        self.device, self.W = dev, W
        self.S, self.T = int(search_size), int(template_size)
        self.search_offset, self.search_scale = float(search_offset), float(search_scale)
        self.model_offset, self.model_scale = float(model_offset), float(model_scale)
        self.use_z, self.use_graph, self.shape, self.few = bool(use_z), use_graph, shape, bool(few)
        self.search = torch.zeros((W, self.S, 3), dtype=torch.float32, device=dev)
        self.template = torch.zeros((W, self.T, 3), dtype=torch.float32, device=dev)
        self.counts = torch.zeros((W, 3), dtype=torch.int32, device=dev)          # search, first-frame, previous-frame
        self.info = torch.zeros((W, 2, 2), dtype=torch.int32, device=dev) if info is None else info     # (n, draws used) of search / template
        self.cap, self.crop_out, self.out_ptr, self.cnt_ptr = 0, None, None, None
        nbytes = (2 * W + int(admissions)) * ops.CROP_JOB.itemsize
        self.jobs_dev = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        self.jobs_host = torch.zeros(nbytes, dtype=torch.uint8).pin_memory()      # staging: the host waits for every step's result
        self.jobs = self.jobs_host.numpy().view(ops.CROP_JOB)                     # before it rewrites the table
        self.reg_jobs_dev = torch.zeros(2 * W * ops.REGULARIZE_JOB.itemsize, dtype=torch.uint8, device=dev)
        self.draws = ops.mt19937_draws(dev, max(8192, 4 * max(self.S, self.T) + 1024))
        self.model = _BoxedForward(tracker, select=not self.few)
        # GraphedHotPath of `model` (its static inputs ARE search / template), ops.StateWatch of the tracker as of its capture; the
        # resampling table and what its copy on the device addresses
        self.graph = self._watch = self.reg_jobs = self._table = None
        self.info_host = torch.empty((W, 2, 2), dtype=torch.int32).pin_memory()
        self.result_host = self._read = None                         # (W,5), or (W,P,5) for `few`: sized by the first result; numpy views
        self._done = torch.cuda.Event()

    def reserve(self, cap):
        """Crop slots of `cap` points per crop: grow-only, a larger request moves them (and their pointer tables)."""
        if cap > self.cap:
            self.cap = int(cap)
            self.crop_out = torch.zeros((self.W, 3, self.cap, 3), dtype=torch.float32, device=self.device)
            self.out_ptr, self.cnt_ptr = slot_pointers(self.crop_out.data_ptr(), self.counts.data_ptr(), self.W, self.cap)

    def ready(self, cap):
        """Before a run or a step: drop a model graph captured before the tracker's weights or cached parameters changed (load_state_dict,
        training, train() / eval(): it would replay the old weights, or read freed buffers), capture one if there is none, make the crop
        slots hold `cap` points, and build and upload the resampling table if anything it addresses moved since its last upload."""
        if self._watch is not None and self._watch.changed():
            self.graph = self._watch = None
        if self.use_graph and self.graph is None:
            with torch.no_grad():
                self.graph = GraphedHotPath(self.model, self.search, self.template, watch=False)
            self.search, self.template = self.graph.search, self.graph.template
            self._watch = ops.StateWatch(self.tracker)
        self.reserve(cap)
        table = (self.search.data_ptr(), self.template.data_ptr(), self.crop_out.data_ptr(), self.cap)
        if table != self._table:
            self.reg_jobs = resample_table(self.shape, self.out_ptr, self.cnt_ptr, self.cap, table[0], table[1], self.info.data_ptr(),
                                           self.S, self.T)
            self.upload_resampling()
            self._table = table

    def upload_resampling(self):                                  # fixed address: captured graphs read the table when they replay
        ops.upload_jobs(self.reg_jobs, self.reg_jobs_dev)

    def write_main_jobs(self):
        main_crop_fields(self.jobs, self.out_ptr, self.cnt_ptr, self.cap)

    def bounds(self, boxes, extra, ref=None):
        """The float64 bounds of the 2 * width main jobs (ptt_track_crop_bounds, microseconds for 48 boxes): the search crops around
        `ref` (the REF_BOX boxes; None: `boxes`) with the margin `extra` (gt wlh[1] * 0.6), the template crops around `boxes`."""
        ops.track_crop_bounds(boxes if ref is None else ref, self.search_offset, self.search_scale, extra, self.jobs[0::2], job_stride=2)
        ops.track_crop_bounds(boxes, self.model_offset, self.model_scale, None, self.jobs[1::2], job_stride=2)

    def admission_jobs(self, slots, table=None):
        """admission_fields over the current crop slots into `table` (default: the entries behind the main jobs: the same launch)."""
        return admission_fields(self.jobs[2 * self.W:] if table is None else table, slots, self.out_ptr, self.cnt_ptr, self.cap)

    def crop(self, n_jobs, crop=None):
        """The crop launch over the table's first n_jobs entries: by value (`few`), else table upload, then ops.crop_compact or
        `crop(jobs, jobs_dev, n_jobs)`."""
        if self.few:
            return ops.crop_compact_host(self.jobs, n_jobs, self.device)
        self.jobs_dev.copy_(self.jobs_host, non_blocking=True)
        crop(self.jobs, self.jobs_dev, n_jobs) if crop is not None else ops.crop_compact(self.jobs_dev, n_jobs)

    def enqueue(self, n_jobs, crop=None):
        """One step's device work on the current stream: the crop launch, resampling into the model's input buffers, the
        model, the two read-backs, and the event wait() waits for."""
        self.crop(n_jobs, crop)
        ops.regularize(self.reg_jobs_dev, 2 * self.W, self.draws)
        self.info_host.copy_(self.info, non_blocking=True)       # behind the resampling, ahead of the model: off the frame's tail
        with torch.no_grad():
            rows = self.graph() if self.use_graph else self.model(self.search, self.template)     # inputs are in the static buffers
        if self.result_host is None or self.result_host.shape != rows.shape:
            self.result_host = torch.empty(tuple(rows.shape), dtype=torch.float32).pin_memory()
            self._read = (self.result_host.numpy(), self.info_host.numpy())
        self.result_host.copy_(rows, non_blocking=True)          # float32 rows: x, y, z, theta (degrees), score
        self.mark()

    def mark(self):                                               # wait() waits for everything enqueued on the current stream so far
        self._done.record(torch.cuda.current_stream(self.device))

    def wait(self):
        self._done.synchronize()

    def update(self, boxes, active, rng_pos, est_buf, ref=None, read=None):
        """post_process (eval_tracking_utils.py:266-274) in one call (ptt_track_select_update) on the two pinned read-backs (or
        `read` = (proposals, info) host arrays): the first arg-max of the scores where the read-back is (W,P,5) (:267-269), box_i =
        get_box_by_offset(box_{i-1}, best proposal, USE_Z_AXIS) for the `active` slots. `ref`: the REF_BOX boxes — post_process :270
        moves the REF box (and keeps its wlh) — None = the current results. An implausibly large x / y offset is redrawn from
        numpy's GLOBAL generator (:205-208), whose state then is "seeded with 1 and advanced by the template's (else the search's)
        resampling draws" — the draw counts come back with the boxes (rng_pos); a draw table that ran out raises. est_buf: the rows."""
        if ref is not None:
            boxes[active != 0] = ref[active != 0]
        est, info = self._read if read is None else read
        ops.track_select_update(est, info, boxes, self.use_z, active, rng_pos, est_buf)
