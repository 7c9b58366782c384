"""OnlineTracker — the tracking loop on LIVE data: one full LiDAR scan per step, several targets that come and go, no ground truth.

TrackletRunner (tracklet_runner.py) is an evaluation harness: it wants every cloud of every tracklet before the first frame,
pre-cropped around the ground truth, with a ground-truth box per frame. A live integrator has one scan per time step and a box
per target from its own detector at the moment the target appears. OnlineTracker is the entry point for that:

    ot = OnlineTracker(tracker, device, slots=8)
    boxes = ot.step(scan, add={7: (center, wlh, quat)})      # target 7 initialised on this scan: its frame 0
    boxes = ot.step(scan)                                    # {7: (center, wlh, quat, score)}
    boxes = ot.step(scan, add={9: ...}, drop=(7,))
    boxes = ot.step_raw(raw, steps=[('affine', V2C)])        # the sensor's (N, C) rows: de-interleaved and transformed on the device

What a step computes for a continuing target is what TrackletRunner._steps computes for frame i of a tracklet whose clouds are
the scans since the target's `add`, with REF_BOX = previous_result — bit for bit, because both drive the same TrackCore
(track_core.py) at width = slots: the same job tables, resampling, model graph and float64 box update, one step at a time.
The first-frame crops of a step's new targets are a launch of their own BEHIND the model, from a staging table of their own: the
core's pinned table is still being read by that step's upload when they are written (so admissions=0, and TrackCore.admission_jobs
writes into the table it is given). New here are only the life cycle of the slots (SlotTable), the two resident scan buffers,
and the crop kernel: a scan is 35k - 130k points, so the crops go through ptt_crop_scan_f32 (every job spread over the chip)
from SCAN_CROP_MIN_POINTS points on, through ptt_crop_compact_f32 (one workgroup per job) below — identical results.

    host    crop bounds of the live boxes (float64)                         -> one 2 * slots job table, one upload
    device  scan -> one of two resident (3, scan_capacity) buffers          (the previous scan stays alive: its crop around the
                                                                             previous result is the template's `previous` segment)
            crop    job 2s: this scan around target s's previous result, job 2s + 1: the previous scan around it (eager)
            resampling to 1024 / 512 straight into the model's inputs       (eager)
            tracker forward + best proposal for `slots` frames               (hipGraph replay)
            first-frame template crops of the targets added on this scan    (eager, one launch, only when there are any)
    host    one (slots, 5) + (slots, 2, 2) read-back, float64 box update of the continuing targets

Out of scope (INTEGRATION.md §3 "Live scans"): one hipGraph for the whole frame, SHAPE_AGGREGATION = all (an unbounded
per-target store), the REF_BOX modes (they need ground truth), sharding targets over GPUs, reading dataset files.
"""
import numpy as np
import torch

from . import ops
from .scene_store import check_raw
from .track_core import TrackCore, unit_boxes
from .tracklet_runner import tracking_modes

# ptt_crop_scan_f32 from this many points per scan on (scan_crop=None). Measured by scripts/online_tracker_timing.py
# (profiles/online_tracker_timing.json): the smallest measured N from which the chunked kernel is not slower at 2 jobs.
SCAN_CROP_MIN_POINTS = 32768


class SlotTable(object):
    """Which target holds which of `n` slots: host-only bookkeeping. A new id takes the lowest free slot; a dropped id frees its
    slot for reuse; ids are reported in the order they were added. plan() validates a step's drops and adds WITHOUT changing
    anything (ValueError: unknown id to drop, id already live, more adds than free slots); commit() applies what plan() returned."""

    def __init__(self, n):
        self.n = int(n)
        if self.n < 1:
            raise ValueError("slots must be >= 1, got %d" % self.n)
        self.slot_of = {}                                         # id -> slot, in insertion order

    @property
    def ids(self):
        return list(self.slot_of)

    def free(self):
        used = set(self.slot_of.values())
        return [s for s in range(self.n) if s not in used]

    def plan(self, add=(), drop=()):
        """-> (drop_ids, [(id, slot), ...] for the adds, in their order); raises ValueError and changes nothing."""
        drop, add = list(drop), list(add)
        if len(set(drop)) != len(drop) or len(set(add)) != len(add):
            raise ValueError("an id is listed twice in add / drop")
        for i in drop:
            if i not in self.slot_of:
                raise ValueError("drop: target %r holds no slot" % (i,))
        gone = set(drop)
        for i in add:
            if i in self.slot_of and i not in gone:
                raise ValueError("add: target %r is already live" % (i,))
        used = set(s for i, s in self.slot_of.items() if i not in gone)
        free = [s for s in range(self.n) if s not in used]
        if len(add) > len(free):
            raise ValueError("add: %d new targets, %d of %d slots free" % (len(add), len(free), self.n))
        return drop, list(zip(add, free))

    def commit(self, plan):
        drop, adds = plan
        for i in drop:
            del self.slot_of[i]
        for i, s in adds:
            self.slot_of[i] = s


def _as_box(box):
    parts = [np.asarray(v, np.float64).reshape(-1) for v in box]
    if [p.shape for p in parts] != [(3,), (3,), (4,)]:
        raise ValueError("a box is (center (3), wlh (3), quaternion (w, x, y, z))")
    return tuple(parts)


class OnlineTracker(object):
    def __init__(self, tracker, device, slots=8, scan_capacity=1 << 18, search_size=1024, template_size=512, search_offset=0.0,
                 search_scale=1.25, model_offset=0.0, model_scale=1.25, use_z=True, use_graph=True,
                 shape_aggregation="firstandprevious", scan_crop=None):
        """`tracker` and the sizes / offsets / scales as TrackletRunner's. slots: targets tracked at once (the model's batch
        width: every step runs the model at this width, empty slots as all-zero clouds). scan_capacity: the largest scan, in
        points (two resident buffers of that size, and crop slots that can hold a whole scan: no survivor is ever dropped).
        shape_aggregation: first / previous / firstandprevious (parsed by tracking_modes). scan_crop: True / False forces
        ptt_crop_scan_f32 / ptt_crop_compact_f32, None picks by SCAN_CROP_MIN_POINTS."""
        shape, _ = tracking_modes(shape_aggregation)
        if shape == "all":
            raise ValueError("SHAPE_AGGREGATION = all keeps an unbounded per-target store of every earlier crop: out of scope for "
                             "OnlineTracker (first, previous and firstandprevious are supported)")
        if int(scan_capacity) < 1:
            raise ValueError("scan_capacity must be >= 1")
        dev = self.device = torch.device(device)
        self.scan_capacity = int(scan_capacity)
        self.scan_crop = scan_crop
        # the step's buffers, tables, model graph and box update at width = slots; crop slots that hold a whole scan
        self.core = core = TrackCore(tracker, device, slots, search_size, template_size, search_offset, search_scale, model_offset,
                                     model_scale, use_z, use_graph, shape)
        S = self.S = core.W
        self.scans = torch.zeros((2, 3, self.scan_capacity), dtype=torch.float32, device=dev)
        core.reserve(self.scan_capacity)
        # the first-frame template crops of a step's new targets: a table of their own (at most `slots` jobs)
        self.add_jobs_dev = torch.zeros(S * ops.CROP_JOB.itemsize, dtype=torch.uint8, device=dev)
        self.add_jobs_host = torch.zeros(S * ops.CROP_JOB.itemsize, dtype=torch.uint8).pin_memory()
        self.add_jobs_np = self.add_jobs_host.numpy().view(ops.CROP_JOB)
        self.scan_ws = ops._ws(ops.crop_scan_workspace(2 * S, self.scan_capacity), dev)
        self.est_buf = np.zeros((S, 5), np.float32)
        # step_raw: the staging buffer of a host scan's interleaved rows (made at the first call) and its one-job ingest table
        self._raw_stage = None
        self._raw_job_host = torch.zeros(ops.SCAN_JOB.itemsize, dtype=torch.uint8).pin_memory()
        self._raw_job_np = self._raw_job_host.numpy().view(ops.SCAN_JOB)
        self.reset()

    # ------------------------------------------------------------------ state
    def reset(self):
        """Forget every target and both scans (the buffers and the captured model graph stay)."""
        S = self.S
        torch.cuda.synchronize(self.device)
        self.table = SlotTable(S)
        self.boxes = unit_boxes(S)                                # an empty slot: a unit box, never used
        self.extra = np.zeros(S)                                  # wlh[1] * 0.6 of the target's initial box (the search crop's margin)
        self.rng_pos = np.zeros(S, np.int64)                      # where numpy's global generator stands for each target
        self.cur = 0                                              # the scan buffer the NEXT step fills
        self.n_prev = 0                                           # points of the previous scan
        self.core.write_main_jobs()                               # the crop slots never move: every scan fits

    @property
    def targets(self):
        """ids currently holding a slot, in the order they were added."""
        return self.table.ids

    # ------------------------------------------------------------------ helpers
    def _check_scan(self, scan):
        """-> (tensor view of the scan, N); ValueError for anything but a (3, N) float32 C-contiguous numpy array or a (3, N)
        float32 torch tensor with N <= scan_capacity."""
        if isinstance(scan, np.ndarray):
            if scan.dtype != np.float32 or scan.ndim != 2 or scan.shape[0] != 3 or not scan.flags['C_CONTIGUOUS']:
                raise ValueError("scan must be a (3, N) float32 C-contiguous array, got %s %s" % (scan.dtype, scan.shape))
            t = torch.from_numpy(scan)
        elif isinstance(scan, torch.Tensor):
            if scan.dtype != torch.float32 or scan.dim() != 2 or scan.shape[0] != 3:
                raise ValueError("scan must be a (3, N) float32 tensor, got %s %s" % (scan.dtype, tuple(scan.shape)))
            if scan.is_cuda and scan.device != self.device:
                raise ValueError("scan lives on %s, the tracker on %s" % (scan.device, self.device))
            t = scan
        else:
            raise ValueError("scan must be a numpy array or a torch tensor, got %s" % type(scan).__name__)
        n = int(t.shape[1])
        if n > self.scan_capacity:
            raise ValueError("scan of %d points, scan_capacity=%d" % (n, self.scan_capacity))
        return t, n

    def _crop(self, max_points):
        """-> crop(jobs, jobs_dev, n_jobs), one launch over a device table (host copy: `jobs`): ptt_crop_scan_f32 for large scans."""
        def crop(jobs, jobs_dev, n_jobs):
            if bool(self.scan_crop) if self.scan_crop is not None else max_points >= SCAN_CROP_MIN_POINTS:
                ops.crop_scan_check(jobs, n_jobs, max_points)
                ops.crop_scan_device(jobs_dev, n_jobs, max_points, self.scan_ws)
            else:
                ops.crop_compact(jobs_dev, n_jobs)
        return crop

    # ------------------------------------------------------------------ public
    def step(self, scan, add=None, drop=()):
        """One time step. scan: (3, N) float32 — a C-contiguous numpy array or a torch tensor on the host (pinned: an
        asynchronous copy) or on the device; N <= scan_capacity, N = 0 allowed. drop: ids whose slots are freed BEFORE this scan
        is processed. add: {id: (center (3), wlh (3), quaternion (w, x, y, z))} — targets initialised on THIS scan (their frame
        0): their result for this step is the given box with score None, and their first-frame template crop is taken now.
        -> {id: (center, wlh, quat, score or None)} for every live target. ValueError (bad scan, N > scan_capacity, unknown id
        in drop, id already live, more adds than free slots) leaves the state unchanged. The scan may be reused by the caller
        as soon as the call returns."""
        t, n = self._check_scan(scan)
        return self._step(n, add, drop, lambda cur: self.scans[cur, :, :n].copy_(t, non_blocking=True))

    def step_raw(self, raw, steps=None, add=None, drop=()):
        """step() on the sensor's own buffer: raw is an (N, C) float32 scan of interleaved rows (x, y, z, then C - 3 columns that
        are dropped; 3 <= C <= 16, N <= scan_capacity) — a C-contiguous numpy array or a contiguous torch tensor on the host
        (pinned: an asynchronous copy) or on the device (read in place); steps: its way into the reference frame (ops.scan_steps'
        list: ('rotate', 3x3) / ('translate', 3) / ('affine', 3x4 or 4x4), at most four). A host scan is staged into a device
        buffer of scan_capacity * C floats (allocated at the first call, grown if C grows); one ptt_scan_ingest_f32 launch writes
        the planar scan straight into the resident buffer step() copies into, and the rest is step()'s own code: the same
        results as step() on the de-interleaved, transformed scan. A bad raw or bad steps raise ValueError and leave the state
        unchanged, as step()'s refusals do."""
        dev = self.device
        t = check_raw(raw, dev, self.scan_capacity)
        recs = ops.scan_steps(steps)
        n, C = int(t.shape[0]), int(t.shape[1])
        if not t.is_cuda and (self._raw_stage is None or self._raw_stage.numel() < self.scan_capacity * C):
            self._raw_stage = torch.empty(self.scan_capacity * C, dtype=torch.float32, device=dev)
        job = self._raw_job_np
        job[0] = np.zeros((), ops.SCAN_JOB)
        job['raw'] = t.data_ptr() if t.is_cuda else self._raw_stage.data_ptr()
        job['out'] = self.scans.data_ptr() + self.cur * 3 * self.scan_capacity * 4
        job['ld'], job['n_points'], job['row_floats'], job['n_steps'] = self.scan_capacity, n, C, len(recs)
        job['steps'][0, :len(recs)] = recs
        if n:
            ops.scan_ingest_check(job, 1, n)

        def place(cur):
            if n:
                if not t.is_cuda:
                    self._raw_stage[:n * C].copy_(t.reshape(-1), non_blocking=True)
                # the one-job table is read from pinned host memory; the step waits for the device before it returns
                ops.scan_ingest_device(self._raw_job_host, 1, n, dev)
        return self._step(n, add, drop, place)

    def _step(self, n, add, drop, place):
        """What step() and step_raw() share: everything but the form the scan arrives in. place(cur) enqueues, inside the device
        context, whatever writes the n points of this scan into self.scans[cur]; it runs once nothing can raise any more."""
        core, S, dev = self.core, self.S, self.device
        add = {} if add is None else dict(add)
        new_boxes = {i: _as_box(b) for i, b in add.items()}
        plan = self.table.plan(list(add), drop)
        # ---- nothing raised: the state changes from here on
        self.table.commit(plan)
        cur, prev = self.cur, 1 - self.cur
        self.cur = prev
        with torch.cuda.device(dev):
            place(cur)
        n_prev, self.n_prev = self.n_prev, n
        new_slots = set(s for _, s in plan[1])
        active = np.zeros(S, np.int32)
        for i, s in self.table.slot_of.items():
            active[s] = s not in new_slots
        boxes = self.boxes
        scores = None
        if active.any():
            core.ready(self.scan_capacity)        # the model graph: captured at the first tracked step, again after the weights changed
            # the 2 * slots crop table: job 2s = this scan around target s's previous result into slot 0 (the search crop, margin
            # wlh[1] * 0.6 of its initial box), job 2s + 1 = the previous scan around it into slot 2 (get_model's previous segment)
            jobs = core.jobs
            esz, ld = 4, self.scan_capacity
            live = active.astype(bool)
            jobs['ld'] = ld
            jobs['points'][0::2] = self.scans.data_ptr() + cur * 3 * ld * esz
            jobs['points'][1::2] = self.scans.data_ptr() + prev * 3 * ld * esz
            jobs['n_points'][0::2] = np.where(live, n, 0)
            jobs['n_points'][1::2] = np.where(live, 0 if core.shape == "first" else n_prev, 0)
            core.bounds(boxes, self.extra)
            with torch.cuda.device(dev):
                core.enqueue(2 * S, self._crop(max(n, n_prev)))
        if plan[1]:
            for i, s in plan[1]:
                boxes['center'][s], boxes['wlh'][s], boxes['quat'][s] = new_boxes[i]
                self.extra[s] = new_boxes[i][1][1] * 0.6
            if core.shape in ("firstandprevious", "first"):
                # frame 0 of the new targets: the first-frame template crop (get_model's first segment, slot 1), fixed for the
                # target's life. Only their jobs: an empty job would zero the count of a continuing target's slot 1
                k = len(plan[1])
                slots = np.array([s for _, s in plan[1]])
                aj = core.admission_jobs(slots, self.add_jobs_np)
                aj['points'], aj['ld'], aj['n_points'] = self.scans.data_ptr() + cur * 3 * self.scan_capacity * 4, self.scan_capacity, n
                ops.track_crop_bounds(np.ascontiguousarray(boxes[slots]), core.model_offset, core.model_scale, None, aj)
                with torch.cuda.device(dev):
                    self.add_jobs_dev.copy_(self.add_jobs_host, non_blocking=True)
                    self._crop(n)(self.add_jobs_np, self.add_jobs_dev, k)
        # the pinned staging tables and the caller's scan are free again once this step's device work is done
        with torch.cuda.device(dev):
            core.mark()
        core.wait()
        if active.any():
            # post_process as TrackletRunner._steps: box <- get_box_by_offset(box, best proposal); boxes of new and empty slots are
            # not touched (active = 0)
            core.update(boxes, active, self.rng_pos, self.est_buf)
            scores = self.est_buf[:, 4]
        for _, s in plan[1]:
            self.rng_pos[s] = 0                   # after the update: it records the draw count of every slot's resampling, empty ones too
        out = {}
        for i, s in self.table.slot_of.items():
            out[i] = (boxes['center'][s].copy(), boxes['wlh'][s].copy(), boxes['quat'][s].copy(), float(scores[s]) if active[s] else None)
        return out
