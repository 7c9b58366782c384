"""N4 — the reference's sequential tracking loop (TrackingEvaluator.test_batch / test_frame,
tools/eval_utils/eval_tracking_utils.py:77-152) with everything but a few float64 box updates on the device.

"Tracklet frames/sec" in the reference is this loop at B = 1: for frame i, crop the cloud around the PREVIOUS result
box and resample it to 1024 points (prepare_search :155-184), build the template from the first and the previous
frame's crops resampled to 512 (prepare_template :186-229), run the model (:231-264), take the best proposal and move
the box (post_process :266-274). Frame i needs frame i-1's box, so a tracklet is strictly sequential; different
tracklets are independent.

TrackletRunner keeps the clouds of up to `batch` tracklets resident in HBM and advances them in LOCKSTEP, one frame of
every tracklet per step:

    host    crop bounds of B boxes (float64, ptt_track_crop_bounds)       -> one job table in pinned memory, one upload
    device  ptt_crop_compact_f32   2B jobs: search crop, previous-frame template crop     (1 launch)
            ptt_regularize_f32     2B jobs: resample to 1024 / 512 straight into the model's input buffers (1 launch)
            the tracker forward for the B frames                                           (hipGraph replay)
            ptt_select_box_f32     best proposal of each frame                             (inside the graph)
    host    one (B,5) + (B,2,2) read-back, float64 box update of B boxes (ptt_track_box_by_offset)

That step's buffers, job tables, model graph and box update are a TrackCore (track_core.py), which PackedTrackletRunner and
OnlineTracker drive too; the runner adds the lockstep groups, the whole-frame graph of a handful of tracklets and the `all` store.

At batch = 1 this is the reference's own mode (one tracklet, one frame at a time) with the per-frame PCIe traffic cut
to ~0.5 KB; at batch = 48 it is the throughput mode for evaluating a dataset's tracklets.

The evaluator's two TEST settings (tools/cfgs/*/ptt.yaml:149-150) are arguments, parsed as the reference parses them
(tracking_modes):
    REF_BOX            previous_result (shipped) / previous_gt / current_gt: the box the search area is cropped around and
                       the box update starts from (prepare_search :155-162, post_process :270); a result taken from a
                       ground-truth box keeps that box's wlh.
    SHAPE_AGGREGATION  firstandprevious (shipped) / first / previous / all: which earlier frames' crops (always around the
                       RESULT boxes) make the template (prepare_template :186-216). first / previous resample one crop slot;
                       all keeps a per-tracklet store of the crops of frames 0..i-1 in HBM to which the template crop job
                       APPENDS cloud i-1 (ptt_crop_job.append): one crop per frame, the launches of firstandprevious.
The defaults are the shipped pair, with the launches and results they had before the settings existed.
"""
import numpy as np
import torch

from . import graph_policy, ops
from .track_core import TrackCore, unit_boxes


SHAPE_AGGREGATIONS = ("firstandprevious", "first", "previous", "all")
REF_BOXES = ("previous_result", "previous_gt", "current_gt")


def tracking_modes(shape_aggregation="firstandprevious", ref_box="previous_result"):
    """cfg.TEST.SHAPE_AGGREGATION, cfg.TEST.REF_BOX -> (one of SHAPE_AGGREGATIONS, one of REF_BOXES), read as the reference reads
    them: a case-insensitive substring test in the reference's order (prepare_template, eval_tracking_utils.py:187-216: anything
    without FIRST / PREVIOUS is `all`, and "first_and_previous" is `first`; prepare_search :156-162: anything else raises)."""
    agg, ref = str(shape_aggregation).upper(), str(ref_box).upper()
    if "FIRSTANDPREVIOUS" in agg:
        shape = "firstandprevious"
    elif "FIRST" in agg:
        shape = "first"
    elif "PREVIOUS" in agg:
        shape = "previous"
    else:
        shape = "all"
    for name in REF_BOXES:
        if name.upper() in ref:
            return shape, name
    raise ValueError("reference_BB must be set with previous_result/previous_gt/current_gt")


def upload_clouds(clouds, dev):
    """One tracklet's clouds ((3, N_i) float32 arrays / tensors) -> a list of device tensors whose rows are `stride(0)` apart and
    whose points are adjacent; tensors already on `dev` in that layout are used in place."""
    if all(isinstance(c, np.ndarray) for c in clouds) and len(clouds) > 0:
        # host arrays: ONE upload per tracklet — the frames side by side in a (3, sum N_i) buffer, every frame a
        # column range of it (the crop kernel takes the row stride) — instead of one small copy per frame
        sizes = [c.shape[1] for c in clouds]
        packed = torch.from_numpy(np.ascontiguousarray(np.concatenate([c[0:3] for c in clouds], axis=1), np.float32))
        packed = packed.to(dev)                  # pageable copy: pinning a fresh buffer per tracklet costs more than it saves
        offs = np.concatenate([[0], np.cumsum(sizes)])
        return [packed[:, offs[i]:offs[i + 1]] for i in range(len(clouds))]
    row = [(c if isinstance(c, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(c, np.float32)))
           .to(dev, torch.float32) for c in clouds]
    return [t if t.stride(1) == 1 else t.contiguous() for t in row]


class TrackletRunner(object):
    def __init__(self, tracker, device, batch=1, search_size=1024, template_size=512, search_offset=0.0,
                 search_scale=1.25, model_offset=0.0, model_scale=1.25, use_z=True, use_graph=True,
                 shape_aggregation="firstandprevious", ref_box="previous_result"):
        """`tracker`: ptt_amd.models.trackers.PTT in eval mode on `device`. Sizes / offsets / scales are
        DATA_CONFIG.{SEARCH,TEMPLATE}_INPUT_SIZE, SEARCH_BB_*, MODEL_BB_* and USE_Z_AXIS
        (tools/cfgs/kitti_models/ptt.yaml:8-17); shape_aggregation / ref_box are TEST.SHAPE_AGGREGATION / TEST.REF_BOX
        (:149-150), parsed by tracking_modes."""
        self.shape, self.ref_box = tracking_modes(shape_aggregation, ref_box)
        self.tracker, self.use_graph = tracker, use_graph
        dev, B = self.device, self.B = torch.device(device), int(batch)
        # a handful of tracklets: the crop table rides in the crop launch's arguments (no upload), and the host picks the best
        # proposal itself from the (B,P,5) read-back — two launches less per frame of a chain that is launches
        self.few = 2 * B <= ops.CROP_JOBS_BY_VALUE_MAX
        self.whole = bool(self.few and use_graph)    # ... and the whole frame is ONE hipGraph (_capture_frame): the core captures none
        info = None
        if self.whole:
            # one read-back buffer: (B,P,5) proposals, then the (B,2,2) resampling counts
            self.P = int(tracker.box_voting_head.model_cfg.SA_CONFIG.NPOINTS)
            self.n_box = B * self.P * 5
            self.readback = torch.zeros(self.n_box + B * 4, dtype=torch.float32, device=dev)
            self.readback_host = torch.zeros(self.n_box + B * 4, dtype=torch.float32).pin_memory()
            info = self.readback[self.n_box:].view(torch.int32).view(B, 2, 2)
        self.core = TrackCore(tracker, dev, B, search_size, template_size, search_offset, search_scale, model_offset, model_scale,
                              use_z, use_graph and not self.few, self.shape, few=self.few, info=info)
        self.S, self.T, self._model = self.core.S, self.core.T, self.core.model
        # few tracklets: crops + resampling + model + read-backs as one graph, and the tracker's state as of its capture (ops.StateWatch)
        self._frame = self._watch = None
        # SHAPE_AGGREGATION = all: per tracklet the canonical-frame crops of frames 0..i-1, (B, capacity, 3), and their running
        # totals (device scalars the append crop raises; the host learns them from the template's read-back info[0])
        self.store = self.store_count = None
        self.store_growths = 0                                       # how often a store was enlarged (over the runner's life)
        self.stream = None                                           # run_overlapped gives every runner its own stream
        self.profile = None       # set to {} before run(): per-frame host_pre / device / host_post milliseconds are appended

    draws = property(lambda self: self.core.draws, lambda self, table: setattr(self.core, "draws", table))     # the core's draw table

    # ------------------------------------------------------------------ device buffers of one group of tracklets
    def _load(self, tracklets):
        """tracklets: list (<= batch) of (clouds, boxes): clouds = list of (3,N_i) float32 arrays / tensors, boxes =
        list of (center (3), wlh (3), quat (4)) ground-truth boxes (frame 0 initialises; wlh[1] enters the search crop,
        eval_tracking_utils.py:165-169)."""
        dev, B, core = self.device, self.B, self.core
        T = max(len(c) for c, _ in tracklets)
        self.clouds = []
        # per frame i the cloud fields (address, row stride, points) of the interleaved 2B-job table: even jobs = frame i ...
        ff = [np.zeros((T, 2 * B), dt) for dt in (np.uint64, np.int64, np.int32)]
        cap = 1
        for b, (clouds, _) in enumerate(tracklets):
            row = upload_clouds(clouds, dev)
            for i, t in enumerate(row):
                ff[0][i, 2 * b], ff[1][i, 2 * b], ff[2][i, 2 * b] = t.data_ptr(), t.stride(0), t.shape[1]
                cap = max(cap, t.shape[1])
            self.clouds.append(row)
        core.ready(cap)
        ff[0][ff[2] == 0] = core.crop_out.data_ptr()               # empty jobs still carry a valid address
        for f in ff:
            f[1:, 1::2] = f[:-1, 0::2]                             # ... odd jobs = frame i - 1
        if self.shape == "first":
            ff[2][:, 1::2] = 0                                     # the template is frame 0's crop alone: no per-frame crop
        elif self.shape == "all":
            # a finished tracklet appends nothing (its frame `length` would otherwise add cloud length - 1 to its store)
            lengths = np.array([len(c) for c, _ in tracklets] + [0] * (B - len(tracklets)))
            ff[2][:, 1::2] *= (np.arange(T)[:, None] < lengths[None, :])
        self.frame_fields = ff
        if self.shape == "all":
            # every group starts with an empty store; a store that grew in an earlier group keeps its capacity
            if self.store is None or self.store.shape[1] < cap:
                self.store = torch.zeros((B, cap, 3), dtype=torch.float32, device=dev)
                self.store_count = torch.zeros(B, dtype=torch.int32, device=dev)
            self.store_count.zero_()
            self.store_total = np.zeros(B, np.int64)
            self._store_tables()

    def _store_tables(self):
        """SHAPE_AGGREGATION = all: point the template crop jobs (odd entries of the pinned crop table: append into the store) and
        the template resampling jobs (one segment: the whole store, its count the running total) at the current store, and upload
        the resampling table. A captured frame graph reads both tables when it replays (the crop table from pinned memory, the
        resampling table from device memory), so a store that moved needs this upload, not a new capture."""
        B, cap = self.B, self.store.shape[1]
        ptr = (self.store.data_ptr() + np.arange(B) * (cap * 3 * 4)).astype(np.uint64)
        cnt = (self.store_count.data_ptr() + np.arange(B) * 4).astype(np.uint64)
        t = self.core.reg_jobs[1::2]
        t['seg'][:, 0], t['seg_count'][:, 0], t['seg_capacity'][:, 0] = ptr, cnt, cap
        self.store_jobs = (ptr, cnt, cap)
        self.core.upload_resampling()

    def _reserve_store(self, i):
        """Before frame i appends cloud i - 1: every store must hold its total plus all of that cloud's points (a crop keeps
        at most those), so that no point is ever dropped. Otherwise the stores grow geometrically: a new buffer, a device copy
        of the used rows, new job pointers (_store_tables); the host waited for frame i - 1, so nothing reads the old buffer."""
        need = int((self.store_total + self.frame_fields[2][i, 1::2]).max())
        cap = self.store.shape[1]
        if need <= cap:
            return
        used = int(self.store_total.max())
        grown = torch.empty((self.B, max(need, 2 * cap), 3), dtype=torch.float32, device=self.device)
        grown[:, :used].copy_(self.store[:, :used])
        self.store = grown
        self.store_growths += 1
        self._store_tables()
        jobs = self.core.jobs[1::2]
        jobs['out'], jobs['capacity'] = self.store_jobs[0], self.store_jobs[2]

    def _first_frame_crop(self):
        """Frame 0: cloud 0 of every tracklet cropped around its ground-truth box 0 into slot 1 (get_model's first segment, fixed
        for the whole tracklet) — the even entries of the crop table; the odd ones are empty jobs (count 0) into slot 2."""
        core = self.core
        core.write_main_jobs()
        first = core.admission_jobs(np.arange(self.B), core.jobs[0::2])
        first['points'], first['ld'], first['n_points'] = (f[0, 0::2] for f in self.frame_fields)
        ops.track_crop_bounds(self.boxes, core.model_offset, core.model_scale, None, first, job_stride=2)
        core.jobs['points'][1::2] = core.crop_out.data_ptr()
        core.crop(2 * self.B)

    def _frame_jobs(self, i, extra2, ref=None):
        """The crop table of tracked frame i >= 1 written into the pinned staging buffer with three array assignments and the
        core's two bounds calls: job 2b = cloud i of tracklet b around its reference box into slot 0 (the search crop, `extra2` = gt_wlh1 * 0.6;
        `ref` = the REF_BOX boxes, None = the current results), job 2b + 1 = cloud i - 1 around its current result into slot 2
        (get_model's previous-frame segment) or appended to its store (all). The per-frame cloud fields were laid out for
        all frames by _load (self.frame_fields); `out` / `count` were set for these slots once (_steps)."""
        jobs = self.core.jobs
        pts, ld, npts = self.frame_fields
        jobs['points'], jobs['ld'], jobs['n_points'] = pts[i], ld[i], npts[i]
        self.core.bounds(self.boxes, extra2, ref)

    # ------------------------------------------------------------------ one group in lockstep
    def _steps(self, tracklets):
        """Generator form of one lockstep group: every `yield` sits between "frame i's device work is enqueued" and
        "the host waits for it", so that a driver can enqueue ANOTHER group's frame in between (run_overlapped). The
        generator's return value (StopIteration.value) is the group's result list."""
        B, core, n = self.B, self.core, len(tracklets)
        self._load(tracklets)
        lengths = np.array([len(c) for c, _ in tracklets] + [0] * (B - n))
        T = int(lengths.max())
        boxes = self.boxes = unit_boxes(B)
        gt_wlh1 = np.zeros((T, B))
        # REF_BOX previous_gt / current_gt: frame i's reference box (frames past a tracklet's end: a unit box, never used)
        gt = None if self.ref_box == "previous_result" else unit_boxes((T, B))
        for b, (_, gts) in enumerate(tracklets):
            boxes['center'][b], boxes['wlh'][b], boxes['quat'][b] = gts[0][0], gts[0][1], gts[0][2]
            for i, bx in enumerate(gts):
                gt_wlh1[i, b] = bx[1][1]
                if gt is not None:
                    gt['center'][i, b], gt['wlh'][i, b], gt['quat'][i, b] = bx[0], bx[1], bx[2]
        # per step: whole-batch copies (a result taken from a ground-truth reference box carries that box's wlh)
        history = [(np.ones(B, np.int32), boxes['center'].copy(), boxes['wlh'].copy(), boxes['quat'].copy(), None)]
        rng_pos = np.zeros(B, np.int64)            # where numpy's global generator stands for each tracklet
        # frame 0: the first-frame template crop is fixed for the whole tracklet. Only firstandprevious and first read slot 1:
        # previous resamples slot 2 alone, and all takes frame 0's crop from its store, to which frame 1 appends it — no launch
        # for those two
        if self.shape in ("firstandprevious", "first"):
            self._first_frame_crop()
        # the job table travels through ONE pinned staging buffer: its copy must have left the host before frame 1's
        # table is written into it (every later frame waits for its boxes anyway)
        core.mark()
        core.wait()
        core.write_main_jobs()                                    # every tracked frame crops into the same slots
        if self.shape == "all":                                  # ... or the template crop appends to the tracklet's store
            jobs = core.jobs
            jobs['out'][1::2], jobs['count'][1::2], jobs['capacity'][1::2] = self.store_jobs
            jobs['append'][1::2] = 1
        extra_search = np.ascontiguousarray(gt_wlh1 * 0.6)        # (T, B): gt_box.wlh[1] * 0.6 enters the search crop (:321)
        est_buf = np.zeros((B, 5), np.float32)
        active_all = (np.arange(T)[:, None] < lengths[None, :]).astype(np.int32)
        whole, read, info = self.whole, None, core.info_host.numpy()
        if whole:                                                # one read-back buffer: (B,P,5) proposals, then the resampling counts
            host = self.readback_host.numpy()
            info = host[self.n_box:].view(np.int32).reshape(B, 2, 2)
            read = (host[:self.n_box].reshape(B, self.P, 5), info)

        prof = self.profile
        if prof is not None:
            import time
            for k in ('host_pre_ms', 'device_ms', 'host_post_ms', 'frame_ms'):
                prof.setdefault(k, [])
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for i in range(1, T):
            if prof is not None:
                t_a = time.perf_counter()
                ev0.record(torch.cuda.current_stream(self.device))
            active = active_all[i]
            # the search crop of frame i is taken around the REF_BOX (prepare_search :156-162: by default the previous result),
            # the template crop around the previous RESULT (prepare_template :187-216 with results_BBs[frame_id - 1]); a finished
            # tracklet's later frames have n_points 0
            ref = None if gt is None else gt[i - 1] if self.ref_box == "previous_gt" else gt[i]
            if self.shape == "all":
                self._reserve_store(i)
            self._frame_jobs(i, extra_search[i], ref)
            if whole:
                # a handful of tracklets: the WHOLE frame is one hipGraph replay — crops (their table read from pinned host
                # memory, rewritten here), resampling, read-back of the draw counts, tracker, read-back of the proposals
                if self._frame is None:
                    self._capture_frame()
                self._frame.replay()
                core.mark()
            else:
                core.enqueue(2 * B)
            if prof is not None:
                ev1.record(torch.cuda.current_stream(self.device))
                t_b = time.perf_counter()
            yield i
            core.wait()
            if prof is not None:
                t_c = time.perf_counter()
            core.update(boxes, active, rng_pos, est_buf, ref, read)   # post_process (:266-274)
            if self.shape == "all":                              # the template's n is the store's new total (one segment)
                self.store_total[:] = info[:, 1, 0]
            history.append((active, boxes['center'].copy(), boxes['wlh'].copy(), boxes['quat'].copy(), est_buf[:, 4].copy()))
            if prof is not None:
                t_d = time.perf_counter()
                ev1.synchronize()
                prof['host_pre_ms'].append((t_b - t_a) * 1e3)        # crop bounds, job upload, enqueue of the frame's launches
                prof['device_ms'].append(ev0.elapsed_time(ev1))      # crop + resample + model graph + read-back, on the device
                prof['host_post_ms'].append((t_d - t_c) * 1e3)       # float64 box update, history
                prof['frame_ms'].append((t_d - t_a) * 1e3)
        # per-tracklet result lists, assembled once (four array copies per step instead of 4 x B small ones)
        results = []
        for b in range(n):
            rows = []
            for act, c, wlh, q, sc in history:
                if act[b]:
                    rows.append((c[b], wlh[b], q[b]) if sc is None else (c[b], wlh[b], q[b], float(sc[b])))
            results.append(rows)
        return results

    def _run_group(self, tracklets):
        gen = self._steps(tracklets)
        while True:
            try:
                next(gen)
            except StopIteration as stop:
                return stop.value

    def _frame_body(self):
        core = self.core
        ops.crop_regularize_pinned(core.jobs_host, core.reg_jobs_dev, 2 * self.B, core.draws)     # crop w, then resampling w
        rows = self._model(core.search, core.template)
        if rows.data_ptr() != self.readback.data_ptr():      # a box head that did not take the preallocated output: one copy
            self.readback[:self.n_box].view(self.B, self.P, 5).copy_(rows)
        return rows

    def _capture_frame(self):
        """One frame of a handful of tracklets as ONE hipGraph: called at the first tracked frame of the first group, when the
        job tables hold valid pointers (the warm-up runs execute them). The box head writes its proposals straight into the
        read-back buffer whose tail the resampling kernel fills with its draw counts (the core's `info` lives there): ONE
        device-to-host copy per frame."""
        head = self.tracker.box_voting_head
        with torch.no_grad():
            cur = torch.cuda.current_stream(self.device)
            side = torch.cuda.Stream(device=self.device)
            # SHAPE_AGGREGATION = all: each warm-up run appends frame i - 1's crop to the stores once more — their totals are
            # put back afterwards, so that the replay below appends it once (what the extra runs wrote past them is overwritten).
            # The copy is taken on `cur` BEFORE `side` waits for it: the warm-ups on `side` are then ordered after it
            totals = self.store_count.clone() if self.shape == "all" else None
            side.wait_stream(cur)
            head.pred_box_out = self.readback[:self.n_box].view(self.B, self.P, 5)
            try:
                with torch.cuda.stream(side):
                    for _ in range(3):                       # weight packing / LDS attributes happen here, not in capture
                        self._frame_body()
                cur.wait_stream(side)
                torch.cuda.synchronize(self.device)
                if totals is not None:
                    self.store_count.copy_(totals)
                self._frame = torch.cuda.CUDAGraph()
                with graph_policy.capture_scope(), torch.cuda.graph(self._frame):
                    self._frame_body()
                    self.readback_host.copy_(self.readback, non_blocking=True)
                self._watch = ops.StateWatch(self.tracker)
            finally:
                head.pred_box_out = None                     # the tracker may be shared: the hook is only live during capture

    def _drop_stale_graphs(self):
        """Once per run (the weights cannot change inside one): a frame graph captured before the tracker's weights or cached parameters
        changed would replay the old weights, or read freed buffers — it is dropped and captured again at the next frame (the core
        checks its model graph itself, TrackCore.ready)."""
        if self._watch is not None and self._watch.changed():
            self._frame = self._watch = None

    # ------------------------------------------------------------------ public
    def run(self, tracklets):
        """tracklets: list of (clouds, boxes) as in `_load`. Returns, per tracklet, the list of result boxes
        [(center, wlh, quat[, score]), ...] — element 0 is the frame-0 ground-truth box, as in the reference
        (eval_tracking_utils.py:96-100)."""
        self._drop_stale_graphs()
        out = []
        for g in range(0, len(tracklets), self.B):
            out.extend(self._run_group(tracklets[g:g + self.B]))
        return out


def run_overlapped(runners, tracklets):
    """Throughput form of the tracking loop: the tracklets are dealt to `len(runners)` TrackletRunners (each with its own
    buffers, model graph and HIP stream) whose lockstep groups advance ALTERNATELY — while the host waits for group A's
    boxes and computes its next crop bounds, group B's frame is on the device. Same per-tracklet results as
    runner.run(). Measured on one MI355X (round 3, scripts/probes/tracklet_groups_probe.py): 96 tracklets as 2 x 48 alternating
    10.7k frames/s against 9.8-10.3k one group after the other (144 / 192 tracklets as 3 / 4 groups: 10.7k / 10.5k) — the
    model graph of a 48-wide group fills the chip, so what overlaps is the host bubble (~0.5 ms per step) and the
    latency-bound sampling; splitting 48 tracklets into 2 x 24 loses more in half-filled graphs than it hides (round 2:
    7.8k against 8.4k). bench.py reports the single 48-wide group.
    tracklets: list of (clouds, boxes); returns the results in input order."""
    R = len(runners)
    dev = runners[0].device
    for r in runners:
        if r.stream is None:
            r.stream = torch.cuda.Stream(device=dev)
        r._drop_stale_graphs()
    # deal whole groups round-robin: runner k takes groups k, k+R, ...
    queues = [[] for _ in runners]
    pos = k = 0
    while pos < len(tracklets):
        b = runners[k % R].B
        queues[k % R].append((pos, tracklets[pos:pos + b]))
        pos += b
        k += 1
    results = [None] * len(tracklets)
    active = [None] * R                                             # (generator, start index) of the group in flight
    while any(queues) or any(a is not None for a in active):
        for r, runner in enumerate(runners):
            if active[r] is None and queues[r]:
                start, group = queues[r].pop(0)
                active[r] = (runner._steps(group), start)           # a generator: nothing of it has run yet
            if active[r] is not None:
                gen, start = active[r]
                with torch.cuda.stream(runner.stream):
                    try:
                        next(gen)                                   # wait for this group's frame (if any), enqueue its next one
                    except StopIteration as stop:                   # at once for single-frame tracklets: nothing to track
                        results[start:start + len(stop.value)] = stop.value
                        active[r] = None
    return results
