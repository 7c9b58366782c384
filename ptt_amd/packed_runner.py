"""PackedTrackletRunner — a dataset's tracklets through a fixed number of slots, every freed slot refilled at once.

TrackletRunner.run advances groups of `batch` tracklets in lockstep: a group costs max(length) - 1 steps at the full model width
however few of its tracklets are still alive, and tracking datasets have very uneven tracklet lengths. Here a tracklet takes a
slot for its frames 1 .. L-1 and the slot goes to the next waiting tracklet in the very next step:

    pr = PackedTrackletRunner(tracker, device, slots=48)
    results = pr.run(tracklets)             # TrackletRunner.run's input and return value, in input order
    pr.stats                                # steps, slot_steps, live_slot_steps, admissions, migrated — of that run

What a step computes is what TrackletRunner._steps computes, because both drive the same TrackCore (track_core.py): its buffers,
resampling table, model graph with the selection on the device and float64 box update, one step at a time at width = slots.
A frame's result depends on the width the model runs at, not on the slot or the batch-mates, so with drain_slots=None every
row is bit for bit TrackletRunner(batch=slots)'s. New here are only

    PackedPlan      the whole schedule, made on the host from the lengths alone (no device needed);
    admission jobs  the first-frame template crop (cloud 0 around ground-truth box 0 into crop slot 1) of the tracklets admitted
                    in a step rides behind that step's 2 * slots crop jobs, in the same launch (the core's table has `slots`
                    admission entries, TrackCore.admission_jobs): frame 1 is tracked in the step of the admission;
    the drain       drain_slots=k: once nothing waits and at most k tracklets are alive they move ONCE to a second core of
                    width k (first-frame crop and its count device to device; box, generator position and frame index on the
                    host) and the run ends there: the tail costs steps of width k. A frame's bits depend on the width, so a
                    migrated tracklet's rows FROM its migration frame on are not bitwise those of the wide run.

Clouds: a tracklet given as host arrays goes to the device in the step of its admission, side by side in one buffer as TrackletRunner
does (upload_clouds), and released when it finishes: at most `slots` tracklets are resident. Device tensors are used in place.

Out of scope: SHAPE_AGGREGATION = all (a per-slot growing store that is reset at a refill and moved at the drain is a change of
its own), sharding over GPUs, reading dataset files.
"""
import numpy as np
import torch

from . import ops
from .track_core import TrackCore, unit_boxes
from .tracklet_runner import tracking_modes, upload_clouds

ORDERS = ("longest_first", "input")


def _check_schedule(slots, order, drain_slots):
    if int(slots) < 1:
        raise ValueError("slots must be >= 1, got %d" % int(slots))
    if order not in ORDERS:
        raise ValueError("order must be one of %s, got %r" % (", ".join(ORDERS), order))
    if drain_slots is not None and not 1 <= int(drain_slots) <= int(slots):
        raise ValueError("drain_slots must lie in 1..slots=%d, got %d" % (int(slots), int(drain_slots)))


class PackedStep(object):
    """One step of a PackedPlan. width: the width of the core that runs it. admit: [(slot, tracklet)] taken from the queue in this
    step; track: [(slot, tracklet, frame)], the frames it tracks, by slot; migrate: None, or [(wide slot, drain slot, tracklet)] —
    the move to the drain core, made in this step before anything is launched. The slots of admit and track are those of the core
    that runs the step (the drain core's in the step of the migration)."""
    __slots__ = ("width", "admit", "track", "migrate")

    def __init__(self, width, admit, track, migrate):
        self.width, self.admit, self.track, self.migrate = width, admit, track, migrate


class PackedPlan(object):
    """The schedule of `lengths` (frames per tracklet, frame 0 included) through `slots` slots: host-only.

    A tracklet of length L holds a slot for its frames 1 .. L-1; lengths 0 and 1 never take one. Every step first gives the free
    slots (lowest first) to the waiting tracklets — order "input": in input order, "longest_first": longest first, ties by input
    index — and tracks frame 1 of an admitted tracklet in that same step; a slot whose tracklet ended is free in the next step. So
    no slot idles while a tracklet waits. drain_slots=k: in the first step in which, after the refill, nothing waits and at most k
    tracklets are alive, they move to slots 0 .. of a core of width k (in the order of their slots) and stay there.

    steps: [PackedStep]; n_steps, slot_steps (sum of the steps' widths), live_slot_steps (tracked frames), admissions,
    migration_step (index into steps, or None), migrated (tracklets moved)."""

    def __init__(self, lengths, slots, order="longest_first", drain_slots=None):
        _check_schedule(slots, order, drain_slots)
        lengths = [int(n) for n in lengths]
        if any(n < 0 for n in lengths):
            raise ValueError("a tracklet's length cannot be negative")
        self.lengths, self.slots, self.order = lengths, int(slots), order
        self.drain_slots = None if drain_slots is None else int(drain_slots)
        queue = [t for t, n in enumerate(lengths) if n >= 2]
        if order == "longest_first":
            queue.sort(key=lambda t: (-lengths[t], t))
        self.admission_order = list(queue)
        width = self.slots
        holder, frame = [-1] * width, [0] * width                   # per slot: its tracklet (-1: free), the frame it tracks next
        self.steps, self.migration_step, self.migrated = [], None, 0
        head = 0
        while head < len(queue) or any(t >= 0 for t in holder):
            admit = []
            for s in range(width):
                if holder[s] < 0 and head < len(queue):
                    holder[s], frame[s] = queue[head], 1
                    admit.append((s, queue[head]))
                    head += 1
            migrate = None
            alive = [s for s in range(width) if holder[s] >= 0]
            if self.drain_slots is not None and self.migration_step is None and head == len(queue) and len(alive) <= self.drain_slots:
                migrate = [(s, k, holder[s]) for k, s in enumerate(alive)]
                moved = dict((s, k) for s, k, _ in migrate)
                admit = [(moved[s], t) for s, t in admit]
                width = self.drain_slots
                holder, frame = ([holder[s] for s in alive] + [-1] * (width - len(alive)),
                                 [frame[s] for s in alive] + [0] * (width - len(alive)))
                self.migration_step, self.migrated = len(self.steps), len(migrate)
            track = [(s, holder[s], frame[s]) for s in range(width) if holder[s] >= 0]
            self.steps.append(PackedStep(width, admit, track, migrate))
            for s, t, i in track:
                frame[s] = i + 1
                if i + 1 >= lengths[t]:
                    holder[s] = -1
        self.n_steps = len(self.steps)
        self.slot_steps = sum(st.width for st in self.steps)
        self.live_slot_steps = sum(len(st.track) for st in self.steps)
        self.admissions = len(queue)


class _Lane(TrackCore):
    """A TrackCore of one width with the per-slot host state of a packed run: boxes, generator positions, chosen rows."""

    def start(self, cap):
        """Before a run: ready for clouds of `cap` points, the fixed fields of the crop table and fresh per-slot state."""
        self.ready(cap)
        self.write_main_jobs()
        self.boxes = unit_boxes(self.W)                           # an empty slot: a unit box, never used
        self.rng_pos = np.zeros(self.W, np.int64)                 # where numpy's global generator stands for each slot's tracklet
        self.est_buf = np.zeros((self.W, 5), np.float32)


class PackedTrackletRunner(object):
    def __init__(self, tracker, device, slots=48, order="longest_first", drain_slots=None, search_size=1024, template_size=512,
                 search_offset=0.0, search_scale=1.25, model_offset=0.0, model_scale=1.25, use_z=True, use_graph=True,
                 shape_aggregation="firstandprevious", ref_box="previous_result"):
        """`tracker`, the sizes / offsets / scales, shape_aggregation and ref_box as TrackletRunner's. slots: the width every step
        runs the model at (empty slots as all-zero clouds). order / drain_slots: see PackedPlan; drain_slots=k runs the tail on a
        second core of width k, whose frames are those of TrackletRunner(batch=k), not bitwise those of batch=slots."""
        _check_schedule(slots, order, drain_slots)
        self.shape, self.ref_box = tracking_modes(shape_aggregation, ref_box)
        if self.shape == "all":
            raise ValueError("SHAPE_AGGREGATION = all keeps a growing per-tracklet store of every earlier crop, which a refill would "
                             "have to reset and the drain to move: out of scope for PackedTrackletRunner (first, previous and "
                             "firstandprevious are supported)")
        self.device = torch.device(device)
        self.slots, self.order = int(slots), order
        self.drain_slots = None if drain_slots is None else int(drain_slots)
        args = (search_size, template_size, search_offset, search_scale, model_offset, model_scale, use_z, use_graph, self.shape)
        # every slot may be admitted in one step: as many admission entries as slots
        self.core = self.wide = _Lane(tracker, device, self.slots, *args, admissions=self.slots)
        self.drain = None if self.drain_slots is None else _Lane(tracker, device, self.drain_slots, *args, admissions=self.drain_slots)
        self.plan = None
        self.stats = dict(steps=0, slot_steps=0, live_slot_steps=0, admissions=0, migrated=0)

    # ------------------------------------------------------------------ host tables of one run
    def _frame_tables(self, tracklets):
        """Per frame of every tracklet, at index base[t] + i: the cloud's address, row stride and size (filled at the tracklet's
        upload), the search crop's margin gt_wlh[i][1] * 0.6 and the ground-truth box. -> the largest cloud, in points."""
        lengths = self.plan.lengths
        self.base = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        total = int(self.base[-1])
        self.ptr, self.ld, self.npts = np.zeros(total, np.uint64), np.zeros(total, np.int64), np.zeros(total, np.int32)
        gt = self.gt = np.zeros(total, ops.TRACK_BOX)
        wlh1 = np.zeros(total)
        cap = 1
        for t, (clouds, gts) in enumerate(tracklets):
            for i, bx in enumerate(gts):
                g = self.base[t] + i
                gt['center'][g], gt['wlh'][g], gt['quat'][g] = bx[0], bx[1], bx[2]
                wlh1[g] = bx[1][1]
                cap = max(cap, int(clouds[i].shape[1]))
        self.extra = np.ascontiguousarray(wlh1 * 0.6)
        return cap

    def _admit(self, lane, admit, tracklets):
        """Upload the admitted tracklets' clouds; their slots start from ground-truth box 0 with the generator at 0."""
        for s, t in admit:
            row = self.clouds[t] = upload_clouds(tracklets[t][0], self.device)
            g0 = self.base[t]
            for i, c in enumerate(row):
                self.ptr[g0 + i], self.ld[g0 + i], self.npts[g0 + i] = c.data_ptr(), c.stride(0), c.shape[1]
            lane.boxes[s] = self.gt[g0]
            lane.rng_pos[s] = 0

    def _migrate(self, moves, continuing):
        """wide -> drain: box and generator position on the host; the first-frame crop (crop slot 1, rows and count) of the
        tracklets that have one already, device to device. Every other buffer is rewritten by each step."""
        src, dst = self.wide, self.drain
        old, new = np.array([m[0] for m in moves]), np.array([m[1] for m in moves])
        dst.boxes[new], dst.rng_pos[new] = src.boxes[old], src.rng_pos[old]
        if continuing and self.shape in ("firstandprevious", "first"):
            cap = min(src.cap, dst.cap)                           # a crop holds at most the largest cloud of the run: <= both
            o = torch.as_tensor([m[0] for m in continuing], device=self.device)
            n = torch.as_tensor([m[1] for m in continuing], device=self.device)
            dst.crop_out[n, 1, :cap] = src.crop_out[o, 1, :cap]
            dst.counts[n, 1] = src.counts[o, 1]

    # ------------------------------------------------------------------ one step
    def _step(self, lane, st):
        core, W, dev = lane, lane.W, self.device
        tr = np.array(st.track, np.int64).reshape(-1, 3)
        slots, g = tr[:, 0], self.base[tr[:, 1]] + tr[:, 2]       # the live slots and their frames' rows in the frame tables
        main = core.jobs[:2 * W]
        # job 2s = cloud i of slot s's tracklet around its reference box into slot 0 (the search crop), job 2s + 1 = cloud i - 1
        # around its current result into slot 2 (get_model's previous segment); n_points = 0 for empty slots
        pts, ld, npts = np.full(2 * W, core.crop_out.data_ptr(), np.uint64), np.zeros(2 * W, np.int64), np.zeros(2 * W, np.int32)
        pts[2 * slots], ld[2 * slots], npts[2 * slots] = self.ptr[g], self.ld[g], self.npts[g]
        pts[2 * slots + 1], ld[2 * slots + 1] = self.ptr[g - 1], self.ld[g - 1]
        if self.shape != "first":                                 # first: the template is frame 0's crop alone
            npts[2 * slots + 1] = self.npts[g - 1]
        main['points'], main['ld'], main['n_points'] = pts, ld, npts
        boxes = lane.boxes
        extra = np.zeros(W)
        extra[slots] = self.extra[g]
        ref = None
        if self.ref_box != "previous_result":                     # REF_BOX previous_gt / current_gt: the tracklet's own ground truth
            ref = unit_boxes(W)
            ref[slots] = self.gt[g - 1 if self.ref_box == "previous_gt" else g]
        core.bounds(boxes, extra, ref)
        n_jobs = 2 * W
        if st.admit and self.shape in ("firstandprevious", "first"):
            # frame 0 of the admitted tracklets: cloud 0 around ground-truth box 0 into slot 1 (get_model's first segment), fixed
            # for the tracklet's life. Their boxes still ARE box 0
            new = np.array([s for s, _ in st.admit])
            g0 = self.base[np.array([t for _, t in st.admit])]
            aj = core.admission_jobs(new)
            aj['points'], aj['ld'], aj['n_points'] = self.ptr[g0], self.ld[g0], self.npts[g0]
            ops.track_crop_bounds(np.ascontiguousarray(boxes[new]), core.model_offset, core.model_scale, None, aj)
            n_jobs += len(new)
        with torch.cuda.device(dev):
            core.enqueue(n_jobs)
        core.wait()
        # post_process as TrackletRunner._steps: a REF_BOX from the ground truth is the box that moves (and keeps its wlh)
        active = np.zeros(W, np.int32)
        active[slots] = 1
        core.update(boxes, active, lane.rng_pos, lane.est_buf, ref)
        res = self.rows
        res['center'][g], res['wlh'][g], res['quat'][g] = boxes['center'][slots], boxes['wlh'][slots], boxes['quat'][slots]
        self.scores[g] = lane.est_buf[slots, 4]

    # ------------------------------------------------------------------ public
    def run(self, tracklets):
        """tracklets: list of (clouds, boxes) as TrackletRunner.run takes them. Returns, per tracklet and in input order, the list
        of result boxes [(center, wlh, quat[, score]), ...] — element 0 is the frame-0 ground-truth box; a tracklet without frames
        gives an empty list. ValueError (a tracklet whose cloud and box counts differ) before anything changes."""
        tracklets = list(tracklets)
        for t, (clouds, gts) in enumerate(tracklets):
            if len(clouds) != len(gts):
                raise ValueError("tracklet %d has %d clouds and %d boxes" % (t, len(clouds), len(gts)))
        plan = self.plan = PackedPlan([len(c) for c, _ in tracklets], self.slots, self.order, self.drain_slots)
        cap = self._frame_tables(tracklets)
        self.rows, self.scores = self.gt.copy(), np.zeros(len(self.gt), np.float32)     # row 0 of a tracklet: its box 0
        self.clouds = [None] * len(tracklets)
        lane = self.wide
        if plan.n_steps:
            with torch.cuda.device(self.device):
                lane.start(cap)
                if plan.migration_step is not None:
                    self.drain.start(cap)
        for st in plan.steps:
            if st.migrate is None:
                self._admit(lane, st.admit, tracklets)
            else:
                lane = self.drain
                new = set(t for _, t in st.admit)
                self._migrate(st.migrate, [m for m in st.migrate if m[2] not in new])
                self._admit(lane, st.admit, tracklets)
            self._step(lane, st)
            for _, t, i in st.track:
                if i + 1 == plan.lengths[t]:
                    self.clouds[t] = None                         # the host has waited for the step: nothing reads them any more
        self.stats = dict(steps=plan.n_steps, slot_steps=plan.slot_steps, live_slot_steps=plan.live_slot_steps,
                          admissions=plan.admissions, migrated=plan.migrated)
        out = []
        rows, scores = self.rows, self.scores
        for t, n in enumerate(plan.lengths):
            g0 = int(self.base[t])
            out.append([(rows['center'][g].copy(), rows['wlh'][g].copy(), rows['quat'][g].copy()) if g == g0 else
                        (rows['center'][g].copy(), rows['wlh'][g].copy(), rows['quat'][g].copy(), float(scores[g]))
                        for g in range(g0, g0 + n)])
        return out
