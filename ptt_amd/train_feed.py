"""N5 — training batches made on the device: the reference's KittiTrackingDataset.get_train_items
(ptt/datasets/kitti/kitti_dataset_tracking.py:44-179; nuscenes/nus_dataset_tracking.py:153-288 is the same code) for a whole
batch in two launches, from tracklets that stay resident in HBM.

    feeder = TrainBatchFeeder(tracklets, device, batch_size=48)
    for epoch in range(n_epochs):
        feeder.set_epoch(epoch)
        for batch in feeder:                     # search_points, template_points, cls_label, reg_label, batch_size
            trainer.step(batch)

What the reference does per sample on the host — pick (tracklet, frame, augmentation) from the dataset index, draw the offsets,
crop the search area with its labels, crop the template from the first and the previous frame, reject crops of <= 20 points,
resample to the fixed sizes — happens here as

    host    the index plan, the offsets and O(B) float64 box arithmetic                 -> one pinned table, one upload
    device  ptt_crop_compact_f32   3 jobs per candidate: search crop + labels, first-frame crop, previous-frame crop
            ptt_train_batch_f32    validity, replacement of rejected samples, resampling, labels — straight into the batch

and no point count ever travels to the host. Two departures from the reference, both because it draws from numpy's global
generator (per worker process, order-dependent):
  * the offsets of dataset index j in epoch e come from np.random.RandomState([seed, e, j]), drawn in the reference's call order
    (the search normal, its redraws inside get_box_by_offset x before y, the template uniform, its redraws): a sample depends on
    (seed, e, j) alone, not on batch composition, shuffling or the number of ranks;
  * the resampling indices are Philox4x32-10 outputs addressed by (draw, j, search / template, e) under the key `seed`
    (include/ptt_hip.h, N5), so the device holds no generator state.
A rejected sample is replaced as the reference replaces it, by a uniformly random dataset index — drawn ahead of time: every
batch carries `spare` extra candidates (np.random.RandomState([seed, e, batch number]).randint(0, len, spare)), and the kernel
hands the r-th rejected primary the r-th valid spare.

DATA_AUGMENTOR (`augmentor=`, what ptt.datasets.augmentor.DataAugmentor takes): the queue of random_world_flip / _rotation /
_scaling of a sample is one map [x'; y'] = M [x; y], z' = kz z. The host draws it per candidate from a generator of its own,
RandomState([seed, e, j, 0x415547]) — so turning the augmentor on moves no offset, index or crop — forms M, kz and the augmented
reg_label in float64, and ships five float32 per candidate in a ptt_train_aug table behind the candidates (the same upload);
ptt_train_batch_aug_f32 applies the map to the rows it has just gathered, right before it stores them.
"""
import warnings

import numpy as np
import torch

from . import ops
from .datasets.augmentor import DataAugmentor, augmentor_utils
from .datasets.kitti import box_math as bm
from .track_core import slot_pointers
from .tracklet_shard import dist_info, shard_indices

_MVN = None
AUG_STREAM = 0x415547         # 'AUG': the last seed word of a candidate's augmentation generator


def _search_normal(rs):
    """KalmanFiltering(bnd=[1, 1, 5]).sample(1)[0] = RandomState.multivariate_normal(zeros(3), diag(1, 1, 5), size=1)[0]
    (kitti_tracking_utils.py:167-184) from the generator `rs`, as numpy forms it — standard_normal((1, 3)) times
    sqrt(s)[:, None] * v of the covariance's SVD — with that factor computed once."""
    global _MVN
    if _MVN is None:
        _, s, v = np.linalg.svd(np.array(np.diag([1, 1, 5]), np.float64))
        _MVN = np.sqrt(s)[:, None] * v
    x = np.dot(rs.standard_normal((1, 3)).reshape(-1, 3), _MVN)
    x += np.zeros(3)
    return x[0]


def _host_seed(seed, *rest):
    """The RandomState seed sequence [seed, ...]: numpy takes 32-bit words, a seed beyond them appends its high word."""
    seed = int(seed)
    return [seed & 0xffffffff] + [int(r) for r in rest] + ([seed >> 32] if seed >> 32 else [])


class _Queue(object):
    """Pre-drawn np.random.uniform(-1, 1) replacements, handed to box_math.get_box_by_offset in its calling order."""

    def __init__(self):
        self.values = []

    def __call__(self):
        return self.values.pop(0)


class _OutputSet(object):
    """One of the `depth` sets of tensors a batch is produced into."""

    def __init__(self, f, dev):
        B, S, T = f.B, f.S, f.T
        z = lambda shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=dev)
        self.search, self.template, self.cls, self.reg = z((B, S, 3)), z((B, T, 3)), z((B, S)), z((B, 4))
        self.src, self.idx_search, self.idx_template = z((B,), torch.int32), z((B, S), torch.int32), z((B, T), torch.int32)
        self.info = z((4,), torch.int32)
        d = self.desc = np.zeros(1, ops.TRAIN_BATCH_DESC)
        d['search_points'], d['template_points'], d['cls_label'], d['reg_label'] = (t.data_ptr() for t in (self.search, self.template, self.cls, self.reg))
        d['src_out'], d['idx_search_out'], d['idx_template_out'] = self.src.data_ptr(), self.idx_search.data_ptr(), self.idx_template.data_ptr()
        d['info'], d['totals'] = self.info.data_ptr(), f.totals.data_ptr()
        d['B'], d['n_cand'], d['search_size'], d['template_size'], d['min_points'] = B, f.C, S, T, f.min_points
        d['seed_lo'], d['seed_hi'] = f.seed & 0xffffffff, f.seed >> 32
        self.done = torch.cuda.Event()
        self.batch = {'search_points': self.search, 'template_points': self.template, 'cls_label': self.cls, 'reg_label': self.reg,
                      'batch_size': B}


def dataset_length(n_frames, candidates_per_frame, sampled_interval):
    """KittiTrackingDataset.__len__ in training (:44-47)."""
    return int(n_frames) * int(candidates_per_frame) // int(sampled_interval)


def locate(index, candidates_per_frame, sampled_interval):
    """Dataset indices -> (annotation index, augmentation index): __getitem__'s `index *= sample_interval` (:51), then
    get_anno_index / get_aug_index (:221-225); the annotation index addresses frame_seq_map (:211-219)."""
    full = np.asarray(index, np.int64) * int(sampled_interval)
    return full // int(candidates_per_frame), full % int(candidates_per_frame)


class TrainBatchPlan(object):
    """The host half of TrainBatchFeeder, usable without a device: the index plan of the reference's training dataset over
    `tracklets`, the epoch's order and this rank's share of it, and plan(epoch, batch) — the dataset indices, offsets, moved
    boxes' crop quantities and reg_label of a batch. Arguments as TrainBatchFeeder's (which adds the device side)."""

    def __init__(self, tracklets, batch_size=48, search_size=1024, template_size=512, search_offset=0.0, search_scale=1.25,
                 model_offset=0.0, model_scale=1.25, use_z=True, refine_box=True, candidates_per_frame=4, sampled_interval=1,
                 min_points=20, spare=None, seed=0, shuffle=True, drop_last=True, rank=None, world=None, augmentor=None):
        self.B, self.S, self.T = int(batch_size), int(search_size), int(template_size)
        self.spare = max(4, self.B // 8) if spare is None else int(spare)
        self.C = self.B + self.spare
        if self.B < 1 or self.spare < 0 or self.C > ops.TRAIN_MAX_CANDS:
            raise ValueError("batch_size + spare must be 1..%d candidates, got %d + %d" % (ops.TRAIN_MAX_CANDS, self.B, self.spare))
        self.search_offset, self.search_scale = float(search_offset), float(search_scale)
        self.model_offset, self.model_scale = float(model_offset), float(model_scale)
        self.use_z, self.refine_box = bool(use_z), bool(refine_box)
        self.cpf, self.interval = int(candidates_per_frame), int(sampled_interval)
        if self.cpf < 1 or self.interval < 1:
            raise ValueError("candidates_per_frame and sampled_interval must be positive")
        self.min_points = int(min_points)
        self.seed = int(seed)
        if not 0 <= self.seed < 1 << 64:
            raise ValueError("seed must be a non-negative integer below 2^64")
        self.shuffle, self.drop_last = bool(shuffle), bool(drop_last)
        if rank is None or world is None:
            rank, world = dist_info()
        self.rank, self.world = int(rank), int(world)
        self.epoch = 0
        self._orders = {}
        self._augment(augmentor)
        self._tables(tracklets)
        self.length = dataset_length(self.n_frames, self.cpf, self.interval)
        if self.length < 1:
            raise ValueError("no training sample: %d frames, %d candidates per frame, interval %d" % (self.n_frames, self.cpf, self.interval))
        n_local = len(shard_indices(self.length, self.rank, self.world))
        self.n_batches = n_local // self.B if self.drop_last else -(-n_local // self.B)

    @staticmethod
    def config_args(data_cfg):
        """The constructor arguments a DATA_CONFIG section (tools/cfgs/*/ptt.yaml:6-24; a mapping) sets: sizes, offsets, scales,
        USE_Z_AXIS, REFINE_BOX_SIZE (True where the key is absent, as in p2b.yaml), NUM_CANDIDATES_PERFRAME, SAMPLED_INTERVAL."""
        get = lambda key, default: data_cfg[key] if key in data_cfg else default
        return dict(search_size=get('SEARCH_INPUT_SIZE', 1024), template_size=get('TEMPLATE_INPUT_SIZE', 512),
                    search_offset=get('SEARCH_BB_OFFSET', 0.0), search_scale=get('SEARCH_BB_SCALE', 1.25),
                    model_offset=get('MODEL_BB_OFFSET', 0.0), model_scale=get('MODEL_BB_SCALE', 1.25), use_z=get('USE_Z_AXIS', True),
                    refine_box=get('REFINE_BOX_SIZE', True), candidates_per_frame=get('NUM_CANDIDATES_PERFRAME', 4),
                    sampled_interval=get('SAMPLED_INTERVAL', 1), augmentor=get('DATA_AUGMENTOR', None))

    @classmethod
    def from_config(cls, tracklets, data_cfg, batch_size, **kw):
        return cls(tracklets, batch_size=batch_size, **dict(cls.config_args(data_cfg), **kw))

    def _tables(self, tracklets):
        """The per-frame tables the index plan addresses: frame_seq_map (:38, :211-219), the frames' sizes and ground-truth boxes,
        the first and the previous frame of every frame. Tracklets without frames are skipped, as an empty annotation list is."""
        npts, trk, frm, first, prev, boxes = [], [], [], [], [], []
        for t, (clouds, gts) in enumerate(tracklets):
            if len(clouds) != len(gts):
                raise ValueError("tracklet %d: %d clouds, %d boxes" % (t, len(clouds), len(gts)))
            base = len(trk)
            for i, c in enumerate(clouds):
                npts.append(int(c.shape[1]))
                trk.append(t)
                frm.append(i)
                first.append(base)
                prev.append(base + max(i - 1, 0))
                boxes.append(gts[i])
        self.n_frames = len(trk)
        self.npts = np.array(npts, np.int32)
        self.tracklet_of, self.frame_of = np.array(trk, np.int64), np.array(frm, np.int64)
        self.first_of, self.prev_of = np.array(first, np.int64), np.array(prev, np.int64)
        self.center = np.array([b[0] for b in boxes], np.float64).reshape(-1, 3)
        self.wlh = np.array([b[1] for b in boxes], np.float64).reshape(-1, 3)
        self.quat = np.array([b[2] for b in boxes], np.float64).reshape(-1, 4)
        self.cap = int(max(1, self.npts.max() if self.n_frames else 1))

    # ------------------------------------------------------------------ the plan of a batch (host only)
    def __len__(self):
        return self.n_batches

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def _order(self, epoch):
        """This rank's dataset indices of an epoch, in order."""
        if epoch not in self._orders:
            perm = np.random.RandomState(_host_seed(self.seed, epoch)).permutation(self.length) if self.shuffle else np.arange(self.length)
            if len(self._orders) > 1:
                self._orders.clear()
            self._orders[epoch] = perm[np.array(shard_indices(self.length, self.rank, self.world), np.int64)]
        return self._orders[epoch]

    def plan(self, epoch, batch):
        """The host-side description of batch `batch` of epoch `epoch`: dict of
             index (C,)  the dataset indices, B primaries then the spares;   anno, aug, tracklet, frame (C,)  what they address;
             search_offset, template_offset (C,3)  the offsets as used (after get_box_by_offset's redraws);   reg_label (C,4) float64
        plus, for the launch, the frames and the boxes' crop quantities (`_frames`, `_jobs`). With an augmentor also aug_map (C,5)
        float32, aug_draws (C, len(aug_kinds)), aug_kinds and reg_label_raw; reg_label is then the augmented one (_augmentation)."""
        epoch, batch = int(epoch), int(batch)
        if not 0 <= batch < self.n_batches:
            raise IndexError("batch %d of %d" % (batch, self.n_batches))
        B, C = self.B, self.C
        order = self._order(epoch)
        prim = order[(batch * B + np.arange(B)) % len(order)]
        number = batch * self.world + self.rank                # the batch's number over all ranks
        spares = np.random.RandomState(_host_seed(self.seed, epoch, number)).randint(0, self.length, self.spare)
        index = np.concatenate([prim, spares]).astype(np.int64)
        anno, aug = locate(index, self.cpf, self.interval)
        first, prev = self.first_of[anno], self.prev_of[anno]
        # the offsets (x, y, z; z doubles as theta in degrees, :127) in the reference's call order, per candidate
        off_s, off_t = np.zeros((C, 3)), np.zeros((C, 3))
        redraw_s, redraw_t = _Queue(), _Queue()
        rs = np.random.RandomState(0)
        for c in np.nonzero(aug)[0]:
            rs.seed(_host_seed(self.seed, epoch, index[c]))
            off_s[c] = _search_normal(rs)                                              # :124-125
            w = self.wlh[anno[c]]
            if off_s[c, 0] > w[0]:                                                     # get_box_by_offset :208-211
                redraw_s.values.append(rs.uniform(-1, 1))
            if off_s[c, 1] > min(w[1], 2):
                redraw_s.values.append(rs.uniform(-1, 1))
            off_t[c] = rs.uniform(low=-0.3, high=0.3, size=3)                          # :155-156
            off_t[c, 2] = off_t[c, 2] * 5.0
            w = self.wlh[prev[c]]
            if off_t[c, 0] > w[0]:
                redraw_t.values.append(rs.uniform(-1, 1))
            if off_t[c, 1] > min(w[1], 2):
                redraw_t.values.append(rs.uniform(-1, 1))
        gc, gw, gq = self.center[anno], self.wlh[anno], self.quat[anno]
        sc, sq, off_s = bm.get_box_by_offset(gc, gw, gq, off_s, self.use_z, uniform=redraw_s)           # :128
        pc, pq, off_t = bm.get_box_by_offset(self.center[prev], self.wlh[prev], self.quat[prev], off_t, self.use_z, uniform=redraw_t)   # :160
        # the float64 crop quantities of the four boxes of every candidate (ptt_track_crop_bounds: microseconds): column 0 the
        # search crop (:129-138, :320), 1 / 2 the template's first / previous frame, 3 the ground-truth box the labels are taken against
        jobs = np.zeros((C, 4), ops.CROP_JOB)
        refine = self.refine_box
        for k, (c_, w_, q_, off, scale, extra) in enumerate((
                (sc, gw, sq, self.search_offset, self.search_scale, gw[:, 1] * 0.6),
                (self.center[first], self.wlh[first], self.quat[first], self.model_offset, self.model_scale, None),
                (pc, self.wlh[prev], pq, self.model_offset, self.model_scale, None),
                (gc, gw, gq, self.search_offset if refine else 0.0, self.search_scale if refine else 1.0, None))):
            boxes = np.zeros(C, ops.TRACK_BOX)
            boxes['center'], boxes['wlh'], boxes['quat'] = c_, w_, q_
            ops.track_crop_bounds(boxes, off, scale, extra, jobs[:, k], job_stride=4)
        # reg_label (:321-325): the ground-truth centre carried through the sample box's translate / rotate, and -theta
        R2 = bm.q_rotation_matrix(bm.q_from_matrix(jobs['rot'][:, 0].reshape(C, 3, 3)))
        reg = np.concatenate([np.einsum('...ij,...j->...i', R2, gc + jobs['trans'][:, 0]), -off_s[:, 2:3]], 1)
        out = {'index': index, 'anno': anno, 'aug': aug, 'tracklet': self.tracklet_of[anno], 'frame': self.frame_of[anno],
               'search_offset': off_s, 'template_offset': off_t, 'reg_label': reg,
               '_frames': (anno, first, prev), '_jobs': jobs}
        if self.aug_steps is not None:
            out['reg_label_raw'], out['aug_kinds'] = reg, self.aug_kinds
            out['aug_map'], out['reg_label'], out['aug_draws'] = self._augmentation(epoch, index, reg)
        return out

    def _augment(self, augmentor):
        """The DATA_AUGMENTOR queue as the flat list of its draws, `aug_steps` = [(kind, range)] with kind flip_x / flip_y /
        rotation / scaling (`aug_kinds`: the kinds alone, the columns of plan()['aug_draws']); None without an augmentor. A
        scaling whose range is a no-op draws nothing and is left out. Unknown NAMEs and axes raise here (DataAugmentor's checks)."""
        self.aug_steps, self.aug_kinds = None, ()
        if augmentor is None:
            return
        if not isinstance(augmentor, DataAugmentor):
            augmentor = DataAugmentor(None, augmentor, None)
        steps = []
        for name, arg in augmentor.steps:
            if name == 'random_world_flip':
                steps += [('flip_' + axis, None) for axis in arg]
            elif name == 'random_world_rotation':
                steps.append(('rotation', arg))
            elif not augmentor_utils.scaling_is_noop(arg):
                steps.append(('scaling', arg))
        self.aug_steps, self.aug_kinds = steps, tuple(kind for kind, _ in steps)

    def _augmentation(self, epoch, index, reg):
        """DataAugmentor.forward of every candidate as ONE map: whatever the queue, the points go through [x'; y'] = M [x; y],
        z' = kz z. -> (aug_map (C,5) float32 = m00, m01, m10, m11, kz; the augmented reg_label (C,4) float64; the draws (C, len(
        aug_kinds)) float64, flags as 0 / 1). The draws of dataset index j come from RandomState([seed, epoch, j, AUG_STREAM]) in
        queue order, through augmentor_utils' own calls; M, kz and the label's centre are formed in float64, with the cos / sin
        of the angle as float32 holds it (the angle the reference's rotation uses); theta follows the operations one by one."""
        C, steps = len(index), self.aug_steps
        amap, out, draws = np.zeros((C, 5)), np.array(reg, np.float64), np.zeros((C, len(steps)))
        rs = np.random.RandomState(0)
        for c in range(C):
            rs.seed(_host_seed(self.seed, epoch, index[c]) + [AUG_STREAM])
            M, kz, theta = np.eye(2), 1.0, reg[c, 3]
            for k, (kind, span) in enumerate(steps):
                if kind == 'flip_x':                                   # negates y
                    d = augmentor_utils.draw_flag(rs)
                    if d:
                        M[1], theta = -M[1], -theta
                elif kind == 'flip_y':                                 # negates x
                    d = augmentor_utils.draw_flag(rs)
                    if d:
                        M[0], theta = -M[0], -(theta + np.pi)
                elif kind == 'rotation':
                    d = augmentor_utils.draw_uniform(rs, span)
                    a = np.float64(np.float32(d))
                    M = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]).dot(M)
                    theta = theta + d
                else:
                    d = augmentor_utils.draw_uniform(rs, span)
                    M, kz = M * d, kz * d
                draws[c, k] = d
            amap[c, 0:4], amap[c, 4] = M.reshape(4), kz
            out[c, 0:2], out[c, 2], out[c, 3] = M.dot(reg[c, 0:2]), kz * reg[c, 2], theta
        return (amap + 0.0).astype(np.float32), out, draws



class TrainBatchFeeder(TrainBatchPlan):
    """Training batches of `batch_size` samples out of resident tracklets; see the module text for what a sample is.

    tracklets: list of (clouds, boxes) as TrackletRunner takes them — clouds = list of (3, N_i) float32 arrays, boxes = list of
    (center (3), wlh (3), quaternion (w, x, y, z)) ground-truth boxes — uploaded once, one packed buffer per tracklet. The other
    arguments are DATA_CONFIG's (from_config reads them): {SEARCH,TEMPLATE}_INPUT_SIZE, SEARCH_BB_*, MODEL_BB_*, USE_Z_AXIS,
    REFINE_BOX_SIZE, NUM_CANDIDATES_PERFRAME, SAMPLED_INTERVAL. min_points: a search crop or a template of that many points or
    fewer rejects the sample (the reference's 20). spare: replacement candidates per batch, default max(4, batch_size // 8).
    seed: a non-negative integer below 2^64. shuffle: the epoch's order is RandomState([seed, epoch]).permutation(len), else the
    identity; it is dealt to the ranks as tracklet_shard.shard_indices deals tracklets (rank / world default to the process
    group). drop_last=False fills the last batch by wrapping to the rank's first indices. augmentor: a DATA_AUGMENTOR section (a
    list of entries, a mapping with AUG_CONFIG_LIST, or a DataAugmentor), applied to search_points, template_points and reg_label
    of every sample (module text); from_config reads the key when the config has it.

    len(feeder) = batches per epoch for this rank; set_epoch(e) selects the epoch; iterating yields dicts with the keys, shapes
    and dtypes of train_step.synthetic_train_batch. plan(epoch, batch) describes a batch on the host alone. stats() reads the
    counters the kernel keeps (batches, rejected primaries, shortfalls) and is the only call that waits for the device.

    Buffer lifetime and ordering. Batches are produced into `depth` sets of tensors in rotation: the tensors of a yielded batch
    stay valid until `depth` further batches have been requested, and are then overwritten — clone what must live longer.
    Production runs on `stream`, fixed at construction (default: the stream current then) for the feeder's whole life: the crop
    scratch, the device table and the counters are shared by all batches and ordered by that stream alone. When a batch is
    requested from another stream, the feeder makes that stream wait for the batch (an event), so whatever the consumer enqueues after receiving it sees complete
    data; and it orders the reuse of a set after the consumer: each request marks the current stream, and a set is refilled only
    behind the mark made right after its previous batch was handed out. The consumer must therefore have ENQUEUED its reads of
    a batch on the stream it requested it from before it requests the next one (trainer.step does: it copies the batch into its
    own static tensors). The job table travels through `depth` pinned staging buffers; before one is rewritten the host checks
    that its upload of `depth` batches ago has left — the only wait on the production path, and one that has long passed unless
    the host runs `depth` batches ahead of the device."""

    def __init__(self, tracklets, device, batch_size=48, search_size=1024, template_size=512, search_offset=0.0, search_scale=1.25,
                 model_offset=0.0, model_scale=1.25, use_z=True, refine_box=True, candidates_per_frame=4, sampled_interval=1,
                 min_points=20, spare=None, seed=0, shuffle=True, drop_last=True, rank=None, world=None, depth=2, stream=None,
                 augmentor=None):
        self.device = dev = torch.device(device)
        if dev.type != 'cuda':
            raise RuntimeError("TrainBatchFeeder runs on the HIP device (there is no CPU fallback)")
        TrainBatchPlan.__init__(self, tracklets, batch_size, search_size, template_size, search_offset, search_scale, model_offset, model_scale,
                                use_z, refine_box, candidates_per_frame, sampled_interval, min_points, spare, seed, shuffle, drop_last, rank, world,
                                augmentor)
        self.depth = max(1, int(depth))
        # one producer stream for the feeder's whole life: the scratch, the device table and the counters are shared by all batches
        # and ordered by that stream alone
        self.stream = stream if stream is not None else torch.cuda.current_stream(dev)
        self.timing_events = None         # (start, end) HIP events: recorded on the producer stream around the upload and the two launches
        self._issued = 0
        self._warned = False
        self._upload(tracklets)
        self._buffers()

    @classmethod
    def from_config(cls, tracklets, device, data_cfg, batch_size, **kw):
        """The feeder of a DATA_CONFIG section (TrainBatchPlan.config_args); keyword arguments override it."""
        return cls(tracklets, device, batch_size=batch_size, **dict(cls.config_args(data_cfg), **kw))

    # ------------------------------------------------------------------ resident data
    def _upload(self, tracklets):
        """One upload per tracklet: its frames side by side in a (3, sum N_i) buffer (as TrackletRunner._load packs them). A
        tracklet whose clouds are all float32 tensors on this device with adjacent points (SceneStore's views) is used in place:
        pointer and row stride come from the tensor, which is kept alive here — the same bytes, so the same batches."""
        dev = self.device
        self.packed = []
        ptr, ld = [], []
        here = dev if dev.index is not None else torch.device('cuda', torch.cuda.current_device())      # what a tensor's .device says
        for clouds, _ in tracklets:
            if not clouds:
                continue
            if all(isinstance(c, torch.Tensor) and c.device == here and c.dtype == torch.float32 and c.dim() == 2 and c.shape[0] >= 3
                   and c.stride(1) == 1 for c in clouds):
                for c in clouds:
                    self.packed.append(c)
                    ptr.append(c.data_ptr())
                    ld.append(c.stride(0))
                continue
            arrs = [np.ascontiguousarray((c.cpu().numpy() if isinstance(c, torch.Tensor) else np.asarray(c))[0:3], np.float32) for c in clouds]
            sizes = [a.shape[1] for a in arrs]
            total = max(1, sum(sizes))
            packed = torch.from_numpy(np.ascontiguousarray(np.concatenate(arrs + [np.zeros((3, total - sum(sizes)), np.float32)], axis=1))).to(dev)
            self.packed.append(packed)
            offs = np.concatenate([[0], np.cumsum(sizes)])
            for i in range(len(sizes)):
                ptr.append(packed.data_ptr() + int(offs[i]) * 4)
                ld.append(packed.stride(0))
        self.ptr, self.ld = np.array(ptr, np.uint64), np.array(ld, np.int64)

    def _buffers(self):
        dev, C, cap = self.device, self.C, self.cap
        self.crop_out = torch.zeros((C, 3, cap, 3), dtype=torch.float32, device=dev)       # search, first, previous
        self.labels = torch.zeros((C, cap), dtype=torch.uint8, device=dev)
        self.counts = torch.zeros((C, 3), dtype=torch.int32, device=dev)
        self.totals = torch.zeros(4, dtype=torch.int64, device=dev)
        self.jobs_bytes = 3 * C * ops.CROP_JOB.itemsize
        aug_at = self.jobs_bytes + C * ops.TRAIN_CAND.itemsize        # the augmentation records ride at the end of the same table
        nbytes = aug_at + (C * ops.TRAIN_AUG.itemsize if self.aug_steps is not None else 0)
        self.table_dev = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        self.cands_dev = self.table_dev[self.jobs_bytes:]
        self.aug_dev = self.table_dev[aug_at:] if self.aug_steps is not None else None
        out_ptr, cnt_ptr = slot_pointers(self.crop_out.data_ptr(), self.counts.data_ptr(), C, cap)
        lab_ptr = (self.labels.data_ptr() + np.arange(C) * cap).astype(np.uint64)
        self._staging = []
        for _ in range(self.depth):
            pinned = torch.zeros(nbytes, dtype=torch.uint8).pin_memory()
            host = pinned.numpy()
            jobs = host[:self.jobs_bytes].view(ops.CROP_JOB).reshape(C, 3)
            cands = host[self.jobs_bytes:aug_at].view(ops.TRAIN_CAND)
            augs = host[aug_at:].view(ops.TRAIN_AUG) if self.aug_steps is not None else None
            jobs['out'], jobs['count'], jobs['capacity'] = out_ptr, cnt_ptr, cap
            jobs['label_out'][:, 0] = lab_ptr
            cands['search'], cands['first'], cands['prev'] = out_ptr[:, 0], out_ptr[:, 1], out_ptr[:, 2]
            cands['label'], cands['counts'], cands['capacity'] = lab_ptr, cnt_ptr[:, 0], cap
            self._staging.append({'pinned': pinned, 'jobs': jobs, 'cands': cands, 'augs': augs, 'uploaded': torch.cuda.Event(), 'used': False})
        self._sets = [_OutputSet(self, dev) for _ in range(self.depth)]
        self._marks = [torch.cuda.Event() for _ in range(self.depth)]
        self.last = None                                      # the _OutputSet of the latest batch: src, idx_search, idx_template, info
        torch.cuda.current_stream(dev).synchronize()          # the uploads and the zero fills, before another stream touches them

    def _fill(self, st, plan, epoch):
        jobs, cands, src = st['jobs'], st['cands'], plan['_jobs']
        for k, frames in enumerate(plan['_frames']):
            col, n = jobs[:, k], self.npts[frames]
            col['points'] = np.where(n > 0, self.ptr[frames], np.uint64(self.crop_out.data_ptr()))     # an empty frame still carries a valid address
            col['ld'], col['n_points'] = self.ld[frames], n
            for f in ('lo1', 'hi1', 'trans', 'rot', 'lo2', 'hi2'):
                col[f] = src[f][:, k]
        col = jobs[:, 0]
        col['ltrans'], col['lrot'], col['llo'], col['lhi'] = src['trans'][:, 3], src['rot'][:, 3], src['lo2'][:, 3], src['hi2'][:, 3]
        cands['reg'] = plan['reg_label'].astype(np.float32)
        cands['index'], cands['epoch'] = plan['index'].astype(np.uint32), np.uint32(epoch & 0xffffffff)
        if st['augs'] is not None:
            st['augs']['m'], st['augs']['kz'] = plan['aug_map'][:, 0:4], plan['aug_map'][:, 4]

    # ------------------------------------------------------------------ production
    def batch(self, epoch, batch):
        """Enqueue batch `batch` of epoch `epoch` into the next output set and return its dict (see the class text for how long
        the tensors stay valid and what orders producer and consumer)."""
        dev = self.device
        k = self._issued
        self._issued += 1
        out, st = self._sets[k % self.depth], self._staging[k % self.depth]
        cur = torch.cuda.current_stream(dev)
        prod = self.stream
        side = prod != cur
        if side:
            self._marks[k % self.depth].record(cur)
            if k + 1 >= self.depth:
                prod.wait_event(self._marks[(k + 1) % self.depth])     # made right after this set's previous batch was handed out
        if st['used']:
            st['uploaded'].synchronize()                          # the upload of `depth` batches ago has read this staging buffer
        self._fill(st, self.plan(epoch, batch), int(epoch))
        with torch.cuda.stream(prod):
            if self.timing_events is not None:
                self.timing_events[0].record(prod)
            self.table_dev.copy_(st['pinned'], non_blocking=True)
            st['uploaded'].record(prod)
            st['used'] = True
            ops.crop_compact(self.table_dev, 3 * self.C)
            ops.train_batch(self.cands_dev, out.desc, dev, self.aug_dev)
            if self.timing_events is not None:
                self.timing_events[1].record(prod)
            if side:
                out.done.record(prod)
        if side:
            cur.wait_event(out.done)
        self.last = out
        return out.batch

    def __iter__(self):
        epoch = self.epoch
        for b in range(self.n_batches):
            yield self.batch(epoch, b)

    def stats(self):
        """{'batches', 'invalid_primaries', 'shortfall', 'all_invalid'} over the feeder's life, read from the device: waits for
        the batches enqueued so far (the one call here that does). A shortfall — a rejected sample for which no valid spare was
        left, filled by repeating a valid candidate — warns once; raise `spare` if it is frequent."""
        self.stream.synchronize()
        t = self.totals.cpu().tolist()
        out = {'batches': t[0], 'invalid_primaries': t[1], 'shortfall': t[2], 'all_invalid': t[3]}
        if out['shortfall'] and not self._warned:
            self._warned = True
            warnings.warn("TrainBatchFeeder: %d rejected sample(s) in %d batches found no valid spare and repeat another sample of "
                          "their batch; raise `spare` (now %d)" % (out['shortfall'], out['batches'], self.spare), RuntimeWarning, stacklevel=2)
        return out
