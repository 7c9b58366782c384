"""SceneStore — the sensor's raw scans ingested once, kept on the device and shared by every tracklet that passes through them.

The reference keeps `self.lidar_frames[scene][frame]` (KittiTrackingDataset.get_lidar, ptt/datasets/kitti/kitti_dataset_tracking.py:
298-313): a scan is read as interleaved (N, 4) rows (nuScenes: 5 floats per row, PointCloud.load_pcd_bin), reduced to its first
three columns, taken into the reference frame (PointCloud.transform(V2C) under REF_COOR = camera; rotate / translate / rotate /
translate in nus_dataset_tracking.py:140-145) and then handed to every tracklet of that frame; for training, crop_pc(pc, box,
offset=LIDAR_CROP_OFFSET) of it is what the database stores. Here:

    store = SceneStore(device)
    store.add_scans("0019", frames, raws, steps=[('affine', V2C)])      # one upload, one ptt_scan_ingest_f32 launch
    store.scan("0019", 7)                                               # a (3, N) view
    clouds, boxes = store.tracklet("0019", frames, boxes)               # views only: what the runners take
    clouds, boxes = store.preload("0019", frames, boxes, offset=cfg.DATA_CONFIG.LIDAR_CROP_OFFSET)      # ptt_scan_preload_f32
    store.nbytes; ("0019", 7) in store; store.release("0019")

The scans of one add_scans call end up side by side in ONE (3, sum N_i) buffer — points adjacent, rows stride(0) apart: the
layout tracklet_runner.upload_clouds uses in place — so TrackletRunner, PackedTrackletRunner and TrainBatchFeeder read them where
they are, and two tracklets over the same frame read the same memory. File reading, calibration parsing and the annotation
tables stay with the caller: the store starts at arrays.
"""
import numpy as np
import torch

from . import ops
from .datasets.kitti import box_math as bm

_JOBS_PER_LAUNCH = 65535          # the grid's second dimension


def check_raw(raw, device, max_points=None):
    """-> the raw scan as a torch tensor (host or `device`), without a copy. ValueError for anything but an (N, C) float32
    C-contiguous numpy array or contiguous torch tensor (on the host, or on `device`) with 3 <= C <= 16, and for N > max_points."""
    if isinstance(raw, np.ndarray):
        if raw.dtype != np.float32 or raw.ndim != 2 or not raw.flags['C_CONTIGUOUS']:
            raise ValueError("a raw scan must be an (N, C) float32 C-contiguous array, got %s %s" % (raw.dtype, raw.shape))
        t = torch.from_numpy(raw)
    elif isinstance(raw, torch.Tensor):
        if raw.dtype != torch.float32 or raw.dim() != 2 or not raw.is_contiguous():
            raise ValueError("a raw scan must be a contiguous (N, C) float32 tensor, got %s %s" % (raw.dtype, tuple(raw.shape)))
        if raw.is_cuda and raw.device != device:
            raise ValueError("a raw scan lives on %s, its consumer on %s" % (raw.device, device))
        t = raw.detach()
    else:
        raise ValueError("a raw scan must be a numpy array or a torch tensor, got %s" % type(raw).__name__)
    if not ops.SCAN_ROW_FLOATS_MIN <= t.shape[1] <= ops.SCAN_ROW_FLOATS_MAX:
        raise ValueError("a raw scan has %d..%d floats per point, got %d" % (ops.SCAN_ROW_FLOATS_MIN, ops.SCAN_ROW_FLOATS_MAX, t.shape[1]))
    if max_points is not None and t.shape[0] > max_points:
        raise ValueError("raw scan of %d points, capacity %d" % (t.shape[0], max_points))
    return t


def _whole_call(steps):
    """True when `steps` is one step list for every scan: empty, or a list whose entries are (kind, matrix) pairs."""
    return len(steps) == 0 or all(isinstance(s, (tuple, list)) and len(s) == 2 and isinstance(s[0], str) for s in steps)


class SceneStore(object):
    def __init__(self, device):
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError("SceneStore runs on the HIP device (there is no CPU fallback)")
        if self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        self._scans = {}                  # (scene, frame) -> (view, the buffer of its add_scans call)

    # ------------------------------------------------------------------ what is resident
    def __contains__(self, key):
        return tuple(key) in self._scans if isinstance(key, (tuple, list)) and len(key) == 2 else False

    def __len__(self):
        return len(self._scans)

    @property
    def nbytes(self):
        """Device bytes of the buffers the store holds a scan of (a buffer counts once, and as long as one of its scans is resident)."""
        bufs = {buf.data_ptr(): buf for _, buf in self._scans.values()}
        return sum(b.numel() * b.element_size() for b in bufs.values())

    def frames(self, scene):
        return sorted(f for s, f in self._scans if s == scene)

    def release(self, scene):
        """Drop the store's references to every scan of `scene`. Tensors handed out earlier stay valid as long as someone holds them."""
        for key in [k for k in self._scans if k[0] == scene]:
            del self._scans[key]

    # ------------------------------------------------------------------ ingest
    def add_scans(self, scene, frames, raws, steps=None):
        """raws[i]: the (N_i, C_i) float32 scan of frame frames[i] — a C-contiguous numpy array, a host tensor (a pinned one is
        copied asynchronously: leave it alone until the stream has passed) or a tensor on the device (read in place);
        3 <= C_i <= 16, N_i = 0 allowed. steps: the way into the reference frame for every scan of the call (ops.scan_steps'
        list), or a list with one such list per frame. The host scans are staged side by side and uploaded once; one
        ptt_scan_ingest_f32 launch writes all scans into one (3, sum N_i) buffer. ValueError — a (scene, frame) that is already
        resident or listed twice, a bad array, mismatched lengths, bad steps — before anything changes."""
        dev = self.device
        frames, raws = list(frames), list(raws)
        if len(frames) != len(raws):
            raise ValueError("add_scans: %d frames, %d scans" % (len(frames), len(raws)))
        keys = [(scene, f) for f in frames]
        if len(set(keys)) != len(keys):
            raise ValueError("add_scans: a frame is listed twice")
        for key in keys:
            if key in self._scans:
                raise ValueError("add_scans: scene %r frame %r is already resident" % key)
        steps = [] if steps is None else list(steps)
        if _whole_call(steps):
            recs = [ops.scan_steps(steps)] * len(frames)
        elif len(steps) != len(frames):
            raise ValueError("add_scans: steps is neither one step list nor one per frame (%d entries, %d frames)" % (len(steps), len(frames)))
        else:
            recs = [ops.scan_steps(s) for s in steps]
        tensors = [check_raw(r, dev) for r in raws]
        if not frames:
            return
        # ---- nothing raised: stage, upload, ingest
        sizes = np.array([t.shape[0] for t in tensors], np.int64)
        width = np.array([t.shape[1] for t in tensors], np.int64)
        offs = np.concatenate([[0], np.cumsum(sizes)])
        # the staging buffer: pageable host scans first (one region, one upload), then the pinned ones (one asynchronous copy
        # each); every scan starts on 16 bytes, so that 4-float rows take the 16-byte loads. Device scans are read where they are.
        host = [i for i, t in enumerate(tensors) if not t.is_cuda and not t.is_pinned()]
        pinned = [i for i, t in enumerate(tensors) if not t.is_cuda and t.is_pinned()]
        at, total = {}, 0
        for i in host + pinned:
            at[i] = total
            total += -(-int(sizes[i] * width[i]) // 4) * 4
        n_host = at[pinned[0]] if pinned else total
        with torch.cuda.device(dev):
            stage = torch.empty(max(1, total), dtype=torch.float32, device=dev)
            if host and n_host:
                flat = np.zeros(n_host, np.float32)
                for i in host:
                    flat[at[i]:at[i] + int(sizes[i] * width[i])] = tensors[i].numpy().reshape(-1)
                stage[:n_host].copy_(torch.from_numpy(flat))
            for i in pinned:
                stage[at[i]:at[i] + int(sizes[i] * width[i])].copy_(tensors[i].reshape(-1), non_blocking=True)
            packed = torch.empty((3, max(1, int(offs[-1]))), dtype=torch.float32, device=dev)
        jobs = np.zeros(len(frames), ops.SCAN_JOB)
        for i, t in enumerate(tensors):
            jobs['raw'][i] = t.data_ptr() if t.is_cuda else stage.data_ptr() + at[i] * 4
            jobs['steps'][i, :len(recs[i])] = recs[i]
            jobs['n_steps'][i] = len(recs[i])
        jobs['out'] = packed.data_ptr() + offs[:-1] * 4
        jobs['ld'], jobs['n_points'], jobs['row_floats'] = packed.stride(0), sizes, width
        if int(offs[-1]) > 0:
            for lo in range(0, len(jobs), _JOBS_PER_LAUNCH):
                part = jobs[lo:lo + _JOBS_PER_LAUNCH]
                ops.scan_ingest(part, len(part), max(1, int(part['n_points'].max())), dev)
        for i, key in enumerate(keys):
            self._scans[key] = (packed[:, int(offs[i]):int(offs[i + 1])], packed)

    # ------------------------------------------------------------------ hand-out
    def scan(self, scene, frame):
        """The (3, N) float32 view of a resident scan inside its call's shared buffer. KeyError if it is not resident."""
        try:
            return self._scans[(scene, frame)][0]
        except KeyError:
            raise KeyError("scene %r frame %r is not resident" % (scene, frame))

    def tracklet(self, scene, frames, boxes):
        """-> (clouds, boxes) as TrackletRunner.run / PackedTrackletRunner.run / TrainBatchFeeder take a tracklet: the scans' views
        (nothing is copied: two tracklets over one frame get tensors with the same data_ptr()) and the boxes as a list."""
        frames, boxes = list(frames), list(boxes)
        if len(frames) != len(boxes):
            raise ValueError("tracklet: %d frames, %d boxes" % (len(frames), len(boxes)))
        return [self.scan(scene, f) for f in frames], boxes

    def preload(self, scene, frames, boxes, offset):
        """Per frame crop_pc(scan, box, offset=offset) (kitti_tracking_utils.py:275-297; get_lidar's preload, :309-310), on the
        device: -> (clouds, boxes) whose clouds are (3, count_i) views into ONE packed buffer of exactly sum count_i points.
        boxes[i] = (center (3), wlh (3), quaternion (w, x, y, z)). A counting launch, one read-back of the counts, a writing launch.
        offset <= 0 returns tracklet()'s views: the reference crops only when the offset is positive."""
        clouds, boxes = self.tracklet(scene, frames, boxes)
        if not float(offset) > 0 or not clouds:
            return clouds, boxes
        dev, n = self.device, len(clouds)
        jobs = np.zeros(n, ops.PRELOAD_JOB)
        for i, (c, box) in enumerate(zip(clouds, boxes)):
            center, wlh, quat = (np.asarray(v, np.float64).reshape(-1) for v in box)
            if (center.shape, wlh.shape, quat.shape) != ((3,), (3,), (4,)):
                raise ValueError("a box is (center (3), wlh (3), quaternion (w, x, y, z))")
            corners = bm.corners(center, wlh * 1.0, bm.q_rotation_matrix(quat))            # crop_pc :276-279 at scale 1.0
            jobs['hi'][i] = np.max(corners, 1) + offset
            jobs['lo'][i] = np.min(corners, 1) - offset
            jobs['points'][i], jobs['ld'][i], jobs['n_points'][i] = c.data_ptr(), c.stride(0), c.shape[1]
        max_points = max(1, int(jobs['n_points'].max()))
        with torch.cuda.device(dev):
            counts_dev = torch.zeros(n, dtype=torch.int32, device=dev)
            jobs['count'] = counts_dev.data_ptr() + np.arange(n) * 4
            ws = None
            for lo in range(0, n, _JOBS_PER_LAUNCH):                       # out = NULL: count only
                part = jobs[lo:lo + _JOBS_PER_LAUNCH]
                ws = ops._ws(ops.scan_preload_workspace(len(part), max_points), dev) if ws is None else ws
                ops.scan_preload_device(ops.upload_jobs(part), len(part), max_points, ws)
            counts = counts_dev.cpu().numpy().astype(np.int64)             # the one read-back
            offs = np.concatenate([[0], np.cumsum(counts)])
            packed = torch.empty((3, max(1, int(offs[-1]))), dtype=torch.float32, device=dev)
            jobs['out'], jobs['out_ld'], jobs['capacity'] = packed.data_ptr() + offs[:-1] * 4, packed.stride(0), counts
            for lo in range(0, n, _JOBS_PER_LAUNCH):
                part = jobs[lo:lo + _JOBS_PER_LAUNCH]
                ops.scan_preload_device(ops.upload_jobs(part), len(part), max_points, ws)
        return [packed[:, int(offs[i]):int(offs[i + 1])] for i in range(n)], boxes
