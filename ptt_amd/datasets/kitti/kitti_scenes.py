"""KittiTrackingScenes — a KITTI tracking directory turned into what the device loops take: tracklets for TrackletRunner /
PackedTrackletRunner / TrainBatchFeeder / fit, and a per-frame replay for OnlineTracker.step_raw.

The host half (kitti_files.py) reads `root/training/{velodyne,label_02,calib}` (kitti_dataset_tracking.py:25, 266-268), groups the
label rows of one class into tracklets and makes a box of every annotation; the device half is SceneStore: every scan some
tracklet needs is read ONCE, handed to add_scans as the (N, 4) rows np.fromfile gives, de-interleaved and taken into the camera
frame by ptt_scan_ingest_f32 (`steps = [('affine', V2C)]` under REF_COOR camera, none under lidar: :303-308), shared by every
tracklet of that frame, and cropped by ptt_scan_preload_f32 for training (LIDAR_CROP_OFFSET, :40, 309-310).

    ks = KittiTrackingScenes(root, class_name='Car', split='test', ref_coor='camera', device=dev)
    ks.meta, ks.boxes              # per tracklet, no device needed
    ks.load()
    results = PackedTrackletRunner(model, dev).run(ks.tracklets())
    for raw, steps, add, drop in ks.replay('0019'):
        online.step_raw(raw, steps, add=add, drop=drop)

Where this differs from the reference, on purpose:
  * Scene order. The reference walks os.listdir(velodyne), whose order is arbitrary (:270-273); here the scenes of the split
    that exist as directories come in ASCENDING SCENE NUMBER, so the tracklet list is the same on every machine.
  * A scan file whose size is no multiple of 16 bytes (a truncated (N, 4) float32 file) is a ValueError. The reference's bare
    `except` (:312-313) would swallow the reshape error and track on a one-point cloud.
The missing-scan rule is the reference's: KITTI tracking scene 0001 lacks four velodyne files that its labels refer to, and
get_lidar then returns ONE point at the origin, untransformed and uncropped (:312-313). missing='origin' (the default)
reproduces that — a (1, 4) zero row ingested with an empty step list, which preload leaves uncropped; missing='raise' raises
FileNotFoundError instead. Only frames that an annotation of the class refers to are read, as the reference's lazy cache does.
"""
import os

import numpy as np

from . import kitti_files as kf

_ROW_BYTES = 16                        # x, y, z, intensity as float32


class KittiTrackingScenes(object):
    def __init__(self, root, class_name='Car', split='test', ref_coor='camera', device=None, store=None, missing='origin', offset=-1):
        """root: the directory that holds `training/`. class_name: the label type whose tracks are taken. split: what
        kitti_files.scenes_of_split understands. store: a SceneStore to ingest into (default: a new one on `device`, made by
        load()). offset: what tracklets() crops by when it is not told (LIDAR_CROP_OFFSET for training; <= 0: whole scans).
        Construction reads the calibration and label files only; no scan, no device."""
        if str(ref_coor).upper() not in ("CAMERA", "LIDAR"):
            raise ValueError("ref_coor must be camera or lidar, got %r" % (ref_coor,))
        if missing not in ("origin", "raise"):
            raise ValueError("missing must be 'origin' or 'raise', got %r" % (missing,))
        self.root = str(root)
        self.split_path = os.path.join(self.root, "training")
        self.class_name, self.split, self.ref_coor, self.missing = class_name, split, str(ref_coor).lower(), missing
        self.device, self.store, self.offset = device, store, offset
        lidar = os.path.join(self.split_path, "velodyne")
        wanted = set(kf.scenes_of_split(split))
        self.scenes = sorted((d for d in os.listdir(lidar) if d.isdigit() and int(d) in wanted and os.path.isdir(os.path.join(lidar, d))),
                             key=int)
        self.calib, self.meta, self.boxes = {}, [], []
        for scene in self.scenes:
            calib = self.calib[scene] = kf.read_calib(os.path.join(self.split_path, "calib", scene + ".txt"))
            labels = kf.read_labels(os.path.join(self.split_path, "label_02", scene + ".txt"))
            for rows in kf.tracklets_of(labels, class_name):
                self.meta.append({"scene": scene, "track_id": int(rows["track_id"][0]), "frames": [int(f) for f in rows["frame"]],
                                  "rows": rows})
                self.boxes.append([kf.annotation_box(r, calib, self.ref_coor) for r in rows])
        self._missing = set()              # (scene, frame) whose file is absent: the origin point, never cropped
        self._loaded = False

    # ------------------------------------------------------------------ files
    def scan_path(self, scene, frame):
        return os.path.join(self.split_path, "velodyne", scene, "%06d.bin" % frame)

    def frames_of(self, scene):
        """The frames of `scene` that an annotation of the class refers to, ascending."""
        return sorted({f for m in self.meta if m["scene"] == scene for f in m["frames"]})

    def steps_of(self, scene):
        """The scans' way into the frame the boxes live in (:305-307)."""
        return [('affine', self.calib[scene].V2C)] if self.ref_coor == "camera" else []

    def _present(self, scene, frame):
        """True: the scan file is there and whole; False: it is absent and missing='origin'. Raises otherwise."""
        path = self.scan_path(scene, frame)
        if not os.path.isfile(path):
            if self.missing == "raise":
                raise FileNotFoundError(path)
            return False
        if os.path.getsize(path) % _ROW_BYTES:
            raise ValueError("%s: %d bytes is no whole number of (x, y, z, intensity) float32 rows" % (path, os.path.getsize(path)))
        return True

    def _read(self, scene, frame, present):
        """-> (raw (N, 4) float32 as read, its step list)."""
        if not present:
            return np.zeros((1, 4), np.float32), []
        return np.fromfile(self.scan_path(scene, frame), dtype=np.float32).reshape(-1, 4), self.steps_of(scene)

    # ------------------------------------------------------------------ device
    def load(self):
        """Every scan file is checked first (absent under missing='raise': FileNotFoundError; truncated: ValueError — the store
        is untouched), then each is read once and every scene goes to the store in one add_scans call. -> self."""
        if self._loaded:
            return self
        present = {(s, f): self._present(s, f) for s in self.scenes for f in self.frames_of(s)}
        if self.store is None:
            from ...scene_store import SceneStore
            self.store = SceneStore(self.device)
        for scene in self.scenes:
            frames = self.frames_of(scene)
            if not frames:
                continue
            read = [self._read(scene, f, present[(scene, f)]) for f in frames]
            self.store.add_scans(scene, frames, [r for r, _ in read], steps=[s for _, s in read] if self.ref_coor == "camera" else [])
            self._missing.update((scene, f) for f in frames if not present[(scene, f)])
        self._loaded = True
        return self

    def tracklets(self, offset=None):
        """-> [(clouds, boxes)] per tracklet, in the order of `meta`: the store's shared views for offset <= 0 (two tracklets over
        one frame get the same memory), SceneStore.preload's crops for offset > 0 — except a missing scan's origin point, which
        stays as it is. offset None: the one given at construction."""
        self.load()
        offset = self.offset if offset is None else offset
        out = []
        for m, boxes in zip(self.meta, self.boxes):
            scene, frames = m["scene"], m["frames"]
            if not float(offset) > 0:
                out.append(self.store.tracklet(scene, frames, boxes))
                continue
            there = [i for i, f in enumerate(frames) if (scene, f) not in self._missing]
            crops, _ = self.store.preload(scene, [frames[i] for i in there], [boxes[i] for i in there], offset)
            clouds = [self.store.scan(scene, f) for f in frames]
            for i, c in zip(there, crops):
                clouds[i] = c
            out.append((clouds, list(boxes)))
        return out

    # ------------------------------------------------------------------ live replay
    def replay(self, scene):
        """The scene as a live integrator would meet it, for OnlineTracker.step_raw: per annotated frame, ascending,
        (raw (N, 4), steps, add {target id: box}, drop (target ids)). A track is added, with its annotation box, on the frame of
        its first row and dropped on the frame after its last row; where its frame numbers have a gap it is dropped at the gap
        and added again afterwards under the new id (track_id, k), k = 1, 2, ... Each file is read when its frame comes up."""
        if scene not in self.calib:
            raise KeyError("scene %r is not in split %r under %s" % (scene, self.split, self.split_path))
        add_at, last_of = {}, {}
        for m, boxes in zip(self.meta, self.boxes):
            if m["scene"] != scene:
                continue
            k, frames = 0, m["frames"]
            for i, f in enumerate(frames):
                if i == 0 or f != frames[i - 1] + 1:
                    target = m["track_id"] if k == 0 else (m["track_id"], k)
                    add_at.setdefault(f, {})[target] = boxes[i]
                    k += 1
                last_of[target] = f
        live = []
        for f in self.frames_of(scene):
            drop = tuple(t for t in live if last_of[t] < f)
            add = add_at.get(f, {})
            live = [t for t in live if t not in drop] + list(add)
            raw, steps = self._read(scene, f, self._present(scene, f))
            yield raw, steps, add, drop


def kitti_tracklets(data_cfg, class_names, training, device, root=None, store=None, missing='origin'):
    """The dataset of a reference DATA_CONFIG, loaded: DATA_PATH (or `root`), DATA_SPLIT[train | test], REF_COOR, and
    LIDAR_CROP_OFFSET as the preload offset when training, -1 otherwise (:40). class_names: the one class name, or a list
    holding it. -> the loaded KittiTrackingScenes; .tracklets() is what the runners, the feeder and fit take."""
    if not isinstance(class_names, str):
        class_names = list(class_names)
        if len(class_names) != 1:
            raise ValueError("one class is tracked at a time, got %r" % (class_names,))
        class_names = class_names[0]
    mode = 'train' if training else 'test'
    ks = KittiTrackingScenes(data_cfg['DATA_PATH'] if root is None else root, class_name=class_names, split=data_cfg['DATA_SPLIT'][mode],
                             ref_coor=data_cfg['REF_COOR'], device=device, store=store, missing=missing,
                             offset=data_cfg['LIDAR_CROP_OFFSET'] if training else -1)
    return ks.load()
