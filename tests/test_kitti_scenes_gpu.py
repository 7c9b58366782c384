"""KittiTrackingScenes on the GPU, bit for bit against fixture G28 (tests/golden/make_golden_g28.py: the reference's own
KittiTrackingDataset on the tree tests/kitti_tree.py writes) and against the same loops fed from host arrays:

  1. load(): every resident scan == the reference's pc.points, camera and lidar; the missing frame is the one origin point; two
     tracklets over one frame share memory; each .bin is read once, each scene is one add_scans call;
  2. tracklets(offset=10) == the reference's train-mode clouds, the uncropped origin point included;
  3. PackedTrackletRunner on ks.tracklets() == on host tracklets, and eval_metrics.evaluate gives the same numbers;
  4. TrainBatchFeeder on tracklets(offset=10) == on host-built preloaded tracklets;
  5. OnlineTracker.step_raw driven by replay('0019') == step driven by hand on the host-transformed scans;
  6. missing='raise' and a truncated .bin raise before the store changes.

A difference in 1 or 2 is a finding about SceneStore.add_scans / preload: nothing here has a tolerance.
"""
import os
import shutil

import numpy as np
import pytest
import torch

from tests import kitti_tree
from tests import scene_ref as SR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_cache = {}


def _g28():
    if "g28" not in _cache:
        _cache["g28"] = dict(np.load(os.path.join(ROOT, "tests", "golden", "G28_kitti_files.npz")))
    return _cache["g28"]


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("kitti")
    kitti_tree.write_tree(str(root), int(_g28()["seed"]))
    return str(root)


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _same_bits(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    assert np.array_equal(g, w), "%s: %d of %d words differ" % (what, int((g != w).sum()), g.size)


def _scenes(tree, dev, coor, **kw):
    """The loaded dataset of one REF_COOR over all three scenes, shared by the tests that only read it."""
    from ptt_amd.datasets.kitti.kitti_scenes import KittiTrackingScenes
    if kw:
        return KittiTrackingScenes(tree, class_name='Car', split='all', ref_coor=coor, device=dev, **kw)
    if coor not in _cache:
        _cache[coor] = KittiTrackingScenes(tree, class_name='Car', split='all', ref_coor=coor, device=dev).load()
    return _cache[coor]


def _host_tracklets(ks, coor, offset=None):
    """The same tracklets from the fixture's arrays: private host copies of the reference's clouds, the dataset's boxes."""
    g = _g28()
    out = []
    for m, boxes in zip(ks.meta, ks.boxes):
        key = ("scan_%s_%s_%%d" % (coor, m["scene"])) if offset is None else ("crop_%s_%s_%d_%%d" % (coor, m["scene"], m["track_id"]))
        out.append(([g[key % f].copy() for f in m["frames"]], boxes))
    return out


# ------------------------------------------------------------------------------------------------------------ 1. whole scans
@pytest.mark.parametrize("coor", ["camera", "lidar"])
def test_load_gives_the_references_scans(dev, tree, coor, monkeypatch):
    from ptt_amd.scene_store import SceneStore
    g = _g28()
    reads, calls = [], []
    fromfile = np.fromfile
    monkeypatch.setattr(np, "fromfile", lambda path, *a, **k: (reads.append(str(path)), fromfile(path, *a, **k))[1])
    store = SceneStore(dev)
    add_scans = store.add_scans
    store.add_scans = lambda scene, *a, **k: (calls.append(scene), add_scans(scene, *a, **k))[1]
    ks = _scenes(tree, dev, coor, store=store)
    assert len(store) == 0 and ks.load() is ks and ks.load() is ks
    monkeypatch.undo()
    n_files = len(kitti_tree.SCENES) * kitti_tree.FRAMES - 1
    assert len(reads) == len(set(reads)) == n_files and all(r.endswith(".bin") for r in reads)           # each .bin once
    assert calls == list(kitti_tree.SCENES) and len(store) == n_files + 1                                 # one add_scans per scene
    for scene in kitti_tree.SCENES:
        for f in range(kitti_tree.FRAMES):
            _same_bits(store.scan(scene, f), g["scan_%s_%s_%d" % (coor, scene, f)], "%s scan %s/%d" % (coor, scene, f))
    origin = store.scan(*kitti_tree.MISSING)
    assert tuple(origin.shape) == (3, 1) and not bool(origin.any())
    tr = ks.tracklets()
    assert len(tr) == 6 and [len(c) for c, _ in tr] == [4] * 6 and all(b is not None and len(b) == 4 for _, b in tr)
    for s in range(3):                                               # track 1 over frames 0..3, track 0 over 1..4: frames 1..3 are shared
        a, b = tr[2 * s][0], tr[2 * s + 1][0]
        assert [t.data_ptr() for t in a[1:4]] == [t.data_ptr() for t in b[0:3]] and a[0].data_ptr() != b[0].data_ptr()
        assert len({t.untyped_storage().data_ptr() for t in a + b}) == 1                                  # one buffer per scene
    _cache.setdefault(coor, ks)


# ------------------------------------------------------------------------------------------------------- 2. preloaded crops
@pytest.mark.parametrize("coor", ["camera", "lidar"])
def test_preloaded_tracklets_equal_the_references_train_mode(dev, tree, coor):
    g = _g28()
    ks = _scenes(tree, dev, coor)
    offset = int(g["offset"])
    tr = ks.tracklets(offset=offset)
    kept = []
    for m, (clouds, boxes) in zip(ks.meta, tr):
        assert len(clouds) == len(boxes) == len(m["frames"])
        for f, c in zip(m["frames"], clouds):
            want = g["crop_%s_%s_%d_%d" % (coor, m["scene"], m["track_id"], f)]
            _same_bits(c, want, "%s crop %s track %d frame %d" % (coor, m["scene"], m["track_id"], f))
            whole = ks.store.scan(m["scene"], f).shape[1]
            if (m["scene"], f) == kitti_tree.MISSING:
                assert tuple(c.shape) == (3, 1) and not bool(c.any())          # the origin point, handed on as it is
                assert c.data_ptr() == ks.store.scan(m["scene"], f).data_ptr()
            else:
                assert 30 <= c.shape[1] < whole                                # a real crop
                kept.append(c.shape[1])
    assert len(kept) == 22
    # offset <= 0 and the constructor's default: the store's own views
    assert [c.data_ptr() for c in ks.tracklets()[0][0]] == [c.data_ptr() for c in ks.tracklets(offset=-1)[0][0]] \
        == [ks.store.scan("0000", f).data_ptr() for f in ks.meta[0]["frames"]]


def test_kitti_tracklets_reads_the_data_config(dev, tree):
    from ptt_amd.config import EasyDict
    from ptt_amd.datasets.kitti import kitti_tracklets
    g = _g28()
    cfg = EasyDict(DATA_PATH=tree, DATA_SPLIT={'train': 'train', 'test': 'test'}, REF_COOR='lidar', LIDAR_CROP_OFFSET=int(g["offset"]))
    train = kitti_tracklets(cfg, ['Car'], True, dev)
    test = kitti_tracklets(cfg, 'Car', False, dev, root=tree)
    assert train.scenes == ["0000"] and test.scenes == ["0019", "0020"] and train.offset == 10 and test.offset == -1
    for ks in (train, test):                                         # train: LIDAR_CROP_OFFSET crops; test: whole scans
        for m, (clouds, _) in zip(ks.meta, ks.tracklets()):
            for f, c in zip(m["frames"], clouds):
                key = "crop_lidar_%s_%d_%d" % (m["scene"], m["track_id"], f) if ks is train else "scan_lidar_%s_%d" % (m["scene"], f)
                _same_bits(c, g[key], key)
    with pytest.raises(ValueError):
        kitti_tracklets(cfg, ['Car', 'Pedestrian'], False, dev)


# ------------------------------------------------------------------------------------------------- 3. the packed runner
def test_packed_runner_on_the_files_equals_host_tracklets(dev, tree):
    from ptt_amd import eval_metrics
    from ptt_amd.packed_runner import PackedTrackletRunner
    from tests.test_online_tracker_gpu import _tracker
    ks = _scenes(tree, dev, "camera")
    shared, private = ks.tracklets(), _host_tracklets(ks, "camera")
    pr = PackedTrackletRunner(_tracker(dev), dev, slots=4)
    got, want = pr.run(shared), pr.run(private)
    assert [len(r) for r in got] == [len(r) for r in want] == [4] * 6
    moved = 0
    for t, (g_rows, w_rows) in enumerate(zip(got, want)):
        for i, (a, b) in enumerate(zip(g_rows, w_rows)):
            assert len(a) == len(b)
            for x, y in zip(a[:3], b[:3]):
                np.testing.assert_array_equal(x, y, err_msg="tracklet %d frame %d" % (t, i))
            assert len(b) == 3 or a[3] == b[3]
            moved += int(i > 0 and float(np.abs(a[0] - w_rows[0][0]).max()) > 1e-6)
    assert moved > 0
    ea = eval_metrics.evaluate(got, shared, ref_coord='camera', device=dev)
    eb = eval_metrics.evaluate(want, private, ref_coord='camera', device=dev)
    assert ea["success"] == eb["success"] and ea["precision"] == eb["precision"] and ea["frames"].tolist() == [4] * 6
    assert np.array_equal(ea["overlap"], eb["overlap"]) and np.array_equal(ea["accuracy"], eb["accuracy"])
    assert 0.0 < ea["success"] <= 100.0                                           # frame 0 of every tracklet scores its own box
    _cache["packed"] = (got, ea)


def test_kitti_eval_scores_and_writes_the_result_file(dev, tree, tmp_path):
    """The tool's core on the same dataset: the numbers of the run above, and one result line per frame."""
    import io
    from ptt_amd.datasets.kitti import kitti_files as kf
    from ptt_amd.tools.kitti_eval import evaluate_scenes, parse_args
    from tests.test_online_tracker_gpu import _tracker
    ks = _scenes(tree, dev, "camera")
    path = str(tmp_path / "track_result.txt")
    res = evaluate_scenes(_tracker(dev), ks, {}, None, slots=4, results=path)
    lines = open(path).read().splitlines()
    assert len(lines) == 24 and all(len(l.split()) == 27 for l in lines)
    assert [l.split()[:3] for l in lines[:5]] == [["0000", str(f), "0"] for f in (0, 1, 2, 3)] + [["0000", "1", "1"]]
    fp = io.StringIO()
    kf.write_track_results(fp, "0000", 0, 0, ks.boxes[0][0])                       # frame 0's result is the annotation's box
    assert fp.getvalue() == lines[0] + "\n"
    if "packed" in _cache:
        got, ea = _cache["packed"]
        assert res["success"] == ea["success"] and res["precision"] == ea["precision"] and np.array_equal(res["overlap"], ea["overlap"])
    a = parse_args(["--cfg_file", "c.yaml", "--ckpt", "m.pth"])
    assert (a.data_path, a.split, a.slots, a.results, a.missing) == (None, None, 48, None, "origin")


def test_kitti_eval_from_a_config_file_and_a_checkpoint(dev, tree, tmp_path, capsys):
    """The command line in process: a reference-style YAML and a checkpoint of the tests' tracker give the numbers of the run above."""
    import json
    import yaml
    from ptt_amd import fit
    from ptt_amd.config import ptt_model_cfg
    from ptt_amd.tools import kitti_eval
    from tests.test_online_tracker_gpu import _tracker
    plain = lambda d: {k: plain(v) for k, v in d.items()} if isinstance(d, dict) else d
    cfg = dict(CLASS_NAMES=['Car'], MODEL=plain(ptt_model_cfg()), TEST=dict(SHAPE_AGGREGATION='firstandprevious', REF_BOX='previous_result'),
               DATA_CONFIG=dict(DATA_PATH=str(tmp_path / "nowhere"), DATA_SPLIT={'train': 'train', 'test': 'val'}, REF_COOR='camera',
                                LIDAR_CROP_OFFSET=10))
    (tmp_path / "ptt.yaml").write_text(yaml.safe_dump(cfg))
    ckpt = fit.save_checkpoint(fit.checkpoint_state(_tracker(dev), None, 1, 1), str(tmp_path / "checkpoint_epoch_1"))
    res = kitti_eval.main(["--cfg_file", str(tmp_path / "ptt.yaml"), "--ckpt", ckpt, "--data_path", tree, "--split", "all", "--slots", "4",
                           "--results", str(tmp_path / "track_result.txt")])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line == {"success": res["success"], "precision": res["precision"], "tracklets": 6, "frames": 24}
    assert len((tmp_path / "track_result.txt").read_text().splitlines()) == 24
    if "packed" in _cache:
        assert res["success"] == _cache["packed"][1]["success"] and np.array_equal(res["overlap"], _cache["packed"][1]["overlap"])


def test_fit_from_kitti_hands_the_files_tracklets_to_from_config(dev, tree, tmp_path, monkeypatch):
    from ptt_amd import fit
    from ptt_amd.config import EasyDict
    g = _g28()
    seen = {}

    def from_config(cfg, train_tracklets, device, ckpt_dir, val_tracklets=None, **kw):
        seen.update(train=train_tracklets, val=val_tracklets, kw=kw, ckpt_dir=ckpt_dir)
        return lambda **more: []
    monkeypatch.setattr(fit, "from_config", from_config)
    cfg = EasyDict(CLASS_NAMES=['Car'], TRAIN=dict(WITH_EVAL=dict(ENABLE=True, START_EPOCH=0, INTERVAL=1)),
                   DATA_CONFIG=dict(DATA_PATH=tree, DATA_SPLIT={'train': 'train', 'test': 'test'}, REF_COOR='camera', LIDAR_CROP_OFFSET=int(g["offset"])))
    run = fit.from_kitti(cfg, dev, str(tmp_path), slots=4)
    assert seen["kw"] == dict(slots=4) and seen["ckpt_dir"] == str(tmp_path)
    assert run.train_scenes.scenes == ["0000"] and run.val_scenes.scenes == ["0019", "0020"] and len(seen["train"]) == 2 and len(seen["val"]) == 4
    m = run.train_scenes.meta[0]
    _same_bits(seen["train"][0][0][0], g["crop_camera_0000_%d_%d" % (m["track_id"], m["frames"][0])], "the first training cloud")
    _same_bits(seen["val"][0][0][0], g["scan_camera_0019_0"], "the first validation cloud")
    cfg.TRAIN.WITH_EVAL.ENABLE = False
    run = fit.from_kitti(cfg, dev, str(tmp_path), root=tree)
    assert run.val_scenes is None and seen["val"] is None and len(seen["train"]) == 2


# ---------------------------------------------------------------------------------------------------------- 4. the feeder
def test_feeder_on_preloaded_tracklets_equals_host_tracklets(dev, tree):
    from ptt_amd.train_feed import TrainBatchFeeder
    ks = _scenes(tree, dev, "camera")
    offset = int(_g28()["offset"])
    kw = dict(batch_size=4, search_size=128, template_size=64, seed=28)
    fa = TrainBatchFeeder(ks.tracklets(offset=offset), dev, **kw)
    fb = TrainBatchFeeder(_host_tracklets(ks, "camera", offset), dev, **kw)
    assert len(fa) == len(fb) >= 1
    ba, bb = fa.batch(0, 0), fb.batch(0, 0)
    torch.cuda.synchronize()
    for key in ('search_points', 'template_points', 'cls_label', 'reg_label'):
        assert ba[key].shape[0] == 4 and torch.equal(ba[key].view(torch.int32), bb[key].view(torch.int32)), key
    assert float(ba['search_points'].abs().max()) > 0 and torch.equal(fa.last.src, fb.last.src)


# ----------------------------------------------------------------------------------------------------- 5. the online replay
def test_replay_drives_step_raw_as_step_driven_by_hand(dev, tree):
    from ptt_amd.online_tracker import OnlineTracker
    from tests.test_online_tracker_gpu import _tracker
    g = _g28()
    ks = _scenes(tree, dev, "camera")
    a = OnlineTracker(_tracker(dev), dev, slots=4, scan_capacity=512)
    b = OnlineTracker(_tracker(dev), dev, slots=4, scan_capacity=512)
    box = {(m["track_id"], f): bx for m, boxes in zip(ks.meta, ks.boxes) if m["scene"] == "0019" for f, bx in zip(m["frames"], boxes)}
    adds = {0: {1: box[(1, 0)]}, 1: {0: box[(0, 1)]}}                     # track 1 lives over frames 0..3, track 0 over 1..4
    drops = {4: (1,)}
    v2c = ks.calib["0019"].V2C
    scored = 0
    for f, (raw, steps, add, drop) in enumerate(ks.replay("0019")):
        planar = SR.ingest_ref(np.fromfile(ks.scan_path("0019", f), np.float32).reshape(-1, 4), [('affine', v2c)])
        _same_bits(planar, g["scan_camera_0019_%d" % f], "host-transformed scan %d" % f)
        got = a.step_raw(raw, steps, add=add, drop=drop)
        want = b.step(planar, add=adds.get(f), drop=drops.get(f, ()))
        assert list(got) == list(want) == {0: [1], 1: [1, 0], 2: [1, 0], 3: [1, 0], 4: [0]}[f]
        for i in want:
            for x, y in zip(got[i][:3], want[i][:3]):
                np.testing.assert_array_equal(x, y, err_msg="target %s frame %d" % (i, f))
            assert got[i][3] == want[i][3], (i, f, got[i][3], want[i][3])
            scored += int(want[i][3] is not None)
        _same_bits(a.scans[1 - a.cur, :, :a.n_prev], planar, "the resident scan of frame %d" % f)
    assert f == 4 and scored == 6


# ---------------------------------------------------------------------------------------------------------------- 6. errors
def test_missing_and_truncated_scans_raise_before_the_store_changes(dev, tree, tmp_path):
    from ptt_amd.scene_store import SceneStore
    store = SceneStore(dev)
    ks = _scenes(tree, dev, "camera", store=store, missing='raise')
    with pytest.raises(FileNotFoundError, match="0020"):
        ks.load()
    assert len(store) == 0 and store.nbytes == 0
    with pytest.raises(FileNotFoundError):
        ks.tracklets()
    assert len(store) == 0
    cut = str(tmp_path / "cut")
    shutil.copytree(tree, cut)
    path = os.path.join(cut, "training", "velodyne", "0019", "000004.bin")            # the last file of a later scene
    os.truncate(path, os.path.getsize(path) - 4)
    for missing in ("origin", "raise"):                     # scene 0019 is checked before 0020's absent file: a ValueError in both modes
        with pytest.raises(ValueError, match="000004.bin"):
            _scenes(cut, dev, "lidar", store=store, missing=missing).load()
        assert len(store) == 0
