"""SceneStore without a GPU: the numpy restatements of the two scan kernels against fixture g26 (made from the reference's own
PointCloud / crop_pc) bit for bit, the C ABI of ptt_scan_ingest_f32 / ptt_scan_preload_f32 as the header declares it and the
binding mirrors it, and every refusal the host side makes before anything reaches the device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import scene_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _g26():
    return np.load(os.path.join(ROOT, "tests", "golden", "g26_scene_store.npz"))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def test_restatement_equals_the_reference_fixture():
    g = _g26()
    assert [g["raw_%d" % k].shape for k in range(4)] == [(1500, 4), (2049, 4), (1025, 4), (777, 5)]
    for k in range(3):
        got = SR.ingest_ref(g["raw_%d" % k], [('affine', g["v2c"])])
        assert got.dtype == np.float32 and np.array_equal(_bits(got), _bits(g["kitti_%d" % k])), k
        assert np.array_equal(_bits(SR.ingest_ref(g["raw_%d" % k], [('affine', g["v2c"][:3])])), _bits(got))
    chain = [('rotate', g["nus_r1"]), ('translate', g["nus_t1"]), ('rotate', g["nus_r2"]), ('translate', g["nus_t2"])]
    for k in (2, 3):
        assert np.array_equal(_bits(SR.ingest_ref(g["raw_%d" % k], chain)), _bits(g["nus_%d" % k])), k
    # no step: the first three columns, transposed, untouched
    assert np.array_equal(_bits(SR.ingest_ref(g["raw_3"])), _bits(g["raw_3"][:, :3].T))
    kept = []
    for j in range(3):
        scan, box, offset = g["kitti_%d" % int(g["scan_%d" % j])], g["box_%d" % j], float(g["offset_%d" % j])
        want = g["crop_%d" % j]
        assert np.array_equal(_bits(SR.preload_ref(scan, g["lo_%d" % j], g["hi_%d" % j])), _bits(want)), j
        lo, hi = SR.crop_bounds(box[0:3], box[3:6], box[6:10], offset)          # the store's bounds: box_math's corners
        assert np.array_equal(_bits(SR.preload_ref(scan, lo, hi)), _bits(want)), j
        kept.append(want.shape[1])
    assert kept[0] > 50 and kept[1] > 0 and kept[2] == 0 and [float(g["offset_%d" % j]) for j in range(3)] == [10.0, 2.0, 2.0]


def test_restatement_is_strict_and_keeps_the_order():
    pts = np.array([[0, 1, 2, 3, 4], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]], np.float32)
    got = SR.preload_ref(pts, [0.0, -1, -1], [4.0, 1, 1])
    assert got.tolist() == [[1, 2, 3], [0, 0, 0], [0, 0, 0]]


def test_abi_and_struct_mirrors_match_the_header(tmp_path):
    """ptt_scan_step / ptt_scan_job / ptt_preload_job: ctypes and numpy agree with what gcc makes of include/ptt_hip.h."""
    from ptt_amd import _lib, ops
    assert _lib.ABI_VERSION >= 34
    for name in ("ptt_scan_ingest_f32", "ptt_scan_preload_workspace", "ptt_scan_preload_f32"):
        assert name in _lib.EXPORTS, name
    vp, i = ctypes.c_void_p, ctypes.c_int
    assert _lib.PROTOTYPES["ptt_scan_ingest_f32"] == (i, [vp, i, i, vp])
    assert _lib.PROTOTYPES["ptt_scan_preload_workspace"] == (ctypes.c_size_t, [i, i])
    assert _lib.PROTOTYPES["ptt_scan_preload_f32"] == (i, [vp, i, i, vp, ctypes.c_size_t, vp])
    assert (_lib.PTT_SCAN_MAX_STEPS, _lib.SCAN_KINDS) == (4, {"rotate": 1, "translate": 2, "affine": 3})
    pairs = [("ptt_scan_step", _lib.ScanStep, ops.SCAN_STEP), ("ptt_scan_job", _lib.ScanJob, ops.SCAN_JOB),
             ("ptt_preload_job", _lib.PreloadJob, ops.PRELOAD_JOB)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ptt_hip.h"', 'int main(void) {']
    for cname, st, _ in pairs:
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, *_r in st._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines += ['return 0;', '}']
    src = tmp_path / "abi_probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "abi_probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    for cname, st, dt in pairs:
        assert int(got[cname]) == ctypes.sizeof(st) == dt.itemsize, cname
        for fname, *_r in st._fields_:
            assert int(got["%s.%s" % (cname, fname)]) == getattr(st, fname).offset == dt.fields[fname][1], (cname, fname)
    assert (ops.SCAN_STEP.itemsize, ops.SCAN_JOB.itemsize, ops.PRELOAD_JOB.itemsize) == (104, 456, 96)


def test_scan_steps_builds_the_records_and_refuses_the_rest():
    from ptt_amd import ops
    R, t = np.arange(9.0).reshape(3, 3), np.array([1.0, 2.0, 3.0])
    A4 = np.arange(16.0).reshape(4, 4)
    recs = ops.scan_steps([('rotate', R), ('translate', t), ('affine', A4), ('affine', A4[:3])])
    assert recs.dtype == ops.SCAN_STEP and recs['kind'].tolist() == [1, 2, 3, 3]
    assert recs['m'][0].tolist() == list(range(9)) + [0, 0, 0] and recs['m'][1].tolist() == [1, 2, 3] + [0] * 9
    assert recs['m'][2].tolist() == list(range(12)) == recs['m'][3].tolist()               # a 4x4: the top three rows
    assert len(ops.scan_steps(None)) == 0 and len(ops.scan_steps([])) == 0
    assert recs[2:3].tobytes() == ops.scan_steps([('affine', A4.tolist())]).tobytes()      # nested lists are arrays too
    bad = [[('rotate', R)] * 5, [('shear', R)], [('rotate', t)], [('translate', R)], [('affine', R)], [('affine', np.zeros((4, 3)))],
           [('rotate', R, R)], ['rotate'], [('rotate', np.full((3, 3), np.nan))], [('translate', [1.0, np.inf, 0.0])], [('rotate', "abc")],
           5, "rotate", [None]]
    for steps in bad:
        with pytest.raises(ValueError):
            ops.scan_steps(steps)


def _table(n=2):
    from ptt_amd import ops
    jobs = np.zeros(n, ops.SCAN_JOB)
    jobs['row_floats'], jobs['n_points'], jobs['ld'], jobs['n_steps'] = 4, 10, 16, 1
    jobs['steps']['kind'][:, 0] = 3
    return jobs


def test_scan_ingest_check_raises_every_refusal():
    from ptt_amd import ops
    ops.scan_ingest_check(_table(), 2, 10)                                                  # a good table passes
    jobs = _table()
    jobs['steps']['kind'][:, 1:] = 99                                                       # beyond n_steps: not looked at
    jobs['n_points'][1] = 0
    ops.scan_ingest_check(jobs, 2, 10)
    cases = [("row_floats", 2), ("row_floats", 17), ("n_steps", -1), ("n_steps", 5), ("n_points", -1), ("n_points", 11), ("ld", 9)]
    for field, value in cases:
        jobs = _table()
        jobs[field][1] = value
        with pytest.raises(ValueError, match=field):
            ops.scan_ingest_check(jobs, 2, 10)
    for kind in (0, 4, -1):
        jobs = _table()
        jobs['steps']['kind'][1, 0] = kind
        with pytest.raises(ValueError, match="kind"):
            ops.scan_ingest_check(jobs, 2, 10)
    for n_jobs, max_points in ((3, 10), (0, 10), (2, 0)):                                    # a short table, no job, no point
        with pytest.raises(ValueError):
            ops.scan_ingest_check(_table(), n_jobs, max_points)


def test_check_raw_refuses_what_is_not_a_raw_scan():
    import torch
    from ptt_amd.scene_store import check_raw
    dev = torch.device("cuda:0")                                                            # never touched: host inputs only
    ok = np.zeros((7, 4), np.float32)
    assert tuple(check_raw(ok, dev).shape) == (7, 4) and check_raw(ok, dev).data_ptr() == ok.ctypes.data
    assert tuple(check_raw(torch.zeros(0, 16), dev, max_points=0).shape) == (0, 16)
    bad = [ok.astype(np.float64), ok[0], ok[:, :3], ok[::2], np.asfortranarray(ok), np.zeros((7, 2), np.float32),
           np.zeros((7, 17), np.float32), list(ok), torch.zeros(7, 4, dtype=torch.float64), torch.zeros(4, 7).t(), torch.zeros(7)]
    for raw in bad:
        with pytest.raises(ValueError):
            check_raw(raw, dev)
    with pytest.raises(ValueError, match="capacity"):
        check_raw(ok, dev, max_points=6)


def test_scene_store_on_a_cpu_device_raises():
    from ptt_amd.scene_store import SceneStore
    with pytest.raises(RuntimeError, match="HIP device"):
        SceneStore("cpu")
