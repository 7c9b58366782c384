"""OnlineTracker without a GPU: the C ABI of the chunked crop as the header declares it and the binding reads it, the host-only
slot bookkeeping, and the refusals that happen before any device is touched."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_chunked_crop_and_the_binding_carries_it():
    from ptt_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "ptt_hip.h")).read()
    assert re.search(r"\bint\s+ptt_crop_scan_f32\s*\(\s*const\s+ptt_crop_job\s*\*\s*jobs_device\s*,\s*int\s+n_jobs\s*,\s*int\s+max_points\s*,"
                     r"\s*void\s*\*\s*ws\s*,\s*size_t\s+ws_bytes\s*,\s*ptt_stream_t\s+stream\s*\)\s*;", header)
    assert re.search(r"\bsize_t\s+ptt_crop_scan_workspace\s*\(\s*int\s+n_jobs\s*,\s*int\s+max_points\s*\)\s*;", header)
    assert "ptt_crop_scan_f32" in _lib.EXPORTS and "ptt_crop_scan_workspace" in _lib.EXPORTS
    vp, i = ctypes.c_void_p, ctypes.c_int
    assert _lib.PROTOTYPES["ptt_crop_scan_f32"] == (i, [vp, i, i, vp, ctypes.c_size_t, vp])
    assert _lib.PROTOTYPES["ptt_crop_scan_workspace"] == (ctypes.c_size_t, [i, i])
    assert _lib.ABI_VERSION >= 30
    assert ops.SCAN_CROP_CHUNK == _lib.DEFINES["PTT_SCAN_CROP_CHUNK"] and ops.SCAN_CROP_CHUNK % 64 == 0


def test_workspace_query_is_one_word_per_job_and_chunk():
    """A host-only entry point: no device needed."""
    from ptt_amd import ops
    C = ops.SCAN_CROP_CHUNK
    assert ops.crop_scan_workspace(3, 2 * C + 1) == 4 * 3 * 3
    assert ops.crop_scan_workspace(1, C) == 4 and ops.crop_scan_workspace(2, 0) == 8        # an empty cloud still has one chunk
    assert ops.crop_scan_workspace(0, 100) == 0


def test_host_table_check_refuses_labels_appends_and_long_clouds():
    from ptt_amd import ops
    jobs = np.zeros(3, ops.CROP_JOB)
    jobs['n_points'] = [5, 0, 9]
    ops.crop_scan_check(jobs, 3, 9)
    with pytest.raises(ValueError, match="max_points"):
        ops.crop_scan_check(jobs, 3, 8)
    ops.crop_scan_check(jobs, 2, 5)                                # only the first n_jobs entries count
    with pytest.raises(ValueError):
        ops.crop_scan_check(jobs, 4, 9)                            # more jobs than the table holds
    bad = jobs.copy()
    bad['label_out'][2] = 4096
    with pytest.raises(ValueError, match="label_out"):
        ops.crop_scan_check(bad, 3, 9)
    bad = jobs.copy()
    bad['append'][0] = 1
    with pytest.raises(ValueError, match="append"):
        ops.crop_scan_check(bad, 3, 9)


def test_slot_table_add_drop_reuse_full_and_order():
    from ptt_amd.online_tracker import SlotTable
    t = SlotTable(3)
    assert t.ids == [] and t.free() == [0, 1, 2]
    t.commit(t.plan(add=["a", "b"]))
    assert t.ids == ["a", "b"] and t.slot_of == {"a": 0, "b": 1} and t.free() == [2]
    t.commit(t.plan(add=["c"]))
    assert t.ids == ["a", "b", "c"] and t.free() == []
    # full, duplicate, unknown: ValueError, nothing changes
    before = dict(t.slot_of)
    for kw in (dict(add=["d"]), dict(add=["a"]), dict(drop=["z"]), dict(add=["d", "d"], drop=["a", "b"]), dict(drop=["a", "a"]),
               dict(add=["d", "e"], drop=["b"])):
        with pytest.raises(ValueError):
            t.plan(**kw)
        assert t.slot_of == before
    # plan() alone changes nothing
    plan = t.plan(add=["d"], drop=["b"])
    assert t.slot_of == before
    t.commit(plan)
    assert t.slot_of == {"a": 0, "c": 2, "d": 1}                   # the freed slot is reused
    assert t.ids == ["a", "c", "d"]                                # in the order they were added
    # an id dropped and added again in one step: allowed, it takes the lowest free slot
    t.commit(t.plan(add=["a"], drop=["a", "c"]))
    assert t.slot_of == {"d": 1, "a": 0} and t.ids == ["d", "a"] and t.free() == [2]
    with pytest.raises(ValueError):
        SlotTable(0)


def test_shape_aggregation_all_is_refused_before_any_device_work():
    from ptt_amd.online_tracker import OnlineTracker
    with pytest.raises(ValueError, match="out of scope"):
        OnlineTracker(None, "cpu", shape_aggregation="all")
    with pytest.raises(ValueError, match="out of scope"):
        OnlineTracker(None, "cpu", shape_aggregation="something_else")       # parsed as the reference parses it: `all`
