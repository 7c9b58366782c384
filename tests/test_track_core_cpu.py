"""The host-side table builders of ptt_amd.track_core as pure numpy, over made-up base addresses: no GPU."""
import numpy as np
import pytest

from ptt_amd import ops
from ptt_amd import track_core as tc

CROP_OUT, COUNTS, SEARCH, TEMPLATE, INFO = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000
CAP, S, T = 37, 16, 8


@pytest.mark.parametrize("n", [1, 3])
def test_slot_pointers_are_the_closed_form(n):
    out_ptr, cnt_ptr = tc.slot_pointers(CROP_OUT, COUNTS, n, CAP)
    assert out_ptr.dtype == cnt_ptr.dtype == np.uint64 and out_ptr.shape == cnt_ptr.shape == (n, 3)
    for w in range(n):
        for slot in range(3):                                   # a (n, 3, cap, 3) float32 buffer, a (n, 3) int32 one
            assert out_ptr[w, slot] == CROP_OUT + ((w * 3 + slot) * CAP * 3) * 4
            assert cnt_ptr[w, slot] == COUNTS + (w * 3 + slot) * 4


@pytest.mark.parametrize("shape,slots", [("firstandprevious", (1, 2)), ("first", (1,)), ("previous", (2,)), ("all", ())])
def test_resample_table(shape, slots):
    W = 2
    out_ptr, cnt_ptr = tc.slot_pointers(CROP_OUT, COUNTS, W, CAP)
    rj = tc.resample_table(shape, out_ptr, cnt_ptr, CAP, SEARCH, TEMPLATE, INFO, S, T)
    assert rj.dtype == ops.REGULARIZE_JOB and rj.shape == (2 * W,)
    for w in range(W):
        s, t = rj[2 * w], rj[2 * w + 1]
        # the search cloud: slot 0 alone
        assert s['n_seg'] == 1 and s['input_size'] == S
        assert (s['seg'][0], s['seg_count'][0], s['seg_capacity'][0]) == (out_ptr[w, 0], cnt_ptr[w, 0], CAP)
        assert s['out'] == SEARCH + w * S * 3 * 4 and s['info'] == INFO + w * 16
        # the template: the shape's slots in get_model's order; `all` has one segment the runner points at its store
        assert t['n_seg'] == max(1, len(slots)) and t['input_size'] == T
        for k, slot in enumerate(slots):
            assert (t['seg'][k], t['seg_count'][k], t['seg_capacity'][k]) == (out_ptr[w, slot], cnt_ptr[w, slot], CAP)
        assert not t['seg'][len(slots):].any() and not t['seg_count'][len(slots):].any() and not s['seg'][1:].any()
        assert t['out'] == TEMPLATE + w * T * 3 * 4 and t['info'] == INFO + w * 16 + 8


def test_main_crop_fields_and_admission_fields():
    W, admissions = 3, 3
    out_ptr, cnt_ptr = tc.slot_pointers(CROP_OUT, COUNTS, W, CAP)
    jobs = np.zeros(2 * W + admissions, ops.CROP_JOB)
    jobs['n_points'], jobs['append'], jobs['points'] = 5, 1, 99       # left over from an earlier run: cleared
    tc.main_crop_fields(jobs, out_ptr, cnt_ptr, CAP)
    assert (jobs['capacity'] == CAP).all() and not jobs['append'].any() and not jobs['n_points'].any() and not jobs['points'].any()
    main = jobs[:2 * W]
    assert np.array_equal(main['out'][0::2], out_ptr[:, 0]) and np.array_equal(main['count'][0::2], cnt_ptr[:, 0])      # search -> 0
    assert np.array_equal(main['out'][1::2], out_ptr[:, 2]) and np.array_equal(main['count'][1::2], cnt_ptr[:, 2])      # previous -> 2
    assert not jobs['out'][2 * W:].any() and not jobs['count'][2 * W:].any()

    tail = jobs[2 * W:]
    tail['n_points'] = 7
    slots = np.array([2, 0])                                         # not contiguous, not sorted
    aj = tc.admission_fields(tail, slots, out_ptr, cnt_ptr, CAP)
    assert len(aj) == 2 and np.shares_memory(aj, jobs)
    assert np.array_equal(aj['out'], out_ptr[slots, 1]) and np.array_equal(aj['count'], cnt_ptr[slots, 1])
    assert (aj['capacity'] == CAP).all() and not aj['n_points'].any() and not aj['append'].any()
    assert tail['n_points'][2] == 7 and tail['out'][2] == 0          # the entry behind them is not touched
    assert np.array_equal(main['out'][0::2], out_ptr[:, 0])
    # into a strided table: the lockstep runner's frame 0 takes the even main entries
    even = tc.admission_fields(jobs[0:2 * W:2], np.arange(W), out_ptr, cnt_ptr, CAP)
    assert np.array_equal(jobs['out'][0:2 * W:2], out_ptr[:, 1]) and np.array_equal(jobs['out'][1:2 * W:2], out_ptr[:, 2]) and len(even) == W


def test_unit_boxes():
    for n in (0, 1, 4, (3, 2)):
        boxes = tc.unit_boxes(n)
        assert boxes.dtype == ops.TRACK_BOX and boxes.shape == (n if isinstance(n, tuple) else (n,))
        assert (boxes['wlh'] == 1.0).all() and not boxes['center'].any()
        assert (boxes['quat'][..., 0] == 1.0).all() and not boxes['quat'][..., 1:].any()
