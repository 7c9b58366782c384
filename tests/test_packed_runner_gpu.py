"""PackedTrackletRunner on the GPU against TrackletRunner — the oracle — bit for bit: every tracklet's rows (centre, wlh,
quaternion, score) equal what TrackletRunner(tracker, dev, batch=slots) gives for that tracklet ALONE (the same width on both
sides: the forward's kernel choice depends on the batch width, a frame's result does not depend on its batch-mates or its slot).

Five synthetic tracklets of lengths [1, 2, 4, 7, 3]: the smallest input that gives, at 2 and 3 slots, a refill while a neighbour
continues, two admissions in one step, a single-frame tracklet and an empty slot in the tail (the schedule at 2 slots is written
out in test_packed_runner_cpu.py)."""
import numpy as np
import pytest

from ptt_amd import synth
from tests.test_online_tracker_gpu import _make_tracker, _tracker

pytestmark = pytest.mark.gpu
LENGTHS = [1, 2, 4, 7, 3]
_cache = {}


def _tracklets():
    if "tracklets" not in _cache:
        _cache["tracklets"] = [synth.tracklet(400 + k, n) for k, n in enumerate(LENGTHS)]
    return _cache["tracklets"]


def _oracle_rows(tracker, dev, slots, **modes):
    from ptt_amd.tracklet_runner import TrackletRunner
    runner = TrackletRunner(tracker, dev, batch=slots, **modes)
    out = [runner.run([tr])[0] for tr in _tracklets()]
    assert [len(rows) for rows in out] == LENGTHS
    return out


def _expected(dev, slots, shape="firstandprevious", ref_box="previous_result"):
    """The runner's rows of every tracklet alone — computed once per (slots, modes) and shared, never modified."""
    key = (slots, shape, ref_box)
    if key not in _cache:
        _cache[key] = _oracle_rows(_tracker(dev), dev, slots, shape_aggregation=shape, ref_box=ref_box)
    return _cache[key]


def _packed(dev, slots, tracker=None, **kw):
    from ptt_amd.packed_runner import PackedTrackletRunner
    return PackedTrackletRunner(_tracker(dev) if tracker is None else tracker, dev, slots=slots, **kw)


def _same(got, want, what):
    assert len(got) == len(want), what                       # row 0: (centre, wlh, quaternion), later rows with the score
    for g, w, name in zip(got, want, ("centre", "wlh", "quaternion")):
        np.testing.assert_array_equal(g, w, err_msg="%s %s" % (what, name))
    assert len(want) == 3 or got[3] == want[3], (what, got[3], want[3])


def _all_same(got, want, what, upto=None):
    """Rows [0, upto[t]) of every tracklet t (None: all rows) are the oracle's; -> how many tracked rows moved off box 0."""
    assert [len(rows) for rows in got] == LENGTHS
    moved = 0
    for t, (g_rows, w_rows) in enumerate(zip(got, want)):
        n = len(w_rows) if upto is None else upto[t]
        for i in range(n):
            _same(g_rows[i], w_rows[i], "%s: tracklet %d frame %d" % (what, t, i))
            moved += int(i > 0 and float(np.abs(g_rows[i][0] - w_rows[0][0]).max()) > 1e-6)
    return moved


@pytest.mark.parametrize("shape", ["firstandprevious", "first", "previous"])
@pytest.mark.parametrize("order", ["input", "longest_first"])
@pytest.mark.parametrize("slots", [2, 3])
def test_rows_equal_the_runner(dev, slots, order, shape):
    from ptt_amd.packed_runner import PackedPlan
    pr = _packed(dev, slots, order=order, shape_aggregation=shape)
    got = pr.run(_tracklets())
    assert _all_same(got, _expected(dev, slots, shape), "slots %d %s %s" % (slots, order, shape)) > 0
    plan = PackedPlan(LENGTHS, slots, order)
    assert pr.stats == dict(steps=plan.n_steps, slot_steps=plan.n_steps * slots, live_slot_steps=sum(n - 1 for n in LENGTHS if n > 1),
                            admissions=4, migrated=0)
    assert plan.n_steps < sum(max(LENGTHS[g:g + slots]) - 1 for g in range(0, len(LENGTHS), slots))       # lockstep: 9 steps
    assert any(len(st.admit) >= 2 for st in plan.steps) and any(len(st.admit) == 1 and len(st.track) > 1 for st in plan.steps)
    # an empty slot in the tail — but for 2 slots filled longest first, which keeps both busy for all of its 6 steps
    assert any(len(st.track) < slots for st in plan.steps) == ((slots, order) != (2, "longest_first"))
    assert all(c is None for c in pr.clouds)                 # every uploaded tracklet was released when it finished


@pytest.mark.parametrize("ref_box", ["previous_gt", "current_gt"])
def test_ref_box_modes_equal_the_runner(dev, ref_box):
    got = _packed(dev, 2, ref_box=ref_box).run(_tracklets())
    assert _all_same(got, _expected(dev, 2, ref_box=ref_box), ref_box) > 0


@pytest.mark.parametrize("order", ["input", "longest_first"])
def test_migration_to_a_core_of_the_same_width_keeps_the_bits(dev, order):
    """drain_slots == slots: two cores of equal width, so the move itself (first-frame crop and count device to device, box and
    generator position on the host) must not change a bit. In input order the last tracklet is admitted in the step of the
    migration; longest first, a tracklet that continues and one that starts move together."""
    pr = _packed(dev, 2, order=order, drain_slots=2)
    got = pr.run(_tracklets())
    assert pr.stats["migrated"] >= 1 and pr.plan.migration_step is not None
    assert pr.stats["steps"] == pr.plan.n_steps == len(pr.plan.steps)
    assert _all_same(got, _expected(dev, 2), "drain 2 of 2, %s" % order) > 0


@pytest.mark.parametrize("order", ["input", "longest_first"])
def test_narrow_drain_keeps_the_bits_up_to_the_migration(dev, order):
    """slots = 3, drain_slots = 1: the 7-frame tracklet ends alone on a core of width 1. Its rows before the migration frame, and
    every row of the tracklets that ended on the wide core, are the batch = 3 runner's; the later rows come from a model of another
    width and are only required to be there and finite."""
    pr = _packed(dev, 3, order=order, drain_slots=1)
    got = pr.run(_tracklets())
    plan = pr.plan
    assert pr.stats["migrated"] == 1 and plan.steps[plan.migration_step].width == 1
    upto = list(LENGTHS)
    for _, t, i in plan.steps[plan.migration_step].track:
        upto[t] = i                                          # frame i is the first one tracked on the narrow core
    assert upto == [1, 2, 4, 4, 3]
    want = _expected(dev, 3)
    assert _all_same(got, want, "drain 1 of 3, %s" % order, upto=upto) > 0
    for t, rows in enumerate(got):
        _same(rows[0], want[t][0], "tracklet %d: row 0 is the ground-truth box" % t)
        assert len(rows[0]) == 3 and all(len(r) == 4 for r in rows[1:])
        assert all(np.isfinite(np.concatenate([np.ravel(v) for v in r])).all() for r in rows)


def test_a_second_run_and_new_weights(dev):
    """No state leaks from one run into the next; after load_state_dict the next run follows the new weights (a new capture)."""
    tracker = _make_tracker(dev, seed=2)                     # its own object: its weights are overwritten below
    pr = _packed(dev, 2, tracker=tracker)
    want = _expected(dev, 2)
    _all_same(pr.run(_tracklets()), want, "first run")
    _all_same(pr.run(_tracklets()[::-1])[::-1], want, "second run, tracklets reversed")
    graph = pr.core.graph
    new = _make_tracker(dev, seed=3)
    tracker.load_state_dict(new.state_dict())
    got = pr.run(_tracklets())
    assert pr.core.graph is not graph and pr.core.graph.captures == 1
    _all_same(got, _oracle_rows(new, dev, 2), "new weights")
    assert not np.array_equal(got[3][-1][0], want[3][-1][0])                         # ... and not what the old weights give


def test_device_clouds_are_used_in_place_and_bad_tracklets_are_refused(dev):
    import torch
    trs = _tracklets()
    on_dev = [([torch.from_numpy(c).to(dev) for c in clouds], boxes) for clouds, boxes in trs]
    pr = _packed(dev, 3)
    _all_same(pr.run(on_dev), _expected(dev, 3), "device tensors")
    stats = dict(pr.stats)
    with pytest.raises(ValueError, match="clouds and"):
        pr.run(trs[:2] + [(trs[2][0], trs[2][1][:-1])])
    assert pr.stats == stats
