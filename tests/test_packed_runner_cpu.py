"""PackedPlan without a GPU: the schedule of PackedTrackletRunner from the tracklet lengths alone — every frame once and in order,
never more than `slots` alive, no idle slot while a tracklet waits, frame 1 in the admission step, the bound against the lockstep
runner's step count, the single migration of the drain, and the refusals."""
import numpy as np
import pytest


def L(a, b):
    return list(range(a, b))


LISTS = {
    "A": [1, 2, 4, 7, 3, 2, 9, 1, 5],
    "B": [6] * 7,                                   # all equal
    "C": [600] + L(2, 42),                          # one long tracklet and forty short ones
    "D": [5, 0, 3],                                 # fewer tracklets than (most) slot counts, one without frames
}
SLOTS = [1, 2, 3, 48]
ORDERS = ["input", "longest_first"]


def _plan(*args, **kw):
    from ptt_amd.packed_runner import PackedPlan
    return PackedPlan(*args, **kw)


def _lockstep_steps(lengths, slots):
    """TrackletRunner.run: groups of `slots` in input order, each max(length) - 1 steps."""
    return sum(max(max(lengths[g:g + slots]) - 1, 0) for g in range(0, len(lengths), slots))


def _replay(plan):
    """Walk the plan as a runner would and assert its invariants; -> per tracklet the (step, lane width) of every tracked frame."""
    lengths = plan.lengths
    waiting = list(plan.admission_order)
    assert sorted(waiting) == [t for t, n in enumerate(lengths) if n >= 2]          # lengths 0 and 1 take no slot
    holder, seen, migrations = {}, {t: [] for t in waiting}, 0
    for k, st in enumerate(plan.steps):
        if st.migrate is not None:
            migrations += 1
            held = {s: t for s, t in holder.items()}
            moved = {}
            for old, new, t in st.migrate:
                if old in held:                                  # a tracklet admitted in this very step has no wide slot yet
                    assert held.pop(old) == t
                moved[new] = t
            assert not held and len(moved) == len(st.migrate)    # nobody is left behind, no two share a drain slot
            holder = {new: t for new, t in moved.items() if t not in [a[1] for a in st.admit]}
        assert st.width == (plan.slots if plan.migration_step is None or k < plan.migration_step else plan.drain_slots)
        for s, t in st.admit:
            assert 0 <= s < st.width and s not in holder and t == waiting.pop(0)     # a free slot, the queue's order
            holder[s] = t
        assert len(holder) <= st.width
        assert len(holder) == st.width or not waiting            # no free slot while the queue is non-empty
        assert [(s, t) for s, t, _ in st.track] == sorted(holder.items())             # every alive tracklet is tracked
        for s, t, i in st.track:
            assert i == len(seen[t]) + 1                         # in frame order, frame 1 in the admission step
            assert (i == 1) == ((s, t) in st.admit)
            seen[t].append((k, st.width))
            if i + 1 == lengths[t]:
                del holder[s]                                    # free from the next step on
    assert not holder and not waiting
    for t, rows in seen.items():
        assert len(rows) == lengths[t] - 1                       # every frame >= 1 exactly once
        assert [k for k, _ in rows] == list(range(rows[0][0], rows[0][0] + len(rows)))     # a slot is held without a gap
    assert migrations == (0 if plan.migration_step is None else 1)
    return seen


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("slots", SLOTS)
@pytest.mark.parametrize("name", sorted(LISTS))
def test_every_frame_once_in_order_and_no_idle_slot(name, slots, order):
    lengths = LISTS[name]
    plan = _plan(lengths, slots, order)
    _replay(plan)
    live = sum(n - 1 for n in lengths if n >= 2)
    assert plan.n_steps == len(plan.steps) and plan.live_slot_steps == live
    assert plan.slot_steps == plan.n_steps * slots and plan.admissions == sum(n >= 2 for n in lengths)
    assert plan.migration_step is None and plan.migrated == 0
    assert plan.n_steps >= max(-(-live // slots), max(lengths) - 1)                  # what no schedule can beat
    want = [t for t, n in enumerate(lengths) if n >= 2]
    if order == "longest_first":
        want.sort(key=lambda t: (-lengths[t], t))                                    # ties by input index
    assert plan.admission_order == want


@pytest.mark.parametrize("slots", SLOTS)
@pytest.mark.parametrize("name", sorted(LISTS))
def test_input_order_never_takes_more_steps_than_lockstep(name, slots):
    """Greedy refill starts every tracklet no later than its lockstep group would."""
    lengths = LISTS[name]
    assert _plan(lengths, slots, "input").n_steps <= _lockstep_steps(lengths, slots)


def test_list_c_takes_fewer_steps_than_lockstep_wherever_any_schedule_can():
    """List C holds 41 tracklets. At 48 slots they are ONE lockstep group of max(length) - 1 = 599 steps, which no schedule can
    beat (the 600-frame tracklet is strictly sequential): there packed meets that bound exactly. Wherever lockstep needs more
    than one group and a slot is left beside the long tracklet's — 2 or 3 slots — packed is strictly smaller, and at 3 slots it is
    the 599 steps again: the long tracklet no longer holds up its group. At one slot every schedule is the same."""
    lengths = LISTS["C"]
    assert _lockstep_steps(lengths, 48) == 599
    assert _plan(lengths, 48, "input").n_steps == 599
    assert _plan(lengths, 3, "input").n_steps == 599 < _lockstep_steps(lengths, 3)
    assert _plan(lengths, 2, "input").n_steps < _lockstep_steps(lengths, 2)
    assert _plan(lengths, 1, "input").n_steps == sum(n - 1 for n in lengths) == _lockstep_steps(lengths, 1)     # one slot: no choice


def test_fewer_steps_than_lockstep_at_48_slots_once_there_are_two_groups():
    """List C and its reverse: two lockstep groups at 48 slots, each held up by its 600-frame tracklet. Packed in input order
    admits the second long tracklet as soon as the short ones before it have passed through."""
    lengths = LISTS["C"] + LISTS["C"][::-1]
    assert _lockstep_steps(lengths, 48) == 2 * 599
    assert _plan(lengths, 48, "input").n_steps < 599 + 41
    assert _plan(lengths, 48, "longest_first").n_steps == 599


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("slots,drain", [(1, 1), (2, 1), (2, 2), (3, 1), (3, 2), (48, 8), (48, 48)])
@pytest.mark.parametrize("name", sorted(LISTS))
def test_drain_migrates_once_at_the_first_step_it_can(name, slots, drain, order):
    lengths = LISTS[name]
    plan = _plan(lengths, slots, order, drain_slots=drain)
    seen = _replay(plan)
    wide = _plan(lengths, slots, order)
    m = plan.migration_step
    if plan.admissions == 0:
        assert m is None
        return
    # the schedule is the wide plan's: same steps, same frames per step — only the slots and the width change at the migration
    assert plan.n_steps == wide.n_steps
    for a, b in zip(plan.steps, wide.steps):
        assert sorted((t, i) for _, t, i in a.track) == sorted((t, i) for _, t, i in b.track)
    # the first step after whose refill nothing waits and at most `drain` tracklets are alive
    admitted = np.cumsum([len(st.admit) for st in wide.steps])
    first = [k for k, st in enumerate(wide.steps) if admitted[k] == wide.admissions and len(st.track) <= drain][0]
    assert m == first
    st = plan.steps[m]
    assert plan.migrated == len(st.migrate) == len(st.track) >= 1
    assert [new for _, new, _ in st.migrate] == list(range(plan.migrated))            # packed from slot 0, in slot order
    assert [old for old, _, _ in st.migrate] == sorted(old for old, _, _ in st.migrate)
    assert sorted(t for _, _, t in st.migrate) == sorted(t for _, t, _ in st.track)
    for t, rows in seen.items():                                                     # wide before, narrow from the migration on
        assert all(w == (slots if k < m else drain) for k, w in rows)
    assert plan.slot_steps == m * slots + (plan.n_steps - m) * drain


def test_list_a_at_two_slots_step_by_step():
    """The GPU test's schedule, written out: a refill while the neighbour continues, two admissions in one step, an empty slot in
    the tail."""
    plan = _plan([1, 2, 4, 7, 3], 2, "input")
    assert [(st.admit, st.track) for st in plan.steps] == [
        ([(0, 1), (1, 2)], [(0, 1, 1), (1, 2, 1)]),
        ([(0, 3)], [(0, 3, 1), (1, 2, 2)]),
        ([], [(0, 3, 2), (1, 2, 3)]),
        ([(1, 4)], [(0, 3, 3), (1, 4, 1)]),
        ([], [(0, 3, 4), (1, 4, 2)]),
        ([], [(0, 3, 5)]),
        ([], [(0, 3, 6)])]
    plan = _plan([1, 2, 4, 7, 3], 2, "longest_first")
    assert plan.admission_order == [3, 2, 4, 1] and plan.n_steps == 6
    assert plan.steps[3].admit == [(1, 4)] and plan.steps[5].admit == [(1, 1)] and plan.steps[5].track == [(0, 3, 6), (1, 1, 1)]


def test_refusals():
    from ptt_amd.packed_runner import PackedTrackletRunner
    for kw in (dict(slots=0), dict(slots=-1), dict(slots=2, drain_slots=0), dict(slots=2, drain_slots=3), dict(slots=2, order="shortest"),
               dict(slots=2, order=None)):
        with pytest.raises(ValueError):
            _plan([3, 4], **kw)
        with pytest.raises(ValueError):                      # ... and before any device is touched
            PackedTrackletRunner(None, "cpu", **kw)
    with pytest.raises(ValueError):
        _plan([3, -1], 2)
    with pytest.raises(ValueError, match="out of scope"):
        PackedTrackletRunner(None, "cpu", slots=2, shape_aggregation="all")
    with pytest.raises(ValueError, match="out of scope"):
        PackedTrackletRunner(None, "cpu", slots=2, shape_aggregation="something_else")     # parsed as the reference parses it
    with pytest.raises(ValueError, match="reference_BB"):
        PackedTrackletRunner(None, "cpu", slots=2, ref_box="next_gt")
    assert _plan([], 3).n_steps == 0 and _plan([1, 0, 1], 3, drain_slots=2).migration_step is None
