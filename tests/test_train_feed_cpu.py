"""N5 without a device: the generator (the library's host entry point: the function the kernel compiles), the index plan and the
host half of ptt_amd.train_feed (TrainBatchPlan: order, shards, offsets, reg_label) against the reference (fixture G21,
tests/golden/make_golden_g21.py) and against the restatement the GPU tests compare the kernel with (tests/train_feed_ref.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import train_feed_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

PHILOX_KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
              ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
              ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.fixture(scope="module")
def g21():
    g = np.load(os.path.join(GOLD, "G21_train_items.npz"))
    trks = []
    for t in range(int(g["n_tracklets"])):
        n = int(g["n_frames_%d" % t])
        boxes = [g["box_%d_%d" % (t, i)] for i in range(n)]
        trks.append(([g["cloud_%d_%d" % (t, i)] for i in range(n)], [(b[0:3], b[3:6], b[6:10]) for b in boxes]))
    return g, trks


@pytest.mark.parametrize("counter,key,expect", PHILOX_KAT)
def test_philox_known_answers(counter, key, expect):
    """The restatement's numpy Philox4x32-10 and the library's (the function the kernel compiles, called on the host)."""
    from ptt_amd import ops
    assert tuple(int(v) for v in R.philox4x32_10(np.array(counter), np.array(key))) == expect
    assert tuple(int(v) for v in ops.philox4x32_10(counter, key)) == expect


def test_philox_library_equals_restatement_on_the_counters_the_kernel_forms():
    from ptt_amd import ops
    rs = np.random.RandomState(5)
    for _ in range(32):
        ctr = [int(rs.randint(0, 256)), int(rs.randint(0, 1 << 31)), int(rs.randint(0, 2)), int(rs.randint(0, 100))]
        key = [int(v) for v in rs.randint(0, 1 << 32, 2, dtype=np.uint64)]
        assert np.array_equal(ops.philox4x32_10(ctr, key), R.philox4x32_10(np.array(ctr), np.array(key)))


def test_restatement_and_host_plan_equal_the_reference_bitwise(g21):
    """Offsets as used, search crop, labels, reg_label, template and validity of every dataset index of G21: the restatement's, and
    the offsets and reg_label (float32, as the kernel hands it on) TrainBatchPlan.plan forms for the same indices."""
    from ptt_amd.train_feed import TrainBatchPlan
    g, trks = g21
    s = R.settings(candidates_per_frame=int(g["candidates_per_frame"]))
    seed, epoch = int(g["seed"]), int(g["epoch"])
    assert R.length(trks, s) == int(g["len"])
    plan = TrainBatchPlan(trks, batch_size=8, spare=4, seed=seed, shuffle=False)
    assert plan.length == int(g["len"]) and len(plan) == 3
    plans = [plan.plan(epoch, b) for b in range(3)]
    seen_invalid = 0
    for j in range(int(g["len"])):
        c = R.candidate(trks, s, seed, epoch, j)
        p, b = plans[j // 8], j % 8
        assert p['index'][b] == j
        assert np.array_equal(c['search_offset'], g["search_offset_%d" % j]), j
        assert np.array_equal(p['search_offset'][b], g["search_offset_%d" % j]), j
        assert np.array_equal(c['search'], g["search_%d" % j].T), j
        assert np.array_equal(c['label'], g["label_%d" % j]), j
        assert np.array_equal(c['reg'], g["reg_%d" % j]), j
        assert np.array_equal(p['reg_label'][b].astype(np.float32), g["reg_%d" % j].astype(np.float32)), j
        assert c['valid'] == bool(g["valid_%d" % j]), j
        if c['valid']:
            assert np.array_equal(c['template_offset'], g["template_offset_%d" % j]), j
            assert np.array_equal(p['template_offset'][b], g["template_offset_%d" % j]), j
            assert np.array_equal(c['template'], g["template_%d" % j].T), j
        seen_invalid += not c['valid']
    assert 0 < seen_invalid < int(g["len"])


@pytest.mark.parametrize("interval", [1, 2])
def test_index_plan_is_the_reference_arithmetic(g21, interval):
    """len, get_anno_index, get_aug_index and the frame map of the reference (recorded in G21 for both intervals) against
    train_feed.dataset_length / locate, a TrainBatchPlan built with that interval, and the restatement."""
    from ptt_amd import train_feed
    g, trks = g21
    n, fm = int(g["len_interval_%d" % interval]), g["frame_map"]
    anno_ref, aug_ref = g["anno_interval_%d" % interval], g["aug_interval_%d" % interval]
    assert train_feed.dataset_length(len(fm), 4, interval) == n
    anno, aug = train_feed.locate(np.arange(n), 4, interval)
    assert np.array_equal(anno, anno_ref) and np.array_equal(aug, aug_ref)
    plan = train_feed.TrainBatchPlan(trks, batch_size=4, spare=2, sampled_interval=interval, shuffle=False, seed=3)
    assert plan.length == n and len(plan) == n // 4
    assert np.array_equal(np.stack([plan.tracklet_of, plan.frame_of], 1), fm)
    for b in range(len(plan)):
        p = plan.plan(0, b)
        idx = p['index']
        assert idx[:4].tolist() == list(range(4 * b, 4 * b + 4)) and idx.min() >= 0 and idx.max() < n
        assert np.array_equal(p['anno'], anno_ref[idx]) and np.array_equal(p['aug'], aug_ref[idx])
        assert np.array_equal(np.stack([p['tracklet'], p['frame']], 1), fm[anno_ref[idx]])
        assert not p['search_offset'][p['aug'] == 0].any() and p['search_offset'][p['aug'] != 0].all()
    s = R.settings(candidates_per_frame=4, sampled_interval=interval)
    assert R.length(trks, s) == n and [tuple(r) for r in fm] == R.frame_map(trks)
    for j in range(n):
        t, i, a = R.locate(trks, s, j)
        assert (t, i) == tuple(fm[int(anno_ref[j])]) and a == int(aug_ref[j])


def test_shards_partition_the_epoch_permutation(g21):
    """world = 1, 2, 3 (24 = 2 * 3 * 4 samples divide by each): the ranks' orders interleave to the epoch's permutation, which is the
    restatement's; another epoch gives another order; without shuffle it is the identity."""
    from ptt_amd.train_feed import TrainBatchPlan
    _, trks = g21
    mk = lambda **kw: TrainBatchPlan(trks, batch_size=4, spare=2, seed=7, **kw)
    full = mk()._order(2)
    assert sorted(full.tolist()) == list(range(24)) and np.array_equal(full, R.order(trks, R.settings(), 7, 2))
    for world in (1, 2, 3):
        parts = [mk(rank=rank, world=world) for rank in range(world)]
        assert [len(p) for p in parts] == [24 // world // 4] * world
        orders = [p._order(2) for p in parts]
        for rank, o in enumerate(orders):
            assert np.array_equal(o, R.order(trks, R.settings(rank=rank, world=world), 7, 2))
        assert np.array_equal(np.stack(orders, 1).reshape(-1), full)       # rank r takes every world-th index starting at r
        prim = np.concatenate([p.plan(2, b)['index'][:4] for p in parts for b in range(len(p))])
        assert sorted(prim.tolist()) == list(range(24))
    assert not np.array_equal(mk()._order(3), full)
    assert np.array_equal(mk(shuffle=False)._order(2), np.arange(24))


def test_batch_indices_and_drop_last(g21):
    """The plan's primaries and spares are the restatement's; drop_last=False adds a last batch that wraps to the rank's first
    indices."""
    from ptt_amd.train_feed import TrainBatchPlan
    _, trks = g21
    s = R.settings(batch_size=5, spare=3)
    plan = TrainBatchPlan(trks, batch_size=5, spare=3, seed=9)
    assert len(plan) == 4                                      # 24 // 5
    for b in range(4):
        assert np.array_equal(plan.plan(1, b)['index'], R.batch_indices(trks, s, 9, 1, b))
    with pytest.raises(IndexError):
        plan.plan(1, 4)
    keep = TrainBatchPlan(trks, batch_size=5, spare=3, seed=9, drop_last=False)
    assert len(keep) == 5
    order = keep._order(1)
    assert np.array_equal(order, plan._order(1))
    assert keep.plan(1, 4)['index'][:5].tolist() == order[20:24].tolist() + order[:1].tolist()
    assert np.array_equal(keep.plan(1, 2)['index'], plan.plan(1, 2)['index'])


def test_from_config_reads_the_data_config(g21):
    from ptt_amd.config import EasyDict
    from ptt_amd.train_feed import TrainBatchPlan
    _, trks = g21
    cfg = EasyDict(dict(USE_Z_AXIS=False, NUM_CANDIDATES_PERFRAME=2, SEARCH_INPUT_SIZE=256, TEMPLATE_INPUT_SIZE=128, SEARCH_BB_OFFSET=0.1,
                        SEARCH_BB_SCALE=1.5, MODEL_BB_OFFSET=0.2, MODEL_BB_SCALE=1.1, REFINE_BOX_SIZE=False, SAMPLED_INTERVAL=2))
    p = TrainBatchPlan.from_config(trks, cfg, 3, seed=4)
    assert (p.B, p.S, p.T, p.cpf, p.interval, p.use_z, p.refine_box, p.seed) == (3, 256, 128, 2, 2, False, False, 4)
    assert (p.search_offset, p.search_scale, p.model_offset, p.model_scale) == (0.1, 1.5, 0.2, 1.1)
    assert p.length == 6 * 2 // 2 and p.spare == 4
    del cfg['REFINE_BOX_SIZE']                                  # p2b.yaml has no such key: the reference's default is True
    assert TrainBatchPlan.from_config(trks, cfg, 3).refine_box is True
    assert TrainBatchPlan.from_config(trks, {}, 3, spare=1).C == 4 and TrainBatchPlan.from_config(trks, {}, 3).S == 1024
    # the label box follows REFINE_BOX_SIZE (crop_center_pc :307-309): scaled and grown with the search area, or the box itself
    a = TrainBatchPlan.from_config(trks, dict(SEARCH_BB_OFFSET=0.3, SEARCH_BB_SCALE=1.25), 3, shuffle=False).plan(0, 0)['_jobs']
    b = TrainBatchPlan.from_config(trks, dict(SEARCH_BB_OFFSET=0.3, SEARCH_BB_SCALE=1.25, REFINE_BOX_SIZE=False), 3, shuffle=False).plan(0, 0)['_jobs']
    assert np.array_equal(a['lo2'][:, 0], b['lo2'][:, 0]) and (a['hi2'][:, 3] > b['hi2'][:, 3]).all()


def _library_indices(n, size, index, which, epoch, seed):
    """The kernel's draws formed with the library's Philox (ops.philox4x32_10): word i & 3 of block i >> 2, (word * n) >> 32."""
    from ptt_amd import ops
    key = [seed & 0xffffffff, seed >> 32]
    words = np.concatenate([ops.philox4x32_10([t, index, which, epoch], key) for t in range((size + 3) // 4)])[:size]
    return ((words.astype(np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


@pytest.mark.parametrize("n", [3, 21, 37, 1023, 1025, 70000])
def test_drawn_indices_stay_in_range(n):
    seed = (9 << 32) | 17
    for which in (0, 1):
        idx = _library_indices(n, 1024, 12345, which, 3, seed)
        assert idx.min() >= 0 and idx.max() < n
        assert np.array_equal(idx, R.draw_indices(n, 1024, 12345, which, 3, seed))
    assert not np.array_equal(_library_indices(n, 64, 12345, 0, 3, 17), _library_indices(n, 64, 12345, 1, 3, 17))


def test_drawn_indices_are_uniform():
    """n = 37 over 8192 draws: every bin count within 6 standard deviations of the mean (a fixed seed: deterministic)."""
    n, draws = 37, 8192
    idx = _library_indices(n, draws, 4242, 0, 1, 2024)
    assert np.array_equal(idx, R.draw_indices(n, draws, 4242, 0, 1, 2024))
    counts = np.bincount(idx, minlength=n)
    p = 1.0 / n
    mean, sd = draws * p, np.sqrt(draws * p * (1 - p))
    assert counts.sum() == draws and np.abs(counts - mean).max() <= 6 * sd, (counts.min(), counts.max(), mean, sd)


def test_struct_mirrors_match_the_header(tmp_path):
    """ptt_train_cand / ptt_train_batch_desc: ctypes and numpy agree with what gcc makes of include/ptt_hip.h."""
    from ptt_amd import _lib, ops
    pairs = [("ptt_train_cand", _lib.TrainCand, ops.TRAIN_CAND), ("ptt_train_batch_desc", _lib.TrainBatchDesc, ops.TRAIN_BATCH_DESC)]
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
    assert (ops.TRAIN_CAND.itemsize, ops.TRAIN_BATCH_DESC.itemsize) == (72, 104)
    assert _lib.ABI_VERSION >= 28 and ops.TRAIN_MAX_CANDS == 1024


def test_feeder_host_draws_equal_numpys_multivariate_normal():
    """The feeder forms the search offsets from standard_normal and a factor computed once; numpy's multivariate_normal, which the
    reference calls, must give the same numbers bit for bit."""
    from ptt_amd import train_feed
    for j in range(20):
        a = train_feed._search_normal(np.random.RandomState([3, 1, j]))
        b = np.random.RandomState([3, 1, j]).multivariate_normal(np.zeros(3), np.diag([1, 1, 5]), size=1)[0]
        assert np.array_equal(a, b), j
