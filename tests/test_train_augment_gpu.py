"""DATA_AUGMENTOR on the device: TrainBatchFeeder(augmentor=...) (ptt_train_batch_aug_f32) against the un-augmented restatement
(tests/train_feed_ref.py) with the host mirror applied per slot on the draws of the slot's source (tests/train_augment_util.py,
where the bounds are derived). Queues without a rotation are compared bitwise."""
import ctypes

import numpy as np
import pytest
import torch

from tests import train_augment_util as A
from tests import train_feed_ref as R

pytestmark = pytest.mark.gpu
SEED, EPOCH = 5, 2
KEYS = ('search_points', 'template_points', 'cls_label', 'reg_label', 'src', 'idx_search', 'idx_template', 'info')


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def tracklets():
    from ptt_amd import synth
    return [synth.tracklet(seed, 6, n_obj=(100, 300), n_bg=(300, 800)) for seed in range(4)]


@pytest.fixture(scope="module")
def cache():
    """The restatement's per-candidate results for (tracklets, SEED, EPOCH), shared by the tests and never modified by them."""
    return {}


def _feeder(trks, dev, **kw):
    from ptt_amd.train_feed import TrainBatchFeeder
    kw.setdefault("seed", SEED)
    return TrainBatchFeeder(trks, dev, **kw)


def _got(feeder):
    o = feeder.last
    torch.cuda.synchronize()
    return {'search_points': o.search.cpu().numpy(), 'template_points': o.template.cpu().numpy(), 'cls_label': o.cls.cpu().numpy(),
            'reg_label': o.reg.cpu().numpy(), 'src': o.src.cpu().numpy().astype(np.int64), 'idx_search': o.idx_search.cpu().numpy().astype(np.int64),
            'idx_template': o.idx_template.cpu().numpy().astype(np.int64), 'info': o.info.cpu().numpy().astype(np.int64)}


def _expected(tracklets, cache, feeder, cfg, number, **kw):
    ref = R.batch(tracklets, R.settings(**kw), SEED, EPOCH, number, cache)
    assert ref['info'][2] == 0, "the restatement reports a shortfall: this seed exercises the wrap path"
    return A.expected_batch(ref, feeder.plan(EPOCH, number), cfg)


def _assert_within(got, exp, ref, n_scalings, what):
    """Points within the bounds of the util module around the mirror's, everything else bitwise (theta included)."""
    for k in ('cls_label', 'src', 'idx_search', 'idx_template', 'info'):
        assert got[k].dtype == exp[k].dtype and np.array_equal(got[k], exp[k]), (what, k)
    assert np.array_equal(got['reg_label'][:, 3], exp['reg_label'][:, 3]), (what, 'theta')
    for b in range(len(got['src'])):
        A.assert_points_within(got['search_points'][b], exp['search_points'][b], ref['search_points'][b], exp['k'][b], 16, n_scalings, (what, b, 'search'))
        A.assert_points_within(got['template_points'][b], exp['template_points'][b], ref['template_points'][b], exp['k'][b], 16, n_scalings, (what, b, 'template'))


def test_flip_and_scaling_batch_is_bitwise_the_mirrors(dev, tracklets, cache):
    """No rotation: flips are exact and the one scaling is one float32 product on both sides — all eight outputs, for a batch
    without a rejected sample and for one in which two primaries take spares."""
    kw = dict(batch_size=8, spare=4, search_size=64, template_size=32)
    f = _feeder(tracklets, dev, augmentor=A.FLIP_SCALE, **kw)
    replaced = changed = 0
    for number in (0, 10):
        exp = _expected(tracklets, cache, f, A.FLIP_SCALE, number, **kw)
        f.batch(EPOCH, number)
        got = _got(f)
        for k in KEYS:
            assert got[k].dtype == exp[k].dtype and np.array_equal(got[k], exp[k]), (number, k)
        replaced += int(got['info'][0])
        changed += int(not np.array_equal(got['search_points'], R.batch(tracklets, R.settings(**kw), SEED, EPOCH, number, cache)['search_points']))
    assert replaced >= 1 and changed == 2


@pytest.mark.parametrize("name,cfg,numbers", [("p2b_scale", A.P2B_SCALE, (0, 10)), ("two_scales", A.TWO_SCALES, (10,))])
def test_p2b_queue_with_scaling(dev, tracklets, cache, name, cfg, numbers):
    """The p2b.yaml block followed by a scaling (z: one float32 product on both sides, bitwise), and the same between two scalings
    (z within 4 u |z| k: the mirror rounds after each product, the map once)."""
    kw = dict(batch_size=8, spare=4, search_size=256, template_size=128)
    f = _feeder(tracklets, dev, augmentor={'AUG_CONFIG_LIST': cfg}, **kw)
    n_scalings = A.scalings(f.aug_kinds)
    assert n_scalings == (1 if name == "p2b_scale" else 2)
    for number in numbers:
        exp = _expected(tracklets, cache, f, cfg, number, **kw)
        ref = R.batch(tracklets, R.settings(**kw), SEED, EPOCH, number, cache)
        f.batch(EPOCH, number)
        got = _got(f)
        _assert_within(got, exp, ref, n_scalings, (name, number))
        # the label's centre: formed in float64 by the host, against the mirror's float32 rotation (4 u (|x| + |y|) k, held on
        # the host by test_train_augment_cpu.py), plus the cast to float32 of either side (u (|x| + |y|) k each)
        raw = f.plan(EPOCH, number)['reg_label_raw'][got['src']]
        A.assert_centre_within(got['reg_label'][:, :3], exp['reg_label'][:, :3], raw[:, :3], exp['k'], 6, (name, number, 'reg'))
        assert not np.array_equal(got['search_points'], ref['search_points'])


def test_map_entries_are_wired_as_declared(dev, tracklets, cache):
    """ptt_train_batch_aug_f32 with a hand-made table, M = [[2, 4], [-8, 0.5]], kz = -2, on a feeder's crops: products by powers
    of two are exact, so each output carries one rounding however the compiler contracts, and equals numpy's float32
    2x + 4y, -8x + 0.5y, -2z bitwise. A transposed, swapped or mis-strided entry cannot."""
    from ptt_amd import ops
    kw = dict(batch_size=8, spare=4, search_size=64, template_size=32)
    f = _feeder(tracklets, dev, **kw)
    assert f.aug_dev is None
    f.batch(EPOCH, 10)
    plain = _got(f)
    table = np.zeros(f.C, ops.TRAIN_AUG)
    table['m'], table['kz'] = np.array([2, 4, -8, 0.5], np.float32), -2
    aug_dev = torch.from_numpy(table.view(np.uint8)).to(dev)
    ops.train_batch(f.cands_dev, f.last.desc, dev, aug_dev)
    got = _got(f)
    two, four, eight, half = (np.float32(v) for v in (2, 4, 8, 0.5))
    for k in ('search_points', 'template_points'):
        p = plain[k]
        want = np.stack([two * p[..., 0] + four * p[..., 1], -eight * p[..., 0] + half * p[..., 1], -two * p[..., 2]], -1)
        assert want.dtype == np.float32 and np.array_equal(got[k], want), k
        assert np.abs(got[k]).sum() > 0
    for k in KEYS[2:]:
        assert np.array_equal(got[k], plain[k]), k


@pytest.mark.parametrize("sizes", [(66, 30), (64, 32)])
def test_element_stores(dev, tracklets, cache, sizes):
    """Sizes that are no multiples of four, and multiples of four with every output 4 bytes past a 16-byte boundary: the element
    path applies the same map as the float4 path — the moved run equals the run in place bitwise, both are within the bounds
    around the mirror, and the fill words around every buffer survive."""
    kw = dict(batch_size=8, spare=4, search_size=sizes[0], template_size=sizes[1])
    f = _feeder(tracklets, dev, augmentor=A.P2B_SCALE, depth=1, **kw)
    exp = _expected(tracklets, cache, f, A.P2B_SCALE, 10, **kw)
    ref = R.batch(tracklets, R.settings(**kw), SEED, EPOCH, 10, cache)
    f.batch(EPOCH, 10)
    in_place = _got(f)
    _assert_within(in_place, exp, ref, 1, sizes)
    out, moved = f._sets[0], {}
    for field, t, key in (('search_points', out.search, 'search_points'), ('template_points', out.template, 'template_points'),
                          ('cls_label', out.cls, 'cls_label'), ('idx_search_out', out.idx_search, 'idx_search'),
                          ('idx_template_out', out.idx_template, 'idx_template')):
        big = torch.full((t.numel() + 8,), 7, dtype=t.dtype, device=dev)
        assert big.data_ptr() % 16 == 0
        out.desc[field] = big.data_ptr() + 4
        moved[key] = (big, t)
    f.batch(EPOCH, 10)
    torch.cuda.synchronize()
    for key, (big, t) in moved.items():
        got = big[1:1 + t.numel()].view(t.shape).cpu().numpy()
        assert np.array_equal(got.astype(in_place[key].dtype), in_place[key]), key
        assert int(big[0]) == 7 and (big[1 + t.numel():] == 7).all(), key          # nothing written around the buffer
    assert np.array_equal(out.reg.cpu().numpy(), in_place['reg_label']) and np.array_equal(out.src.cpu().numpy(), in_place['src'])


def test_replacement_carries_the_spares_augmentation(dev):
    """The sparse data set of test_train_feed_gpu.test_replacement: primaries 0..3 (2, 3 rejected), spares 0, 1, 0, 2. Slot 2
    is filled by a spare with dataset index 0 and equals slot 0, slot 3 by one with index 1 and equals slot 1 — points and label,
    bitwise, both augmented. With every candidate rejected: zeros, source -1."""
    from ptt_amd import synth
    clouds, boxes = synth.tracklet(3, 2, n_obj=(100, 300), n_bg=(300, 800))
    sparse = ([np.ascontiguousarray(clouds[0][:, :12]), np.zeros((3, 0), np.float32)], boxes)
    kw = dict(batch_size=4, candidates_per_frame=1, shuffle=False, seed=1, search_size=64, template_size=32, spare=4)
    f = _feeder([(clouds, boxes), sparse], dev, augmentor=A.P2B_SCALE, **kw)
    plan = f.plan(0, 0)
    assert plan['index'].tolist() == [0, 1, 2, 3, 0, 1, 0, 2]
    assert np.array_equal(plan['aug_map'][4], plan['aug_map'][0]) and not np.array_equal(plan['aug_map'][2], plan['aug_map'][0])
    f.batch(0, 0)
    got = _got(f)
    assert got['src'].tolist() == [0, 1, 4, 5] and got['info'].tolist() == [2, 3, 0, 0]
    for a, b in ((2, 0), (3, 1)):
        for k in ('search_points', 'template_points', 'reg_label', 'cls_label'):
            assert np.array_equal(got[k][a], got[k][b]), (a, k)
    g = _feeder([(clouds, boxes), sparse], dev, **kw)
    g.batch(0, 0)
    plain = _got(g)
    for k in ('cls_label', 'src', 'idx_search', 'idx_template', 'info'):
        assert np.array_equal(got[k], plain[k]), k
    for b in range(4):
        src = got['src'][b]
        k = A.scale_product(plan['aug_kinds'], plan['aug_draws'][src])
        A.assert_points_within(got['search_points'][b], A.apply_map(plan['aug_map'][src], plain['search_points'][b]), plain['search_points'][b],
                               k, 16, 1, (b, 'the map of the source'))
        assert not np.array_equal(got['search_points'][b], plain['search_points'][b])
    f = _feeder([sparse], dev, batch_size=2, spare=2, candidates_per_frame=1, shuffle=False, seed=1, search_size=64, template_size=32,
                augmentor=A.P2B_SCALE)
    f.batch(0, 0)
    got = _got(f)
    assert got['src'].tolist() == [-1, -1] and got['info'].tolist() == [2, 0, 2, 1]
    for k in ('search_points', 'template_points', 'cls_label', 'reg_label'):
        assert not got[k].any(), k
    assert (got['idx_search'] == -1).all() and (got['idx_template'] == -1).all()


def test_null_table_is_the_old_entry_point(dev, tracklets, cache):
    """ptt_train_batch_aug_f32(aug_device = NULL) against ptt_train_batch_f32 (what a feeder without an augmentor calls) on the
    same candidates: every output bitwise; both equal the restatement."""
    from ptt_amd import ops
    kw = dict(batch_size=8, spare=4, search_size=256, template_size=128)
    f = _feeder(tracklets, dev, **kw)
    f.batch(EPOCH, 10)
    old = _got(f)
    o = f.last
    for t in (o.search, o.template, o.cls, o.reg, o.src, o.idx_search, o.idx_template, o.info):
        t.fill_(3)
    ops._launch("ptt_train_batch_aug_f32", dev, ops._ptr(f.cands_dev), ctypes.c_void_p(0), ctypes.c_void_p(o.desc.ctypes.data))
    new = _got(f)
    ref = R.batch(tracklets, R.settings(**kw), SEED, EPOCH, 10, cache)
    for k in KEYS:
        assert np.array_equal(new[k], old[k]) and np.array_equal(old[k], ref[k]), k


def test_reproducible(dev, tracklets):
    kw = dict(batch_size=8, spare=4, search_size=64, template_size=32, augmentor=A.P2B_SCALE)
    one, two = _feeder(tracklets, dev, **kw), _feeder(tracklets, dev, **kw)
    two.batch(EPOCH, 3)                                         # another history: a different output set, another batch before
    one.batch(EPOCH, 10)
    a = _got(one)
    two.batch(EPOCH, 10)
    b = _got(two)
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k
    one.batch(EPOCH + 1, 10)
    assert not np.array_equal(_got(one)['search_points'], a['search_points'])


def test_both_launches_replay_from_a_graph(dev, tracklets):
    """The crop launch and ptt_train_batch_aug_f32 captured once on an augmented feeder's tables: a replay reads whatever table
    was uploaded last (every address is fixed) and equals the eager batch of that table bitwise, all eight outputs."""
    from ptt_amd import ops
    f = _feeder(tracklets, dev, batch_size=8, spare=4, search_size=64, template_size=32, augmentor=A.P2B_SCALE, depth=1)
    f.batch(EPOCH, 10)
    first = _got(f)
    out = f.last
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.crop_compact(f.table_dev, 3 * f.C)
        ops.train_batch(f.cands_dev, out.desc, dev, f.aug_dev)
    f.batch(EPOCH, 3)                                           # another table in the same device buffers
    eager = _got(f)
    assert f.last is out and not np.array_equal(eager['search_points'], first['search_points'])
    for t in (out.search, out.template, out.cls, out.reg, out.src, out.idx_search, out.idx_template, out.info):
        t.fill_(3)
    graph.replay()
    replayed = _got(f)
    for k in KEYS:
        assert np.array_equal(replayed[k], eager[k]), k
