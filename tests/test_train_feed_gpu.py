"""N5 on the device: ptt_amd.train_feed.TrainBatchFeeder (ptt_crop_compact_f32 + ptt_train_batch_f32) against its CPU restatement
(tests/train_feed_ref.py) and, through fixture G21, against the reference's own get_train_items. Everything the kernel writes is
a gathered row or a host-computed value, so every comparison is bitwise."""
import os
import warnings

import numpy as np
import pytest
import torch

from tests import train_feed_ref as R

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEED, EPOCH = 5, 2


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
    """The restatement's per-candidate results for (tracklets, SEED, epoch), shared by the tests and never modified by them."""
    return {EPOCH: {}, EPOCH + 1: {}}


def _feeder(trks, dev, **kw):
    from ptt_amd.train_feed import TrainBatchFeeder
    kw.setdefault("seed", SEED)
    return TrainBatchFeeder(trks, dev, **kw)


def _got(feeder, batch):
    """Everything a produced batch consists of, as host arrays (the batch dict and the feeder's bookkeeping outputs)."""
    o = feeder.last
    torch.cuda.synchronize()
    assert batch['search_points'] is o.search and batch['batch_size'] == feeder.B
    return {'search_points': o.search.cpu().numpy(), 'template_points': o.template.cpu().numpy(), 'cls_label': o.cls.cpu().numpy(),
            'reg_label': o.reg.cpu().numpy(), 'src': o.src.cpu().numpy().astype(np.int64), 'idx_search': o.idx_search.cpu().numpy().astype(np.int64),
            'idx_template': o.idx_template.cpu().numpy().astype(np.int64), 'info': o.info.cpu().numpy().astype(np.int64)}


KEYS = ('search_points', 'template_points', 'cls_label', 'reg_label', 'src', 'idx_search', 'idx_template', 'info')


def _assert_equal(got, ref, what):
    for k in KEYS:
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), (what, k)


@pytest.mark.parametrize("sizes", [(1024, 512), (256, 128)])
def test_batch_equals_the_restatement(dev, tracklets, cache, sizes):
    """B = 8, spare = 4: all four tensors, the source candidates, both index outputs and the info record, for a batch without a
    rejected sample and for one in which two primaries take spares."""
    f = _feeder(tracklets, dev, batch_size=8, spare=4, search_size=sizes[0], template_size=sizes[1])
    s = R.settings(batch_size=8, spare=4, search_size=sizes[0], template_size=sizes[1])
    assert len(f) == 12 and f.length == R.length(tracklets, s) == 96
    replaced = 0
    for number in (0, 10):
        ref = R.batch(tracklets, s, SEED, EPOCH, number, cache[EPOCH])
        assert ref['info'][2] == 0, "the restatement reports a shortfall: this seed exercises the wrap path"
        assert np.array_equal(f.plan(EPOCH, number)['index'], ref['index'])
        _assert_equal(_got(f, f.batch(EPOCH, number)), ref, (sizes, number))
        replaced += int(ref['info'][0])
        assert ref['search_points'].dtype == np.float32 and ref['cls_label'].dtype == np.float32
        assert set(np.unique(ref['cls_label'])) <= {0.0, 1.0} and ref['cls_label'].sum() > 0
    assert replaced >= 1                                        # batch 10 of this seed rejects two primaries
    st = f.stats()
    assert st == {'batches': 2, 'invalid_primaries': replaced, 'shortfall': 0, 'all_invalid': 0}


def test_batch_equals_the_reference_through_G21(dev):
    """G21's tracklets, every dataset index in order: a valid sample is the reference's crop gathered at the kernel's indices; the
    samples the reference rejects are the ones replaced."""
    g = np.load(os.path.join(GOLD, "G21_train_items.npz"))
    trks = []
    for t in range(int(g["n_tracklets"])):
        n = int(g["n_frames_%d" % t])
        trks.append(([g["cloud_%d_%d" % (t, i)] for i in range(n)],
                     [(g["box_%d_%d" % (t, i)][0:3], g["box_%d_%d" % (t, i)][3:6], g["box_%d_%d" % (t, i)][6:10]) for i in range(n)]))
    f = _feeder(trks, dev, batch_size=8, spare=4, seed=int(g["seed"]), shuffle=False)
    assert f.length == int(g["len"]) == 24 and len(f) == 3
    f.set_epoch(int(g["epoch"]))
    checked = rejected = 0
    for number, batch in enumerate(f):
        got = _got(f, batch)
        plan = f.plan(int(g["epoch"]), number)
        for b in range(8):
            j = number * 8 + b
            assert plan['index'][b] == j
            assert np.array_equal(plan['search_offset'][b], g["search_offset_%d" % j])
            if not bool(g["valid_%d" % j]):
                assert got['src'][b] != b
                rejected += 1
                continue
            assert got['src'][b] == b
            assert np.array_equal(plan['template_offset'][b], g["template_offset_%d" % j])
            crop, label, tpl = g["search_%d" % j].T, g["label_%d" % j], g["template_%d" % j].T
            ids, idt = got['idx_search'][b], got['idx_template'][b]
            assert ids.min() >= 0 and ids.max() < crop.shape[0] and idt.min() >= 0 and idt.max() < tpl.shape[0]
            assert np.array_equal(got['search_points'][b], crop[ids]), j
            assert np.array_equal(got['cls_label'][b], label[ids].astype(np.float32)), j
            assert np.array_equal(got['template_points'][b], tpl[idt]), j
            assert np.array_equal(got['reg_label'][b], g["reg_%d" % j].astype(np.float32)), j
            checked += 1
    assert checked == 20 and rejected == 4


def test_pass_through(dev, tracklets, cache):
    """search_size (template_size) equal to a crop's exact count: that slot's rows arrive in their original order, indices -1 — odd
    sizes, so also the stores of a size that is no multiple of four."""
    s = R.settings(batch_size=8, spare=4)
    ref = R.batch(tracklets, s, SEED, EPOCH, 0, cache[EPOCH])
    b = 3
    assert ref['src'][b] == b
    c = ref['candidates'][b]
    ns, nt = c['search'].shape[0], c['template'].shape[0]
    for sizes in ((ns, 512), (1024, nt), (ns, nt)):
        f = _feeder(tracklets, dev, batch_size=8, spare=4, search_size=sizes[0], template_size=sizes[1])
        s2 = R.settings(batch_size=8, spare=4, search_size=sizes[0], template_size=sizes[1])
        ref2 = R.batch(tracklets, s2, SEED, EPOCH, 0, cache[EPOCH])
        got = _got(f, f.batch(EPOCH, 0))
        _assert_equal(got, ref2, sizes)
        if sizes[0] == ns:
            assert np.array_equal(got['search_points'][b], c['search']) and (got['idx_search'][b] == -1).all()
            assert np.array_equal(got['cls_label'][b], c['label'].astype(np.float32))
        if sizes[1] == nt:
            assert np.array_equal(got['template_points'][b], c['template']) and (got['idx_template'][b] == -1).all()


def test_unaligned_outputs_take_the_element_stores(dev, tracklets, cache):
    """Sizes that are multiples of four, but outputs that start 4 bytes past a 16-byte boundary (a caller's sliced tensors): the
    same batch, written without the float4 / int4 stores."""
    f = _feeder(tracklets, dev, batch_size=8, spare=4, search_size=256, template_size=128)
    ref = R.batch(tracklets, R.settings(batch_size=8, spare=4, search_size=256, template_size=128), SEED, EPOCH, 10, cache[EPOCH])
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
        assert np.array_equal(got.astype(ref[key].dtype), ref[key]), key
        assert int(big[0]) == 7 and (big[1 + t.numel():] == 7).all(), key          # nothing written around the buffer
    assert np.array_equal(out.reg.cpu().numpy(), ref['reg_label']) and np.array_equal(out.src.cpu().numpy(), ref['src'])


def test_from_config_and_sampled_interval(dev, tracklets):
    """The feeder of a DATA_CONFIG mapping with SAMPLED_INTERVAL = 2: half the samples, the even augmentations, and a batch equal
    to the restatement under the same settings."""
    from ptt_amd.train_feed import TrainBatchFeeder
    cfg = dict(SEARCH_INPUT_SIZE=256, TEMPLATE_INPUT_SIZE=128, SAMPLED_INTERVAL=2, NUM_CANDIDATES_PERFRAME=4, SEARCH_BB_SCALE=1.25)
    f = TrainBatchFeeder.from_config(tracklets, dev, cfg, 8, spare=4, seed=SEED)
    s = R.settings(batch_size=8, spare=4, search_size=256, template_size=128, sampled_interval=2)
    assert f.length == R.length(tracklets, s) == 48 and len(f) == 6 and (f.S, f.T, f.interval) == (256, 128, 2)
    ref = R.batch(tracklets, s, SEED, EPOCH, 1, {})
    plan = f.plan(EPOCH, 1)
    assert np.array_equal(plan['index'], ref['index']) and set(plan['aug'].tolist()) <= {0, 2}
    _assert_equal(_got(f, f.batch(EPOCH, 1)), ref, "interval 2")


def test_replacement(dev):
    """Dataset = two good frames (indices 0, 1), a frame of 12 points and an empty frame (2, 3: rejected), one candidate per frame,
    unshuffled: the primaries of batch 0 are 0..3. Under seed 1 the spares are the indices 0, 1, 0, 2 (one spare: 0)."""
    from ptt_amd import synth
    clouds, boxes = synth.tracklet(3, 2, n_obj=(100, 300), n_bg=(300, 800))
    sparse = ([np.ascontiguousarray(clouds[0][:, :12]), np.zeros((3, 0), np.float32)], boxes)
    kw = dict(batch_size=4, candidates_per_frame=1, shuffle=False, seed=1, search_size=64, template_size=32)
    # enough spares: the rejected primaries take the valid spares in order
    f = _feeder([(clouds, boxes), sparse], dev, spare=4, **kw)
    assert f.plan(0, 0)['index'].tolist() == [0, 1, 2, 3, 0, 1, 0, 2]
    got = _got(f, f.batch(0, 0))
    assert got['src'].tolist() == [0, 1, 4, 5] and got['info'].tolist() == [2, 3, 0, 0]
    assert np.array_equal(got['search_points'][2], got['search_points'][0]) and np.array_equal(got['template_points'][3], got['template_points'][1])
    assert np.array_equal(got['reg_label'][2], got['reg_label'][0]) and np.abs(got['search_points']).sum() > 0
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert f.stats()['shortfall'] == 0
    # one spare, two rejected: the second wraps to the first valid candidate; reported, warned about once
    f = _feeder([(clouds, boxes), sparse], dev, spare=1, **kw)
    assert f.plan(0, 0)['index'].tolist() == [0, 1, 2, 3, 0]
    got = _got(f, f.batch(0, 0))
    assert got['src'].tolist() == [0, 1, 4, 0] and got['info'].tolist() == [2, 1, 1, 0]
    assert np.array_equal(got['search_points'][3], got['search_points'][0])
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert f.stats() == {'batches': 1, 'invalid_primaries': 2, 'shortfall': 1, 'all_invalid': 0}
        assert f.stats()['shortfall'] == 1
    assert len([x for x in w if "spare" in str(x.message)]) == 1
    # every candidate rejected: zeros, source -1, all_invalid
    f = _feeder([sparse], dev, batch_size=2, spare=2, candidates_per_frame=1, shuffle=False, seed=1, search_size=64, template_size=32)
    got = _got(f, f.batch(0, 0))
    assert got['src'].tolist() == [-1, -1] and got['info'].tolist() == [2, 0, 2, 1]
    for k in ('search_points', 'template_points', 'cls_label', 'reg_label'):
        assert not got[k].any(), k
    assert (got['idx_search'] == -1).all() and (got['idx_template'] == -1).all()


def test_reproducible_and_independent_of_batch_composition(dev, tracklets, cache):
    kw = dict(batch_size=8, spare=4, search_size=256, template_size=128)
    s = R.settings(**kw)

    def epoch(feeder, e, rs):
        """{dataset index: the sample's four tensors} over the valid primaries of an epoch, and all primaries in order."""
        feeder.set_epoch(e)
        samples, prim = {}, []
        for number, batch in enumerate(feeder):
            got = _got(feeder, batch)
            ref = R.batch(tracklets, rs, SEED, e, number, cache[e])
            assert ref['info'][2] == 0, "the restatement reports a shortfall: this seed exercises the wrap path"
            assert np.array_equal(got['src'], ref['src'])
            index = feeder.plan(e, number)['index']
            prim += index[:8].tolist()
            for b in range(8):
                if got['src'][b] == b:
                    samples[int(index[b])] = tuple(got[k][b].copy() for k in KEYS[:4])
        return samples, prim

    one, prim_one = epoch(_feeder(tracklets, dev, **kw), EPOCH, s)
    again, prim_again = epoch(_feeder(tracklets, dev, **kw), EPOCH, s)
    assert prim_one == prim_again and sorted(prim_one) == list(range(96))
    assert one.keys() == again.keys() and all(np.array_equal(a, b) for j in one for a, b in zip(one[j], again[j]))
    other, prim_other = epoch(_feeder(tracklets, dev, **kw), EPOCH + 1, s)
    assert prim_other != prim_one
    assert any(not np.array_equal(one[j][0], other[j][0]) for j in one if j in other)
    halves, prim_halves = {}, []
    for rank in (0, 1):
        f = _feeder(tracklets, dev, rank=rank, world=2, **kw)
        assert len(f) == 6
        smp, prim = epoch(f, EPOCH, R.settings(rank=rank, world=2, **kw))
        assert not set(smp) & set(halves)
        halves.update(smp)
        prim_halves += prim
    assert sorted(prim_halves) == sorted(prim_one)
    assert halves.keys() == one.keys() and len(one) >= 90
    for j in one:
        assert all(np.array_equal(a, b) for a, b in zip(one[j], halves[j])), j


def test_buffer_lifetime_and_side_stream(dev, tracklets, cache):
    kw = dict(batch_size=8, spare=4, search_size=256, template_size=128)
    s = R.settings(**kw)
    f = _feeder(tracklets, dev, depth=2, **kw)
    f.set_epoch(EPOCH)
    it = iter(f)
    first = next(it)
    kept = {k: v.clone() for k, v in first.items() if torch.is_tensor(v)}
    second = next(it)
    torch.cuda.synchronize()
    assert second['search_points'] is not first['search_points']
    assert all(torch.equal(first[k], kept[k]) for k in kept)               # one further batch: the first is still there
    third = next(it)
    assert third['search_points'] is first['search_points']                # the depth-th further batch takes its set
    # production on a stream of its own: what the consumer enqueues on ITS stream right after receiving a batch sees all of it
    side = torch.cuda.Stream(device=dev)
    f = _feeder(tracklets, dev, depth=2, stream=side, **kw)
    f.set_epoch(EPOCH)
    seen = []
    for number, batch in zip(range(4), f):
        seen.append({k: v.clone() for k, v in batch.items() if torch.is_tensor(v)})        # no synchronisation in between
    torch.cuda.synchronize()
    for number, clones in enumerate(seen):
        ref = R.batch(tracklets, s, SEED, EPOCH, number, cache[EPOCH])
        for k in clones:
            assert np.array_equal(clones[k].cpu().numpy(), ref[k]), (number, k)
    assert f.stats()['batches'] == 4


def test_feeds_the_captured_training_step(dev, tracklets, cache):
    """DataParallelTrainer in graph mode fed by the feeder against an eager trainer fed the restatement's batches, from the same
    initial weights: bit-identical losses (what tests/test_train_graph_gpu.py establishes for resident batches)."""
    from ptt_amd.config import StubDataset, ptt_model_cfg
    from ptt_amd.models import build_network
    from ptt_amd.train_step import DataParallelTrainer

    def trainer(graph):
        torch.manual_seed(1)
        model = build_network(ptt_model_cfg(), 1, StubDataset(training=True)).to(dev).train()
        return DataParallelTrainer(model, dev, graph=graph)

    eager, graphed = trainer(False), trainer(True)
    kw = dict(batch_size=4, spare=2)
    s = R.settings(**kw)
    f = _feeder(tracklets, dev, **kw)
    f.set_epoch(EPOCH)
    for number, batch in zip(range(5), f):
        ref = R.batch(tracklets, s, SEED, EPOCH, number, cache[EPOCH])
        assert ref['info'][2] == 0, "the restatement reports a shortfall: this seed exercises the wrap path"
        rb = {k: torch.from_numpy(ref[k]).to(dev) for k in KEYS[:4]}
        rb['batch_size'] = 4
        le = eager.step(rb).detach().clone()
        lg = graphed.step(batch).detach().clone()
        torch.cuda.synchronize()
        assert torch.equal(le, lg) and bool(torch.isfinite(lg)), (number, float(le), float(lg))
    assert graphed.graph_steps == 2 and graphed.eager_steps == 3 and eager.captured is None
