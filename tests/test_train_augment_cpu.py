"""DATA_AUGMENTOR without a device: the host mirror ptt_amd.datasets.augmentor against the reference (fixture G27,
tests/golden/make_golden_g27.py), and the host half of the feeder's augmentation (TrainBatchPlan: the draw stream, the composite
map, the augmented reg_label) against that mirror. Bounds: tests/train_augment_util.py."""
import json
import os
import pickle

import numpy as np
import pytest

from tests import train_augment_util as A

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = A.U
SEED, EPOCH = 5, 2


class Recording(object):
    """A RandomState that keeps what it hands out."""

    def __init__(self, seed):
        self.rs, self.draws = np.random.RandomState(seed), []

    def choice(self, *a, **kw):
        self.draws.append(float(self.rs.choice(*a, **kw)))
        return bool(self.draws[-1])

    def uniform(self, *a, **kw):
        self.draws.append(self.rs.uniform(*a, **kw))
        return self.draws[-1]


@pytest.fixture(scope="module")
def g27():
    return np.load(os.path.join(GOLD, "G27_augmentor.npz"))


@pytest.fixture(scope="module")
def tracklets():
    from ptt_amd import synth
    return [synth.tracklet(seed, 6, n_obj=(100, 300), n_bg=(300, 800)) for seed in range(4)]


def _plan(trks, **kw):
    from ptt_amd.train_feed import TrainBatchPlan
    kw.setdefault("seed", SEED)
    return TrainBatchPlan(trks, batch_size=8, spare=4, rank=0, world=1, **kw)


def _kinds(cfg):
    return [e['NAME'] for e in cfg]


# ------------------------------------------------------------------ the mirror against the reference
def test_mirror_equals_the_reference_through_G27(g27):
    from ptt_amd.datasets.augmentor import DataAugmentor
    cases = [str(c) for c in g27["cases"]]
    assert len(cases) == 7
    rotated = exact = 0
    for ci, name in enumerate(cases):
        cfg = json.loads(str(g27["cfg_%s" % name]))
        aug = DataAugmentor(None, cfg, None)
        n_rot = _kinds(cfg).count('random_world_rotation')
        for s in range(int(g27["seeds"])):
            key = "%s_%d_" % (name, s)
            search, template, reg = g27[key + "search_in"], g27[key + "template_in"], g27[key + "reg_in"]
            rng = Recording([27, ci, s])
            d = aug.forward({'search_points': search.copy(), 'template_points': template.copy(), 'reg_label': reg.copy()[None]}, rng=rng)
            assert np.array_equal(np.array(rng.draws), g27[key + "draws"]), key                       # the draws: bitwise
            assert d['search_points'].dtype == np.float32 and d['reg_label'].shape == (1, 4) and d['reg_label'].dtype == np.float64
            got = (d['search_points'], d['template_points'], d['reg_label'][0])
            want = (g27[key + "search_out"], g27[key + "template_out"], g27[key + "reg_out"])
            assert got[2][3] == want[2][3], key                                                           # theta: bitwise
            if n_rot == 0:
                assert all(np.array_equal(a, b) for a, b in zip(got, want)), key
                exact += 1
            else:
                scales = [v for e, v in zip(_draw_kinds(cfg), rng.draws) if e == 'scaling']
                k = float(np.prod(scales + [1.0]))
                A.assert_points_within(got[0], want[0], search, k, 4, len(scales), key + "search")
                A.assert_points_within(got[1], want[1], template, k, 4, len(scales), key + "template")
                A.assert_points_within(got[2][None, :3], want[2][None, :3], reg[None, :3], k, 4, len(scales), key + "reg")
                rotated += 1
            # the (4,) label the dataset produces: accepted, same values, same shape back
            rng4 = Recording([27, ci, s])
            d4 = aug.forward({'search_points': search.copy(), 'template_points': template.copy(), 'reg_label': reg.copy()}, rng=rng4)
            assert d4['reg_label'].shape == (4,) and np.array_equal(d4['reg_label'], got[2]) and rng4.draws == rng.draws
            assert np.array_equal(d4['search_points'], got[0]) and np.array_equal(d4['template_points'], got[1])
    assert rotated == 24 and exact == 18


def _draw_kinds(cfg):
    """The kind of every draw a queue makes, in order."""
    out = []
    for e in cfg:
        if e['NAME'] == 'random_world_flip':
            out += ['flip_' + a for a in e['ALONG_AXIS_LIST']]
        elif e['NAME'] == 'random_world_rotation':
            out.append('rotation')
        elif e['WORLD_SCALE_RANGE'][1] - e['WORLD_SCALE_RANGE'][0] >= 1e-3:
            out.append('scaling')
    return out


def test_mirror_draws_from_numpys_global_generator_by_default(g27):
    """rng defaults to np.random: in the state of RandomState(s) it makes the draws of RandomState(s)."""
    from ptt_amd.datasets.augmentor import DataAugmentor
    state = np.random.get_state()
    try:
        key = "p2b_0_"
        np.random.set_state(np.random.RandomState([27, 0, 0]).get_state())
        d = DataAugmentor(None, A.P2B, None).forward({'search_points': g27[key + "search_in"].copy(), 'template_points': g27[key + "template_in"].copy(),
                                                      'reg_label': g27[key + "reg_in"].copy()})
        assert d['reg_label'][3] == g27[key + "reg_out"][3]
    finally:
        np.random.set_state(state)


def test_augmentor_config_forms_and_pickle():
    from ptt_amd.datasets.augmentor import DataAugmentor, augmentor_utils
    import ptt.datasets.augmentor.data_augmentor as alias
    assert alias.DataAugmentor.__name__ == 'DataAugmentor' and alias.__file__ == DataAugmentor.forward.__code__.co_filename

    class Ns(dict):
        __getattr__ = dict.__getitem__

    forms = [A.P2B, {'AUG_CONFIG_LIST': A.P2B}, Ns(AUG_CONFIG_LIST=[Ns(e) for e in A.P2B])]
    steps = [DataAugmentor(None, f, ['Car']).steps for f in forms]
    assert steps[0] == steps[1] == steps[2] == [('random_world_flip', ['x']), ('random_world_rotation', [-0.78539816, 0.78539816])]
    assert DataAugmentor(None, [{'NAME': 'random_world_rotation', 'WORLD_ROT_ANGLE': 0.5}], None).steps[0][1] == [-0.5, 0.5]
    aug = DataAugmentor('root', A.P2B_SCALE, ['Car'], logger=object())
    back = pickle.loads(pickle.dumps(aug))
    assert not hasattr(back, 'logger') or back.logger is None
    assert back.steps == aug.steps and back.root_path == 'root' and len(back.data_augmentor_queue) == 3
    for bad in ([{'NAME': 'random_world_shear'}], [{'NAME': 'forward'}], [{'NAME': 'random_world_flip', 'ALONG_AXIS_LIST': ['z']}]):
        with pytest.raises(ValueError):
            DataAugmentor(None, bad, None)
    assert callable(augmentor_utils.random_flip_along_x) and callable(augmentor_utils.random_flip_along_y)


# ------------------------------------------------------------------ the plan
def test_plan_with_an_augmentor_moves_nothing_else(tracklets):
    plain, aug = _plan(tracklets), _plan(tracklets, augmentor=A.P2B_SCALE)
    assert aug.aug_kinds == ('flip_x', 'rotation', 'scaling') and plain.aug_kinds == ()
    for number in (0, 10):
        p, q = plain.plan(EPOCH, number), aug.plan(EPOCH, number)
        assert 'aug_map' not in p and 'aug_draws' not in p
        for k in ('index', 'anno', 'aug', 'search_offset', 'template_offset'):
            assert np.array_equal(p[k], q[k]), k
        assert np.array_equal(p['reg_label'], q['reg_label_raw'])
        assert np.array_equal(p['_jobs'].view(np.uint8), q['_jobs'].view(np.uint8))
        assert q['aug_map'].shape == (12, 5) and q['aug_map'].dtype == np.float32 and q['aug_draws'].shape == (12, 3)
        assert not np.array_equal(q['reg_label'], q['reg_label_raw'])


@pytest.mark.parametrize("name,cfg", [("flip_scale", A.FLIP_SCALE), ("p2b_scale", A.P2B_SCALE),
                                      ("scale_rot_flip", [A.SCALE, A.P2B[1], {'NAME': 'random_world_flip', 'ALONG_AXIS_LIST': ['y', 'x']}]),
                                      ("repeated", A.P2B + A.P2B), ("two_scales", A.TWO_SCALES)])
def test_plan_map_and_label_agree_with_the_mirror(tracklets, name, cfg):
    plan = _plan(tracklets, augmentor=cfg)
    q = plan.plan(EPOCH, 3)
    rs = np.random.RandomState(9)
    rotation, n_scalings = 'rotation' in plan.aug_kinds, A.scalings(plan.aug_kinds)
    flags = set()
    for c in range(plan.C):
        pts = (rs.standard_normal((32, 3)) * [4.0, 3.0, 1.0]).astype(np.float32)
        draws, raw = q['aug_draws'][c], q['reg_label_raw'][c]
        k = A.scale_product(plan.aug_kinds, draws)
        ms, mt, mreg = A.mirror(cfg, draws, pts, pts[:8], raw)
        got = A.apply_map(q['aug_map'][c], pts)
        assert mreg.shape == (4,)
        assert np.float32(q['reg_label'][c, 3]) == np.float32(mreg[3]), (name, c)                     # theta: bitwise in float32
        if rotation:
            A.assert_points_within(got, ms, pts, k, 16, n_scalings, (name, c))
            A.assert_centre_within(q['reg_label'][c][None, :3], mreg[None, :3], raw[None, :3], k, 4, (name, c, 'reg'))
        else:
            assert np.array_equal(got, ms) and np.array_equal(q['reg_label'][c], mreg), (name, c)
        flags.update((kind, bool(d)) for kind, d in zip(plan.aug_kinds, draws) if kind.startswith('flip'))
    assert len(flags) == 2 * len([kind for kind in set(plan.aug_kinds) if kind.startswith('flip')])      # every flip seen on and off


def test_a_sample_is_a_function_of_seed_epoch_and_index(tracklets):
    """The same dataset index in two different batches (a primary of one, a spare of another, or under another sharding)
    carries the same record; another epoch or seed another one."""
    one = _plan(tracklets, augmentor=A.P2B_SCALE)
    records = {}
    for number in range(len(one)):
        q = one.plan(EPOCH, number)
        for c, j in enumerate(q['index']):
            rec = (q['aug_map'][c].tobytes(), q['reg_label'][c].tobytes(), q['aug_draws'][c].tobytes())
            assert records.setdefault(int(j), rec) == rec, j
    assert len(records) == 96
    from ptt_amd.train_feed import TrainBatchPlan
    half = TrainBatchPlan(tracklets, batch_size=4, spare=4, rank=1, world=2, seed=SEED, augmentor=A.P2B_SCALE)
    q = half.plan(EPOCH, 5)
    for c, j in enumerate(q['index']):
        assert (q['aug_map'][c].tobytes(), q['reg_label'][c].tobytes(), q['aug_draws'][c].tobytes()) == records[int(j)]
    other = one.plan(EPOCH + 1, 0)
    j = int(other['index'][0])
    assert other['aug_draws'][0].tobytes() != records[j][2]
    # the stream is RandomState([seed, epoch, index, 0x415547]), consumed in queue order
    rs = np.random.RandomState([SEED, EPOCH + 1, j, 0x415547])
    flag = rs.choice([False, True], replace=False, p=[0.5, 0.5])
    angle = rs.uniform(-0.78539816, 0.78539816)
    scale = rs.uniform(0.95, 1.05)
    assert other['aug_draws'][0].tolist() == [float(flag), angle, scale]


def test_draw_statistics_over_4096_indices(tracklets):
    cfg = [{'NAME': 'random_world_flip', 'ALONG_AXIS_LIST': ['x', 'y']}, A.P2B[1], A.SCALE]
    plan = _plan(tracklets, augmentor=cfg)
    n = 4096
    amap, reg, draws = plan._augmentation(EPOCH, np.arange(n), np.zeros((n, 4)))
    assert draws.shape == (n, 4) and plan.aug_kinds == ('flip_x', 'flip_y', 'rotation', 'scaling')
    for col in (0, 1):
        assert set(np.unique(draws[:, col])) == {0.0, 1.0}
        assert abs(draws[:, col].mean() - 0.5) <= 4 * 0.5 / np.sqrt(n), col
    lo, hi = -0.78539816, 0.78539816
    assert draws[:, 2].min() >= lo and draws[:, 2].max() < hi
    assert abs(draws[:, 2].mean() - 0.5 * (lo + hi)) <= 4 * (hi - lo) / np.sqrt(12.0) / np.sqrt(n)
    assert draws[:, 3].min() >= 0.95 and draws[:, 3].max() < 1.05
    assert abs(draws[:, 3].mean() - 1.0) <= 4 * 0.1 / np.sqrt(12.0) / np.sqrt(n)
    # every map is a rotation / reflection times its scale
    det = amap[:, 0].astype(np.float64) * amap[:, 3] - amap[:, 1].astype(np.float64) * amap[:, 2]
    sign = np.where(draws[:, 0] != draws[:, 1], -1.0, 1.0)
    assert np.allclose(det, sign * draws[:, 3] ** 2, rtol=1e-6, atol=0) and np.array_equal(amap[:, 4], draws[:, 3].astype(np.float32))


# ------------------------------------------------------------------ configs
def test_from_config_and_config_handling(tracklets):
    from ptt_amd.train_feed import TrainBatchPlan
    cfg = dict(SEARCH_INPUT_SIZE=256, TEMPLATE_INPUT_SIZE=128, DATA_AUGMENTOR={'AUG_CONFIG_LIST': A.P2B})
    plan = TrainBatchPlan.from_config(tracklets, cfg, 8, spare=4, seed=SEED, rank=0, world=1)
    assert plan.aug_kinds == ('flip_x', 'rotation') and (plan.S, plan.T) == (256, 128)
    assert TrainBatchPlan.config_args(dict(SEARCH_INPUT_SIZE=256))['augmentor'] is None
    assert TrainBatchPlan.from_config(tracklets, dict(SEARCH_INPUT_SIZE=256), 8, spare=4, rank=0, world=1).aug_steps is None
    # a scalar angle is [-a, a]
    scalar = _plan(tracklets, augmentor=[{'NAME': 'random_world_rotation', 'WORLD_ROT_ANGLE': 0.5}])
    assert scalar.aug_steps == [('rotation', [-0.5, 0.5])]
    q = scalar.plan(EPOCH, 0)
    j = int(q['index'][0])
    assert q['aug_draws'][0, 0] == np.random.RandomState([SEED, EPOCH, j, 0x415547]).uniform(-0.5, 0.5)
    # a no-op scale draws nothing: the next entry's draw is the generator's first
    noop = _plan(tracklets, augmentor=[{'NAME': 'random_world_scaling', 'WORLD_SCALE_RANGE': [1.0, 1.0005]}, A.P2B[1]])
    assert noop.aug_kinds == ('rotation',)
    q = noop.plan(EPOCH, 0)
    assert q['aug_draws'][0, 0] == np.random.RandomState([SEED, EPOCH, j, 0x415547]).uniform(-0.78539816, 0.78539816)
    assert np.array_equal(q['aug_map'][:, 4], np.ones(12, np.float32))
    # an augmentor that is already built; an empty queue is the identity
    from ptt_amd.datasets.augmentor import DataAugmentor
    assert _plan(tracklets, augmentor=DataAugmentor(None, A.P2B, None)).aug_kinds == ('flip_x', 'rotation')
    q = _plan(tracklets, augmentor=[]).plan(EPOCH, 0)
    assert np.array_equal(q['aug_map'], np.tile(np.array([1, 0, 0, 1, 1], np.float32), (12, 1))) and np.array_equal(q['reg_label'], q['reg_label_raw'])
    # unknown names and axes: at construction
    for bad in ([{'NAME': 'random_world_shear'}], [{'NAME': 'random_world_flip', 'ALONG_AXIS_LIST': ['x', 'z']}]):
        with pytest.raises(ValueError):
            _plan(tracklets, augmentor=bad)
        with pytest.raises(ValueError):
            TrainBatchPlan.from_config(tracklets, dict(DATA_AUGMENTOR=bad), 8, spare=4, rank=0, world=1)


def test_abi_35_structure(tmp_path):
    """ptt_train_aug: ctypes and numpy agree with what gcc makes of include/ptt_hip.h; the older structures keep their sizes."""
    from ptt_amd import _lib, ops
    import ctypes
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ptt_hip.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(ptt_train_aug));']
    lines += ['printf("%s %%zu\\n", offsetof(ptt_train_aug, %s));' % (f, f) for f, *_r in _lib.TrainAug._fields_]
    (tmp_path / "aug_probe.c").write_text("\n".join(lines + ['return 0;', '}']))
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), str(tmp_path / "aug_probe.c"), "-o", str(tmp_path / "aug_probe")])
    got = dict(l.split() for l in subprocess.check_output([str(tmp_path / "aug_probe")]).decode().splitlines())
    assert int(got["size"]) == 32
    for f, *_r in _lib.TrainAug._fields_:
        assert int(got[f]) == getattr(_lib.TrainAug, f).offset == ops.TRAIN_AUG.fields[f][1], f
    assert ctypes.sizeof(_lib.TrainAug) == 32 and ops.TRAIN_AUG.itemsize == 32
    assert ops.TRAIN_AUG.fields['m'][1] == 0 and ops.TRAIN_AUG.fields['kz'][1] == 16
    assert _lib.ABI_VERSION >= 35 and "ptt_train_batch_aug_f32" in _lib.EXPORTS and "ptt_train_batch_f32" in _lib.EXPORTS
    assert len(_lib.PROTOTYPES["ptt_train_batch_aug_f32"][1]) == 4
    assert ops.TRAIN_CAND.itemsize == 72 and ops.TRAIN_BATCH_DESC.itemsize == 104


def test_each_entry_point_reports_under_its_own_name():
    """The argument checks run before anything touches a device: PTT_EINVAL, and the message names the function that was called."""
    from ptt_amd import _lib, ops
    import ctypes
    lib = _lib.lib()
    desc = np.zeros(1, ops.TRAIN_BATCH_DESC)                    # B = 0
    null, d, one = ctypes.c_void_p(0), ctypes.c_void_p(desc.ctypes.data), ctypes.c_void_p(16)
    einval = _lib.DEFINES.get("PTT_EINVAL", -1)
    assert lib.ptt_train_batch_f32(null, d, null) == einval and lib.ptt_last_error_string().decode() == "ptt_train_batch_f32: null pointer"
    assert lib.ptt_train_batch_aug_f32(null, null, d, null) == einval
    assert lib.ptt_last_error_string().decode() == "ptt_train_batch_aug_f32: null pointer"
    assert lib.ptt_train_batch_aug_f32(one, one, d, null) == einval and lib.ptt_last_error_string().decode().startswith("ptt_train_batch_aug_f32: B=0")
    assert lib.ptt_train_batch_f32(one, d, null) == einval and lib.ptt_last_error_string().decode().startswith("ptt_train_batch_f32: B=0")
