"""TEST INFRASTRUCTURE — what tests/test_train_augment_{cpu,gpu}.py share: the queues they run, the host mirror
(ptt_amd.datasets.augmentor, itself held to the reference by fixture G27) replayed on the draws of a plan, and the error bounds
between the mirror's sequential float32 arithmetic and the composite map the plan forms and the kernel applies.

Bounds, u = 2^-24 (float32's unit roundoff), k = the product of the queue's scale factors, (x, y, z) the row BEFORE augmentation:
  x, y  each side carries at most six roundings (cos / sin, two products, the sum, the scale and its cast), each at most
        u (|x| + |y|) k, and between two sides at most twelve; 16 leaves room for their second-order terms;
  z     only ever meets the scales. With at most one scaling both sides compute the one float32 product float32(s) * z (or leave z
        alone): BITWISE. With two or more the mirror rounds after every product, the composite once: |dz| <= 4 u |z| k.
Queues without a rotation are flips (exact) and one float32 product by float32(s) on both sides: bitwise throughout."""
import numpy as np

U = 2.0 ** -24
P2B = [{'NAME': 'random_world_flip', 'ALONG_AXIS_LIST': ['x']},
       {'NAME': 'random_world_rotation', 'WORLD_ROT_ANGLE': [-0.78539816, 0.78539816]}]
SCALE = {'NAME': 'random_world_scaling', 'WORLD_SCALE_RANGE': [0.95, 1.05]}
FLIP_SCALE = [{'NAME': 'random_world_flip', 'ALONG_AXIS_LIST': ['x', 'y']}, SCALE]
P2B_SCALE = P2B + [SCALE]
TWO_SCALES = [SCALE] + P2B + [{'NAME': 'random_world_scaling', 'WORLD_SCALE_RANGE': [0.8, 1.25]}]


class ReplayDraws(object):
    """A stand-in `rng` that hands out recorded draws in order (flags as anything truthy): runs the mirror on the draws of
    another run, e.g. one row of TrainBatchPlan.plan()['aug_draws']."""

    def __init__(self, values):
        self.values = list(values)

    def choice(self, *args, **kw):
        return bool(self.values.pop(0))

    def uniform(self, *args, **kw):
        return float(self.values.pop(0))


def scale_product(kinds, draws):
    return float(np.prod([d for kind, d in zip(kinds, draws) if kind == 'scaling'] + [1.0]))


def scalings(kinds):
    """How many scalings a queue draws (no-op ranges draw none and scale nothing)."""
    return list(kinds).count('scaling')


def mirror(cfg, draws, search, template, reg):
    """DataAugmentor.forward on copies, drawing `draws` (one row of plan()['aug_draws']) -> (search, template, reg_label)."""
    from ptt_amd.datasets.augmentor import DataAugmentor
    rng = ReplayDraws(draws)
    d = DataAugmentor(None, cfg, None).forward({'search_points': np.array(search, np.float32), 'template_points': np.array(template, np.float32),
                                                'reg_label': np.array(reg, np.float64)}, rng=rng)
    assert not rng.values, "the mirror left draws unused"
    return d['search_points'], d['template_points'], d['reg_label']


def apply_map(amap, pts):
    """One aug_map record on (n, 3) float32 rows, in float32, as the kernel does (without its fused multiply-add)."""
    m = np.asarray(amap, np.float32)
    p = np.asarray(pts, np.float32)
    return np.stack([m[0] * p[:, 0] + m[1] * p[:, 1], m[2] * p[:, 0] + m[3] * p[:, 1], m[4] * p[:, 2]], 1)


def assert_points_within(got, expect, before, k, factor_xy, n_scalings, what):
    """|dx|, |dy| <= factor_xy u (|x| + |y|) k; z bitwise when the queue has at most one scaling, |dz| <= 4 u |z| k otherwise.
    (x, y, z) = `before`; k a number or one per row."""
    bound_xy = factor_xy * U * (np.abs(np.asarray(before, np.float64)[:, 0]) + np.abs(np.asarray(before, np.float64)[:, 1])) * k
    err = np.abs(np.asarray(got, np.float64) - np.asarray(expect, np.float64))
    assert (err[:, 0] <= bound_xy).all() and (err[:, 1] <= bound_xy).all(), (what, float((err[:, :2] / np.maximum(bound_xy, 1e-300)[:, None]).max()))
    if n_scalings <= 1:
        assert np.array_equal(np.asarray(got)[:, 2], np.asarray(expect)[:, 2]), (what, 'z: not bitwise', float(err[:, 2].max()))
    else:
        bound_z = 4 * U * np.abs(np.asarray(before, np.float64)[:, 2]) * k
        assert (err[:, 2] <= bound_z).all(), (what, 'z', float((err[:, 2] / np.maximum(bound_z, 1e-300)).max()))


def assert_centre_within(got, expect, before, k, factor_xy, what):
    """reg_label's centre, plan (float64 throughout) against mirror: the mirror's rotation takes the centre through float32 as the
    reference's does, the plan does not — a stated departure. x, y as for points; z is rounded to float32 by the mirror's
    rotation (u |z|, idempotent over repeated rotations) and scaled in float64 on both sides: |dz| <= 4 u |z| k, never
    claimed bitwise. Rows: (n, 3)."""
    got, expect, before = (np.asarray(a, np.float64) for a in (got, expect, before))
    bound_xy = factor_xy * U * (np.abs(before[:, 0]) + np.abs(before[:, 1])) * k
    bound_z = 4 * U * np.abs(before[:, 2]) * k
    err = np.abs(got - expect)
    assert (err[:, 0] <= bound_xy).all() and (err[:, 1] <= bound_xy).all(), (what, float((err[:, :2] / np.maximum(bound_xy, 1e-300)[:, None]).max()))
    assert (err[:, 2] <= bound_z).all(), (what, 'z', float((err[:, 2] / np.maximum(bound_z, 1e-300)).max()))


def expected_batch(ref, plan, cfg):
    """tests/train_feed_ref.batch's un-augmented batch `ref` with the mirror applied per slot on the draws of its source's dataset
    index -> a dict with the keys of `ref` (points, reg_label replaced; the rest shared) plus 'k' (per slot)."""
    out = dict(ref)
    out['search_points'], out['template_points'] = ref['search_points'].copy(), ref['template_points'].copy()
    out['reg_label'] = ref['reg_label'].copy()
    out['k'] = np.ones(len(ref['src']))
    for b, src in enumerate(ref['src']):
        if src < 0:
            continue
        assert plan['index'][src] == ref['index'][src]
        draws = plan['aug_draws'][src]
        s, t, reg = mirror(cfg, draws, ref['search_points'][b], ref['template_points'][b], plan['reg_label_raw'][src])
        out['search_points'][b], out['template_points'][b], out['reg_label'][b] = s, t, reg.astype(np.float32)
        out['k'][b] = scale_product(plan['aug_kinds'], draws)
    return out
