"""Fixture G27 — the REFERENCE's DataAugmentor on small samples (run in the build container against /root/reference, like
make_golden_g21.py; only arrays are committed).

ptt/datasets/augmentor/data_augmentor.py runs the queue of a DATA_AUGMENTOR section through augmentor_utils.py, which draws from
numpy's global generator and rotates through common_utils.rotate_points_along_z. The three files are loaded by path under stub
packages (the dataset package itself asks for a CUDA device at import). G27 = for every (case, seed): numpy's global generator
put into the state of np.random.RandomState([27, case, seed]), DataAugmentor.forward on a 16-point search cloud, an 8-point
template and reg_label[None] — the (1, 4) view on which the reference's functions work (on the (4,) label its own dataset
produces they raise IndexError) — and the draws it made, recorded around np.random.choice / np.random.uniform.

    python tests/golden/make_golden_g27.py        # writes tests/golden/G27_augmentor.npz
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
SEEDS = 6
P2B = [{'NAME': 'random_world_flip', 'ALONG_AXIS_LIST': ['x']},
       {'NAME': 'random_world_rotation', 'WORLD_ROT_ANGLE': [-0.78539816, 0.78539816]}]
CASES = [
    ('p2b', P2B),
    ('flip_xy', [{'NAME': 'random_world_flip', 'ALONG_AXIS_LIST': ['x', 'y']}]),
    ('scalar_angle', [{'NAME': 'random_world_rotation', 'WORLD_ROT_ANGLE': 0.5}]),
    ('scaling', [{'NAME': 'random_world_scaling', 'WORLD_SCALE_RANGE': [0.95, 1.05]}]),
    ('noop_scale', [{'NAME': 'random_world_scaling', 'WORLD_SCALE_RANGE': [1.0, 1.0005]},
                    {'NAME': 'random_world_flip', 'ALONG_AXIS_LIST': ['y']}]),
    ('scale_rot_flip', [{'NAME': 'random_world_scaling', 'WORLD_SCALE_RANGE': [0.9, 1.1]},
                        {'NAME': 'random_world_rotation', 'WORLD_ROT_ANGLE': [-0.3, 0.6]},
                        {'NAME': 'random_world_flip', 'ALONG_AXIS_LIST': ['y', 'x']}]),
    ('repeated', P2B + [{'NAME': 'random_world_flip', 'ALONG_AXIS_LIST': ['x']},
                        {'NAME': 'random_world_rotation', 'WORLD_ROT_ANGLE': [-0.78539816, 0.78539816]}]),
]


class AttrDict(dict):
    __getattr__ = dict.__getitem__


def load_reference():
    """The reference's DataAugmentor class, its modules living under the stub packages refptt.utils / refptt.datasets.augmentor."""
    for name in ("refptt", "refptt.utils", "refptt.datasets", "refptt.datasets.augmentor"):
        pkg = types.ModuleType(name)
        pkg.__path__ = []
        sys.modules[name] = pkg
    mods = {}
    for name, path in (("refptt.utils.common_utils", "ptt/utils/common_utils.py"),
                       ("refptt.datasets.augmentor.augmentor_utils", "ptt/datasets/augmentor/augmentor_utils.py"),
                       ("refptt.datasets.augmentor.data_augmentor", "ptt/datasets/augmentor/data_augmentor.py")):
        spec = importlib.util.spec_from_file_location(name, os.path.join(REF, path))
        mods[name] = sys.modules[name] = importlib.util.module_from_spec(spec)
        parent, _, leaf = name.rpartition(".")
        setattr(sys.modules[parent], leaf, mods[name])
        spec.loader.exec_module(mods[name])
    return mods["refptt.datasets.augmentor.data_augmentor"].DataAugmentor


def main():
    DataAugmentor = load_reference()
    draws = []
    real_choice, real_uniform = np.random.choice, np.random.uniform

    def choice(*a, **kw):
        draws.append(float(real_choice(*a, **kw)))
        return bool(draws[-1])

    def uniform(*a, **kw):
        draws.append(real_uniform(*a, **kw))
        return draws[-1]

    out = {"seeds": SEEDS, "cases": np.array([name for name, _ in CASES])}
    flips = {'x': set(), 'y': set()}
    np.random.choice, np.random.uniform = choice, uniform
    try:
        for ci, (name, cfg) in enumerate(CASES):
            out["cfg_%s" % name] = np.array(json.dumps(cfg))
            aug = DataAugmentor(None, [AttrDict(e) for e in cfg], None)
            for s in range(SEEDS):
                rs = np.random.RandomState([27, ci, s])
                search = (rs.standard_normal((16, 3)) * [3.0, 2.0, 0.7]).astype(np.float32)
                template = (rs.standard_normal((8, 3)) * [2.0, 1.0, 0.7]).astype(np.float32)
                reg = rs.uniform(-0.5, 0.5, 4)
                key = "%s_%d_" % (name, s)
                out[key + "search_in"], out[key + "template_in"], out[key + "reg_in"] = search, template, reg
                np.random.set_state(np.random.RandomState([27, ci, s]).get_state())
                del draws[:]
                d = aug.forward({'search_points': search.copy(), 'template_points': template.copy(), 'reg_label': reg.copy()[None]})
                assert d['search_points'].dtype == np.float32 and d['reg_label'].shape == (1, 4) and d['reg_label'].dtype == np.float64
                out[key + "search_out"], out[key + "template_out"] = d['search_points'], d['template_points']
                out[key + "reg_out"], out[key + "draws"] = d['reg_label'][0], np.array(draws, np.float64)
                k = 0
                for e in cfg:                                    # which draw is which flip: the queue's order
                    if e['NAME'] == 'random_world_flip':
                        for axis in e['ALONG_AXIS_LIST']:
                            flips[axis].add(bool(draws[k]))
                            k += 1
                    elif e['NAME'] == 'random_world_rotation' or e['WORLD_SCALE_RANGE'][1] - e['WORLD_SCALE_RANGE'][0] >= 1e-3:
                        k += 1
                assert k == len(draws), (name, s, k, len(draws))
    finally:
        np.random.choice, np.random.uniform = real_choice, real_uniform
    assert flips == {'x': {False, True}, 'y': {False, True}}, flips
    np.savez_compressed(os.path.join(HERE, "G27_augmentor.npz"), **out)
    print("G27 written: %d cases x %d seeds" % (len(CASES), SEEDS))


if __name__ == "__main__":
    main()
