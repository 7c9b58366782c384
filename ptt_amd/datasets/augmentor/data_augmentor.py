"""ptt.datasets.augmentor.data_augmentor.DataAugmentor: the queue of world augmentations a DATA_AUGMENTOR config lists, run in
order on a sample's data_dict (augmentor_utils). Every entry is parsed once, at construction, into (NAME, argument); the queue
and TrainBatchPlan both work from that list (`steps`)."""
import numpy as np

from . import augmentor_utils

FLIPS = {'x': augmentor_utils.random_flip_along_x, 'y': augmentor_utils.random_flip_along_y}


def _flip(data_dict, axes, rng):
    for axis in axes:
        data_dict = FLIPS[axis](data_dict, rng=rng)
    return data_dict


def _rotation(data_dict, rot_range, rng):
    return augmentor_utils.global_rotation(data_dict, rot_range, rng=rng)


def _scaling(data_dict, scale_range, rng):
    return augmentor_utils.global_scaling(data_dict, scale_range, rng=rng)


OPERATIONS = {'random_world_flip': _flip, 'random_world_rotation': _rotation, 'random_world_scaling': _scaling}
NAMES = tuple(OPERATIONS)


def config_list(augmentor_configs):
    """The entries of a DATA_AUGMENTOR section: a list of them, or a mapping / namespace with AUG_CONFIG_LIST."""
    if isinstance(augmentor_configs, (list, tuple)):
        return list(augmentor_configs)
    if isinstance(augmentor_configs, dict):
        return list(augmentor_configs['AUG_CONFIG_LIST'])
    return list(augmentor_configs.AUG_CONFIG_LIST)


def _pair(value, what):
    pair = [float(v) for v in value]
    if len(pair) != 2:
        raise ValueError("%s must be [low, high], got %r" % (what, value))
    return pair


def parse_entry(cfg, name=None):
    """One entry -> (NAME, argument): the axes of a flip, the [low, high] of a rotation (a scalar a reads as [-a, a]) or of a
    scaling. Raises ValueError for a NAME or an axis the augmentor does not have. name: taken instead of cfg['NAME']."""
    name = cfg['NAME'] if name is None else name
    if name not in OPERATIONS:
        raise ValueError("DATA_AUGMENTOR: unknown NAME %r (one of %s)" % (name, ", ".join(NAMES)))
    if name == 'random_world_flip':
        axes = list(cfg['ALONG_AXIS_LIST'])
        for axis in axes:
            if axis not in FLIPS:
                raise ValueError("random_world_flip: axis %r in ALONG_AXIS_LIST (x or y)" % (axis,))
        return name, axes
    if name == 'random_world_rotation':
        rot = cfg['WORLD_ROT_ANGLE']
        return name, _pair(rot, 'WORLD_ROT_ANGLE') if isinstance(rot, (list, tuple)) else [-float(rot), float(rot)]
    return name, _pair(cfg['WORLD_SCALE_RANGE'], 'WORLD_SCALE_RANGE')


class Step(object):
    """One parsed entry as a callable: step(data_dict, rng=np.random) -> data_dict."""

    def __init__(self, name, argument):
        self.name, self.argument = name, argument

    def __call__(self, data_dict, rng=np.random):
        return OPERATIONS[self.name](data_dict, self.argument, rng)


class DataAugmentor(object):
    """DataAugmentor(root_path, augmentor_configs, class_names, logger=None), as the reference's. augmentor_configs: a list of
    entries or a mapping / namespace with AUG_CONFIG_LIST; an entry is a mapping (EasyDict or dict) with NAME and the NAME's
    setting. forward(data_dict) runs the queue; the three random_world_* methods run one entry on a data_dict, or, called
    without one, hand back the entry as a callable (how the reference fills its queue). rng: where the draws come from —
    numpy's global generator as in the reference, or a RandomState."""

    def __init__(self, root_path, augmentor_configs, class_names, logger=None):
        self.root_path, self.class_names, self.logger = root_path, class_names, logger
        self.steps = [parse_entry(cfg) for cfg in config_list(augmentor_configs)]
        self.data_augmentor_queue = [Step(name, argument) for name, argument in self.steps]

    def __getstate__(self):
        return {key: value for key, value in vars(self).items() if key != 'logger'}

    def __setstate__(self, state):
        vars(self).update(state)

    def _entry(self, name, data_dict, config, rng):
        step = Step(*parse_entry(config, name))
        return step if data_dict is None else step(data_dict, rng=rng)

    def random_world_flip(self, data_dict=None, config=None, rng=np.random):
        return self._entry('random_world_flip', data_dict, config, rng)

    def random_world_rotation(self, data_dict=None, config=None, rng=np.random):
        return self._entry('random_world_rotation', data_dict, config, rng)

    def random_world_scaling(self, data_dict=None, config=None, rng=np.random):
        return self._entry('random_world_scaling', data_dict, config, rng)

    def forward(self, data_dict, rng=np.random):
        """Run the queue on `data_dict` (changed in place and returned)."""
        for step in self.data_augmentor_queue:
            data_dict = step(data_dict, rng=rng)
        return data_dict
