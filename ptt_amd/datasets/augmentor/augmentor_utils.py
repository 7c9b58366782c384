"""ptt.datasets.augmentor.augmentor_utils on the host: the four world augmentations of a training sample,

    data_dict = {'search_points': (n, 3+) float32, 'template_points': (m, 3+) float32, 'reg_label': [x, y, z, theta], ...}

changed in place and returned, as the reference's functions do. Each takes one keyword the reference does not have, `rng`
(default numpy's global generator, which is what the reference draws from): the draws are rng.choice([False, True],
replace=False, p=[0.5, 0.5]) per flip and rng.uniform(lo, hi) per rotation / scaling, so a RandomState in the state of numpy's
global generator reproduces the reference's draws bit for bit.

One departure: `reg_label` may be the (4,) array crop_center_pc returns (the reference indexes reg_label[:, 1] and raises on
it); it is then treated as its (1, 4) view and comes back as (4,). An (n, 4) array works as in the reference.

The reference's conventions are kept as they are: flip "along x" negates y and theta, flip "along y" negates x and maps theta to
-(theta + pi); a positive rotation angle turns x towards y, with float32 cos / sin of the float32 angle applied in float32
(common_utils.rotate_points_along_z goes through torch's .float()) — the label's centre passes through float32 there too, while
theta and the scaled centre stay in the label's own precision."""
import numpy as np

POINT_KEYS = ('search_points', 'template_points')


def draw_flag(rng):
    """One flip decision, in the reference's call."""
    return bool(rng.choice([False, True], replace=False, p=[0.5, 0.5]))


def draw_uniform(rng, value_range):
    return rng.uniform(value_range[0], value_range[1])


def scaling_is_noop(scale_range):
    """global_scaling returns its input untouched, and draws nothing, for a range narrower than 1e-3."""
    return scale_range[1] - scale_range[0] < 1e-3


def _label_rows(data_dict):
    """reg_label as (n, 4) rows that write through to the caller's array."""
    reg = data_dict['reg_label']
    if reg.ndim == 1:
        rows = reg.reshape(1, -1)
        if not np.shares_memory(rows, reg):
            raise ValueError("reg_label of shape %s cannot be viewed as one row" % (reg.shape,))
        return rows
    return reg


def rotate_z_f32(points, angle):
    """(n, 3+) -> (n, 3+) float32: columns 0, 1 turned by `angle` about z in float32 arithmetic, the others passed through."""
    a = np.float32(angle)
    c, s = np.cos(a), np.sin(a)
    p = np.asarray(points).astype(np.float32)
    x, y = p[:, 0].copy(), p[:, 1].copy()
    p[:, 0] = x * c - y * s
    p[:, 1] = x * s + y * c
    return p


def _flip(data_dict, column, theta_of, rng):
    if draw_flag(rng):
        reg = _label_rows(data_dict)
        for key in POINT_KEYS:
            data_dict[key][:, column] = -data_dict[key][:, column]
        reg[:, column] = -reg[:, column]
        reg[:, -1] = theta_of(reg[:, -1])
    return data_dict


def random_flip_along_x(data_dict, rng=np.random):
    return _flip(data_dict, 1, lambda theta: -theta, rng)


def random_flip_along_y(data_dict, rng=np.random):
    return _flip(data_dict, 0, lambda theta: -(theta + np.pi), rng)


def global_rotation(data_dict, rot_range, rng=np.random):
    angle = draw_uniform(rng, rot_range)
    reg = _label_rows(data_dict)
    for key in POINT_KEYS:
        data_dict[key] = rotate_z_f32(data_dict[key], angle)
    reg[:, 0:3] = rotate_z_f32(reg[:, 0:3], angle)
    reg[:, -1] += angle
    return data_dict


def global_scaling(data_dict, scale_range, rng=np.random):
    if scaling_is_noop(scale_range):
        return data_dict
    scale = draw_uniform(rng, scale_range)
    reg = _label_rows(data_dict)
    for key in POINT_KEYS:
        data_dict[key][:, :3] *= scale
    reg[:, :3] *= scale
    return data_dict
