"""Feature-space furthest point sampling ('ffps'): the numpy definition against the reference's matrix formula, and what the
binding, the C entry point's argument checks and the SA module answer without a device."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import dense_ref as R
from tests import ffps_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _matrix_picks(xyz, feat, npoint):
    """The reference's formula (pointnet2_modules.py:64-67): square_distance(cat, cat) -> FPS on the matrix."""
    cat = torch.cat([torch.from_numpy(xyz).transpose(1, 2), torch.from_numpy(feat)], dim=1).transpose(1, 2).contiguous()
    return ffps_ref.fps_with_dist(R.square_distance(cat, cat).numpy(), npoint)


@pytest.mark.parametrize("N,C,npoint", [(64, 8, 32), (256, 128, 128), (200, 37, 77)])
def test_definition_equals_matrix_formula_on_exact_clouds(N, C, npoint):
    """Multiples of 1/4 in [-4, 4]: every partial sum is exact in float32 in any order, so torch's unspecified summation order
    of sum(dim=-1) cannot matter and the picks must be the matrix formula's, all distinct."""
    xyz, feat = ffps_ref.exact_cloud(np.random.RandomState(N + C), 2, N, C)
    got = ffps_ref.ffps(xyz, feat, npoint)
    assert got.dtype == np.int32 and got.shape == (2, npoint)
    assert np.array_equal(got, _matrix_picks(xyz, feat, npoint))
    for b in range(2):
        assert len(set(got[b].tolist())) == npoint and got[b, 0] == 0


def test_ties_lowest_index():
    rs = np.random.RandomState(5)
    xyz = rs.randint(-1, 2, (2, 256, 3)).astype(np.float32)
    feat = rs.randint(-1, 2, (2, 3, 256)).astype(np.float32)
    got = ffps_ref.ffps(xyz, feat, 64)
    assert np.array_equal(got, _matrix_picks(xyz, feat, 64))
    # the tie rule itself, by hand: the first pick after index 0 is the lowest index at the largest distance from point 0
    v = np.concatenate([xyz[0], feat[0].T], axis=1)
    d0 = ((v - v[0]) ** 2).sum(-1)
    assert got[0, 1] == int(np.flatnonzero(d0 == d0.max())[0])


def test_duplicated_rows_and_identical_cloud():
    rs = np.random.RandomState(6)
    xyz, feat = ffps_ref.exact_cloud(rs, 2, 40, 5)
    src = rs.randint(0, 40, (2, 120))
    xyz = np.stack([xyz[b][src[b]] for b in range(2)])
    feat = np.stack([feat[b][:, src[b]] for b in range(2)])
    got = ffps_ref.ffps(xyz, feat, 60)
    assert np.array_equal(got, _matrix_picks(xyz, feat, 60))
    for b in range(2):                                              # while a distinct row is left, the next pick is a new one
        row = lambda k: tuple(xyz[b, k]) + tuple(feat[b, :, k])
        n_distinct = len({row(k) for k in range(120)})
        assert n_distinct <= 40 and len({row(k) for k in got[b, :n_distinct]}) == n_distinct
    same_xyz = np.tile(np.float32([[0.5, -1.25, 2.0]]), (2, 33, 1))
    same_feat = np.tile(np.float32([[1.0], [2.0], [-3.0], [0.25]]), (2, 1, 33))
    assert not ffps_ref.ffps(same_xyz, same_feat, 17).any()
    assert not ffps_ref.ffps(same_xyz, None, 17).any()


def test_no_features_is_plain_distance_without_origin_skip():
    """C = 0: (dx*dx + dy*dy) + dz*dz, and points inside the origin ball ARE selectable (the coordinate op skips them)."""
    rs = np.random.RandomState(7)
    xyz = rs.standard_normal((1, 50, 3)).astype(np.float32)
    xyz[0, 10:20] *= np.float32(1e-3)
    got = ffps_ref.ffps(xyz, None, 50)
    assert sorted(got[0].tolist()) == list(range(50))
    d = xyz[0, 3] - xyz[0]
    assert np.array_equal(ffps_ref.dist_row(xyz[0], 3), (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def test_abi_declares_and_exports_ffps():
    from ptt_amd import _lib
    assert _lib.ABI_VERSION >= 29
    assert "ptt_ffps_f32" in _lib.EXPORTS
    restype, argtypes = _lib.PROTOTYPES["ptt_ffps_f32"]
    assert restype is ctypes.c_int and len(argtypes) == 11
    assert argtypes[2:5] == [ctypes.c_int64] * 3 and argtypes[5:9] == [ctypes.c_int] * 4
    assert os.path.exists(_lib.LIB_PATH), "run `python -m ptt_amd.build` first"
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "ptt_ffps_f32")


def test_argument_checks_come_before_any_runtime_call():
    """Null pointers / sizes below 1 -> PTT_EINVAL, sizes beyond the documented limits -> PTT_EUNSUPPORTED, with a null stream and
    host addresses that are never dereferenced: the checks precede every runtime call, so this needs no device."""
    from ptt_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    fn = lib.ptt_ffps_f32
    fn.restype, fn.argtypes = _lib.PROTOTYPES["ptt_ffps_f32"]
    lib.ptt_last_error_string.restype = ctypes.c_char_p
    einval, eunsup = _lib.DEFINES.get("PTT_EINVAL", -1), _lib.DEFINES.get("PTT_EUNSUPPORTED", -2)
    assert (einval, eunsup) == (-1, -2)
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    call = lambda xyz, feat, B, N, C, npoint, out: fn(xyz, feat, C * N, N, 1, B, N, C, npoint, out, None)
    assert call(None, p, 1, 4, 1, 2, p) == einval
    assert call(p, None, 1, 4, 1, 2, p) == einval                   # features missing with C > 0
    assert call(p, p, 1, 4, 1, 2, None) == einval
    assert call(p, p, 1, 0, 1, 1, p) == einval
    assert call(p, p, 0, 4, 1, 2, p) == einval
    assert call(p, p, 1, 4, 1, 0, p) == einval
    assert call(p, p, 1, 4, -1, 2, p) == einval
    assert call(p, p, 1, 4, 1025, 2, p) == eunsup
    assert b"1024" in lib.ptt_last_error_string()
    assert call(p, p, 1, 16385, 1, 2, p) == eunsup
    assert call(p, p, 1, 16384, 1, 15361, p) == eunsup
    assert fn(p, p, 0, 2 ** 20, 2 ** 20, 1, 4096, 4, 2, p, None) == eunsup     # a cloud's features beyond 2^31 elements


def test_cpu_tensors_are_refused():
    from ptt_amd import ops
    xyz, feat = torch.zeros(1, 8, 3), torch.zeros(1, 2, 8)
    with pytest.raises(RuntimeError, match="CPU tensors are not supported"):
        ops.feature_fps(xyz, feat, 4)


def test_ffps_level_without_features_raises_value_error():
    from ptt_amd.models.backbones_3d.pointnet2.pointnet2_modules import PointnetSAModuleVotes
    sa = PointnetSAModuleVotes(mlp=[0, 16, 16], radius=0.5, nsample=16, sample_method='ffps').eval()
    with pytest.raises(ValueError, match="without point features"):
        sa(torch.zeros(1, 32, 3), None, 8)
