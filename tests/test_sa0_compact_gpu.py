"""SA0 on the balls' distinct rows (ptt_sa_desc.compact_ws, sa_compact_kernel + the compact mode of sa_lds_kernel): the
pooled output is bitwise the dense one (every one of the 32 grouped rows), and the ball table the compaction pass
writes equals a numpy restatement of it (include/ptt_hip.h documents the layout)."""
import numpy as np
import pytest
import torch

from ptt_amd import _lib, ops, synth
from tests.util import fold_layers, mlp_layers

pytestmark = pytest.mark.gpu

NS = 32
HDR = 16


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def layers(dev):
    # the SA0 shape the compact mode serves: 3 -> 64 -> 64 -> 128, BatchNorm folded into the weights
    return fold_layers(mlp_layers(7, [3, 64, 64, 128]), dev, ops, scale_in_weights=True)


def _workspace(B, M, dev):
    n = _lib.lib().ptt_sa_compact_workspace(B, M)
    return torch.full(((n + 3) // 4,), -7, dtype=torch.int32, device=dev)    # poison: nothing may read unwritten words


def _run(xyz, new_xyz, idx, layers, radius, compact, normalize=True):
    out = ops.sa_fused_forward(xyz, new_xyz, idx, None, layers, radius, True, normalize, point_major_out=True,
                               compact=compact)
    torch.cuda.synchronize()
    return out


def _expected_table(xyz, idx):
    """numpy restatement: per ball its distinct neighbours (first occurrences of the (x, y, z) bit patterns, slot order)."""
    bits = xyz.view(np.uint32)
    B, M, _ = idx.shape
    balls = []
    for b in range(B):
        for m in range(M):
            seen, keep = set(), []
            for n in idx[b, m]:
                key = tuple(bits[b, n])
                if key not in seen:
                    seen.add(key)
                    keep.append(int(n))
            balls.append(keep)
    return balls


def _check_table(ws, xyz, idx):
    B, M, _ = idx.shape
    T = B * M
    w = ws.cpu().numpy()
    balls = _expected_table(xyz, idx)
    nd = np.array([len(k) for k in balls])
    cls = np.select([nd <= 4, nd <= 8, nd <= 16], [0, 1, 2], 3)
    np.testing.assert_array_equal(w[HDR:HDR + T], nd)
    for k in range(4):
        c = 4 << k
        n_k = int(w[k])
        assert n_k == int((cls == k).sum()), k
        lst = w[HDR + (1 + k) * T: HDR + (1 + k) * T + n_k]
        np.testing.assert_array_equal(np.sort(lst), np.flatnonzero(cls == k))      # every ball once, order free
        rows = w[HDR + 5 * T + (c - 4) * T: HDR + 5 * T + (c - 4) * T + n_k * c].reshape(n_k, c)
        for q, g in enumerate(lst):
            keep = balls[g]
            np.testing.assert_array_equal(rows[q], keep + [keep[0]] * (c - len(keep)), err_msg="ball %d" % g)
    return nd


def _ball_inputs(s, M, radius, dev):
    xyz = torch.from_numpy(s).to(dev).contiguous()
    new_xyz, _, idx = ops.centres_ball_query(xyz, None, M, radius, NS)      # 'sequence' sampling: the first M points
    return xyz, new_xyz, idx


CLOUDS = [  # (kind, zero clouds, B, N, M, radius)
    ("car", 0, 1, 2048, 512, 0.3), ("car", 0, 48, 2048, 512, 0.3), ("car", 0, 48, 1024, 256, 0.3),
    ("ped", 1, 1, 2048, 512, 0.3), ("ped", 1, 48, 2048, 512, 0.3), ("ped", 1, 48, 1024, 256, 0.3),
    ("dense", 0, 1, 2048, 512, 0.3), ("dense", 0, 48, 2048, 512, 0.3),
]


@pytest.mark.parametrize("kind,zero,B,N,M,radius", CLOUDS)
def test_compact_equals_dense_bitwise(dev, layers, kind, zero, B, N, M, radius):
    K = {"car": 600, "ped": 60, "dense": N}[kind]
    s, _ = synth.frames(11, B, N, 64, K_s=K, kind=kind, zero_clouds=zero)
    xyz, new_xyz, idx = _ball_inputs(s, M, radius, dev)
    dense = _run(xyz, new_xyz, idx, layers, radius, False)
    ws = _workspace(B, M, dev)
    idx_before = idx.clone()
    got = _run(xyz, new_xyz, idx, layers, radius, ws)
    assert torch.equal(idx, idx_before)                   # idx is not modified
    assert torch.equal(got, dense)
    nd = _check_table(ws, s, idx.cpu().numpy())
    if kind != "dense":
        assert nd.mean() < 0.5 * NS                       # the point of the exercise: far fewer rows
    again = _run(xyz, new_xyz, idx, layers, radius, True)
    assert torch.equal(again, got)                        # same launch twice, same bits


def test_compact_stress_geometry(dev, layers):
    s, _ = synth.frames(3, 2, 16384, 64, K_s=16384, kind="dense")
    xyz, new_xyz, idx = _ball_inputs(s, 8192, 0.3, dev)
    dense = _run(xyz, new_xyz, idx, layers, 0.3, False)
    ws = _workspace(2, 8192, dev)
    assert torch.equal(_run(xyz, new_xyz, idx, layers, 0.3, ws), dense)
    _check_table(ws, s, idx.cpu().numpy())


def _hand_built(rs):
    """Balls with exactly 1, 3, 5, 9, 17 and 32 distinct hits, duplicate-only balls, +-0 coordinates, empty balls: idx as
    ball query writes it (ascending hits, then the first hit repeated; an empty ball is all zeros)."""
    N = 160
    base = (rs.uniform(-0.2, 0.2, (N, 3))).astype(np.float32)
    base[100:140] = base[60]                              # 40 copies of one point
    base[140] = [0.0, 0.0, 0.0]
    base[141] = [-0.0, 0.0, 0.0]
    base[142] = [0.0, -0.0, -0.0]
    base[143] = [-0.0, -0.0, -0.0]
    base[144:150] = base[5]                               # more duplicates of an early point
    balls = []

    def ball(hits):
        hits = sorted(hits)
        assert len(hits) <= NS
        balls.append(hits + [hits[0]] * (NS - len(hits)))

    for d in (1, 3, 5, 9, 17, 32):
        ball(list(range(d)))                              # d distinct points
        ball(list(range(10, 10 + d))[:NS])
    ball([60] + list(range(100, 131)))                    # 32 hits, one distinct point
    ball(list(range(100, 110)))                           # 10 hits, one distinct point
    ball([5] + list(range(144, 150)) + list(range(20, 26)))   # 13 hits, 7 distinct
    ball(list(range(140, 144)))                           # +0 / -0 bit patterns: four distinct rows
    ball([140, 141, 2, 3])
    ball([0] * 1)                                         # one hit
    balls.append([0] * NS)                                # empty ball
    balls.append([0] * NS)
    ball([0, 1, 2, 3, 4, 60, 100, 101, 102, 103, 104, 105, 106, 107, 108, 109, 110])   # 17 hits, 6 distinct
    return base, np.array(balls, np.int32)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("normalize", [True, False])
def test_compact_hand_built_balls(dev, layers, B, normalize):
    rs = np.random.RandomState(5)
    clouds, idxs = [], []
    for _ in range(B):
        base, idx = _hand_built(rs)
        clouds.append(base)
        idxs.append(idx)
    s = np.stack(clouds)
    idx_np = np.stack(idxs)
    M = idx_np.shape[1]
    centres = rs.uniform(-0.1, 0.1, (B, M, 3)).astype(np.float32)
    centres[:, 0] = [-0.0, 0.0, -0.0]
    xyz = torch.from_numpy(s).to(dev)
    new_xyz = torch.from_numpy(centres).to(dev)
    idx = torch.from_numpy(idx_np).to(dev)
    dense = _run(xyz, new_xyz, idx, layers, 0.25, False, normalize)
    ws = _workspace(B, M, dev)
    got = _run(xyz, new_xyz, idx, layers, 0.25, ws, normalize)
    assert torch.equal(got, dense)
    nd = _check_table(ws, s, idx_np)
    assert {1, 3, 5, 7, 9, 17, 32} <= set(nd.tolist()) and 4 in nd.tolist()


def test_compact_workspace_too_small_is_an_error(dev, layers):
    s, _ = synth.frames(2, 2, 1024, 64)
    xyz, new_xyz, idx = _ball_inputs(s, 256, 0.3, dev)
    ws = _workspace(2, 128, dev)
    with pytest.raises(RuntimeError):
        _run(xyz, new_xyz, idx, layers, 0.3, ws)
