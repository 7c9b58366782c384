"""The stream shape of ptt_sa_fused_fwd_f32 (hoisted 128-channel layer 0, 128 -> 128 -> 256, 32 neighbours) on the balls'
real hits only (ptt_sa_desc.compact_ws: sa_compact_kernel<false> + sa_stream_compact_kernel): the pooled output is
bitwise the dense kernel's, the ball table equals a numpy restatement (include/ptt_hip.h documents the layout), the call
can be captured, and the hot path enables it on the search branch's last level of large launches only."""
import numpy as np
import pytest
import torch

from ptt_amd import _lib, ops, synth
from ptt_amd.hot_path import FrameHotPath, kitti_model_cfg, randomize_
from ptt_amd.models.backbones_3d.pointnet2 import pointnet2_modules
from tests.util import fold_layers, mlp_layers

pytestmark = pytest.mark.gpu

NS = 32
HDR = 16
SPEC = [131, 128, 128, 256]
# the four stream launches of the 48-frame car step: (points of the level below, centres, radius) -> B * M balls
SHAPES = [(512, 256, 0.5), (256, 128, 0.7), (256, 128, 0.5), (128, 64, 0.7)]      # 12288, 6144, 6144, 3072 balls at B = 48


@pytest.fixture(scope="module")
def params(dev):
    """(remaining layers, xyz weight (3,128)) of a hoisted level with the BatchNorm scale folded into the weights."""
    layers = mlp_layers(17, SPEC)
    folded = fold_layers(layers, dev, ops, scale_in_weights=True)
    rs = np.random.RandomState(3)
    wx = torch.from_numpy((rs.standard_normal((3, 128)) * 0.5).astype(np.float32)).to(dev)
    return folded[1:], wx


def _term(B, N, dev, seed=0):
    rs = np.random.RandomState(1000 + seed)
    return torch.from_numpy(rs.standard_normal((B, N, 128)).astype(np.float32)).to(dev)


def _workspace(B, M, dev):
    n = _lib.lib().ptt_sa_compact_workspace(B, M)
    return torch.full(((n + 3) // 4,), -7, dtype=torch.int32, device=dev)    # poison: nothing may read unwritten words


def _run(xyz, new_xyz, idx, term, params, radius, compact, normalize=True):
    layers, wx = params
    out = ops.sa_fused_forward(xyz, new_xyz, idx, None, layers, radius, True, normalize, point_major_out=True,
                               l0=(term, wx, True), compact=compact)
    torch.cuda.synchronize()
    return out


def _check_table(ws, idx):
    """numpy restatement: slot s of a ball is real iff s == 0 or idx[s] != idx[0]; the real hits in slot order, padded
    with the first one to the class size."""
    B, M, _ = idx.shape
    T = B * M
    w = ws.cpu().numpy()
    flat = idx.reshape(T, NS)
    balls = [[int(r[0])] + [int(v) for v in r[1:] if v != r[0]] for r in flat]
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
    return nd, cls


def _level_inputs(kind, B, N, M, radius, dev, template=False):
    """The level's points as the backbone forms them: furthest point sampling of a synth cloud, then the first N of the
    sample ('sequence' sampling of the levels above), centres = the first M of those."""
    K = (600, 300) if kind == "car" else (60, 40)
    s, t = synth.frames(1000, B, 2048, 1024, K_s=K[0], K_t=K[1], kind=kind, zero_clouds=1 if kind == "ped" else 0)
    cloud = torch.from_numpy(t if template else s).to(dev)
    n0 = 256 if template else 512
    inds = ops.furthest_point_sampling(cloud, n0).long()
    lvl0 = torch.gather(cloud, 1, inds[..., None].expand(-1, -1, 3))
    xyz = lvl0[:, :N].contiguous()
    new_xyz, _, idx = ops.centres_ball_query(xyz, None, M, radius, NS)
    return xyz, new_xyz, idx


@pytest.mark.parametrize("kind", ["car", "ped"])
@pytest.mark.parametrize("shape", range(4))
def test_compact_equals_dense_bitwise(dev, params, kind, shape):
    N, M, radius = SHAPES[shape]
    B = 48
    xyz, new_xyz, idx = _level_inputs(kind, B, N, M, radius, dev, template=shape >= 2)
    term = _term(B, N, dev, shape)
    dense = _run(xyz, new_xyz, idx, term, params, radius, False)
    ws = _workspace(B, M, dev)
    idx_before = idx.clone()
    got = _run(xyz, new_xyz, idx, term, params, radius, ws)
    assert torch.equal(idx, idx_before)                   # idx is not modified
    assert torch.equal(got, dense)
    nd, _ = _check_table(ws, idx.cpu().numpy())
    print("%s shape %d: %d balls, mean real hits %.2f" % (kind, shape, B * M, nd.mean()))
    again = _run(xyz, new_xyz, idx, term, params, radius, True)
    assert torch.equal(again, got)                        # same launch twice, same bits


def _ball(hits):
    return list(hits) + [hits[0]] * (NS - len(hits))


def _hand_built(rs, N, counts):
    """Index table as ball query writes it: `counts[i]` real hits of ball i (distinct points, ascending), then the first
    hit repeated; 0 = an empty ball (all slots 0)."""
    balls = []
    for d in counts:
        if d == 0:
            balls.append([0] * NS)
        else:
            balls.append(_ball(sorted(rs.choice(N, d, replace=False).tolist())))
    return np.array(balls, np.int32)


HAND = {
    # every class, each with a partial last 64-row tile (class 4: 16 balls a tile, 8: 8, 16: 4, 32: 2); B * M odd
    "all_classes": [1, 4, 5, 8, 9, 16, 17, 32, 1, 10, 3, 4, 6, 7, 12, 31, 32, 3, 1, 0, 4, 4, 5, 9, 17, 2, 3],
    # classes 8 and 16 have no ball
    "empty_classes": [1, 4, 32, 3, 2, 32, 32, 1, 4],
    # only class 4, more than one tile, partial last tile
    "one_class": [1, 2, 3, 4] * 9 + [1],
    # exactly full tiles of every class
    "full_tiles": [4] * 16 + [8] * 8 + [16] * 4 + [32] * 2,
}


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", sorted(HAND))
def test_compact_hand_built_balls(dev, params, name, B, normalize):
    rs = np.random.RandomState(5)
    N = 96
    counts = HAND[name]
    M = len(counts)
    idx_np = np.stack([_hand_built(rs, N, counts if b != 1 else counts[::-1]) for b in range(B)])
    s = rs.uniform(-0.4, 0.4, (B, N, 3)).astype(np.float32)
    centres = rs.uniform(-0.2, 0.2, (B, M, 3)).astype(np.float32)
    if B == 3:                                            # an all-zero frame with empty balls only
        s[2] = 0.0
        centres[2] = 0.0
        idx_np[2] = 0
    xyz, new_xyz, idx = (torch.from_numpy(a).to(dev) for a in (s, centres, idx_np))
    term = _term(B, N, dev, 7)
    dense = _run(xyz, new_xyz, idx, term, params, 0.5, False, normalize)
    ws = _workspace(B, M, dev)
    got = _run(xyz, new_xyz, idx, term, params, 0.5, ws, normalize)
    assert torch.equal(got, dense)
    nd, cls = _check_table(ws, idx_np)
    if B == 1:
        assert sorted(nd.tolist()) == sorted(max(c, 1) for c in counts)
    if name == "all_classes":
        assert {1, 4, 5, 8, 9, 16, 17, 32} <= set(nd.tolist()) and (B * M) % 2 == 1
        assert B != 1 or all((cls == k).sum() % (16 >> k) for k in range(4))         # partial last tiles
    if name == "empty_classes" and B == 1:
        assert (cls == 1).sum() == 0 and (cls == 2).sum() == 0


def test_compact_call_is_capturable_and_rebuilds_its_table(dev, params):
    """Captured once, replayed with two other index tables: the table is rebuilt inside the graph, both replays are
    bitwise the eager results."""
    B, N, M, radius = 8, 256, 128, 0.7
    rs = np.random.RandomState(9)
    s = rs.uniform(-1.5, 1.5, (B, N, 3)).astype(np.float32)
    xyz = torch.from_numpy(s).to(dev)
    term = _term(B, N, dev, 9)
    tables = []
    for r in (0.4, 0.7, 1.6):                             # sparse, medium and full balls
        new_xyz, _, idx = ops.centres_ball_query(xyz, None, M, r, NS)
        tables.append(idx.clone())
    eager = [_run(xyz, new_xyz, t, term, params, radius, False).clone() for t in tables]
    idx = tables[0].clone()
    ws = _workspace(B, M, dev)
    _run(xyz, new_xyz, idx, term, params, radius, ws)     # the first call sets the kernel's LDS limit: not inside a capture
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            out = ops.sa_fused_forward(xyz, new_xyz, idx, None, params[0], radius, True, True, point_major_out=True,
                                       l0=(term, params[1], True), compact=ws)
    torch.cuda.current_stream(dev).wait_stream(side)
    for k in (1, 2, 0):
        idx.copy_(tables[k])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager[k]), k
        _check_table(ws, tables[k].cpu().numpy())


def test_compact_workspace_short_or_misaligned_is_an_error(dev, params):
    B, N, M, radius = 2, 256, 128, 0.7
    xyz, new_xyz, idx = _level_inputs("car", B, N, M, radius, dev)
    term = _term(B, N, dev)
    with pytest.raises(RuntimeError, match="PTT_EWORKSPACE"):
        _run(xyz, new_xyz, idx, term, params, radius, _workspace(B, M // 2, dev))
    big = _workspace(B, M + 8, dev)
    with pytest.raises(RuntimeError, match="PTT_EWORKSPACE"):
        _run(xyz, new_xyz, idx, term, params, radius, big[1:])          # 4 bytes off a 16-byte boundary
    assert torch.equal(_run(xyz, new_xyz, idx, term, params, radius, big[4:]),
                       _run(xyz, new_xyz, idx, term, params, radius, False))


class _Spy(object):
    """Records (B * M, compact) of every ops.sa_fused_forward call with a hoisted 128-channel layer 0 (the backbone's levels 1
    and 2; vote aggregation hoists 256 channels)."""

    def __init__(self, monkeypatch):
        self.calls = []
        real = ops.sa_fused_forward

        def spy(xyz, new_xyz, idx, *a, **kw):
            if kw.get("l0") is not None and kw["l0"][0].shape[2] == 128:
                self.calls.append((idx.shape[0] * idx.shape[1], bool(kw.get("compact", False))))
            return real(xyz, new_xyz, idx, *a, **kw)
        monkeypatch.setattr(ops, "sa_fused_forward", spy)


@pytest.mark.parametrize("kind", ["car", "ped"])
def test_hot_path_with_the_level_enabled_is_bitwise_the_dense_one(dev, monkeypatch, kind):
    model = randomize_(FrameHotPath(kitti_model_cfg()), seed=3).to(dev).eval()
    K = (600, 300) if kind == "car" else (60, 40)
    s, t = (torch.from_numpy(a).to(dev) for a in synth.frames(1000, 48, 2048, 1024, K_s=K[0], K_t=K[1], kind=kind))
    spy = _Spy(monkeypatch)
    with torch.no_grad():
        on = {k: v.clone() for k, v in model(s, t).items()}
        torch.cuda.synchronize()
        calls_on, spy.calls = spy.calls, []
        monkeypatch.setattr(pointnet2_modules, "STREAM_COMPACT_MIN_BALLS", 1 << 30)
        off = model(s, t)
        torch.cuda.synchronize()
    # the search branch's last level (48 x 128 balls) alone, and only while the gate lets it
    assert sorted(calls_on) == [(3072, False), (6144, False), (6144, True), (12288, False)]
    assert sorted(spy.calls) == [(3072, False), (6144, False), (6144, False), (12288, False)]
    assert set(on) == set(off)
    for k in on:
        assert torch.equal(on[k], off[k]), k


def test_one_frame_issues_the_same_launches_as_before(dev, monkeypatch):
    """B = 1 (one tracklet frame) stays dense: the same entry points in the same order with the gate at its value and
    with the level disabled, and no compact call."""
    model = randomize_(FrameHotPath(kitti_model_cfg()), seed=3).to(dev).eval()
    s, t = (torch.from_numpy(a).to(dev) for a in synth.frames(1000, 1, 1024, 512))
    names = [n for n in _lib.EXPORTS if n.endswith("_f32") or n.endswith("_jobs")]

    def launches():
        with torch.no_grad():
            model(s, t)                                   # caches, arange tables
            torch.cuda.synchronize()
            ops.start_kernel_timing(names)
            model(s, t)
            return {n: len(v) for n, v in ops.stop_kernel_timing().items() if v}

    assert pointnet2_modules.STREAM_COMPACT_MIN_BALLS > 128        # the search branch's last level of one frame: 128 balls
    spy = _Spy(monkeypatch)
    on = launches()
    assert spy.calls and not any(c for _, c in spy.calls)
    monkeypatch.setattr(pointnet2_modules, "STREAM_COMPACT_MIN_BALLS", 1 << 30)
    assert launches() == on


@pytest.mark.parametrize("B,expect", [
    (8, [(512, False), (1024, False), (1024, False), (2048, False)]),      # 8 x 128 = 1024 balls: below the gate, dense
    (16, [(1024, False), (2048, False), (2048, True), (4096, False)]),     # 16 x 128 = 2048 balls: the gate's value, compact
])
def test_hot_path_gate_at_its_threshold(dev, monkeypatch, B, expect):
    """Either side of STREAM_COMPACT_MIN_BALLS on FrameHotPath: which launch is compacted (the search branch's last level,
    never level 1 whatever its ball count), and the outputs are bitwise those of the all-dense path."""
    assert pointnet2_modules.STREAM_COMPACT_MIN_BALLS == 2048
    model = randomize_(FrameHotPath(kitti_model_cfg()), seed=4).to(dev).eval()
    s, t = (torch.from_numpy(a).to(dev) for a in synth.frames(1000, B, 2048, 1024))
    spy = _Spy(monkeypatch)
    with torch.no_grad():
        on = {k: v.clone() for k, v in model(s, t).items()}
        torch.cuda.synchronize()
        assert sorted(spy.calls) == expect
        monkeypatch.setattr(pointnet2_modules, "STREAM_COMPACT_MIN_BALLS", 1 << 30)
        off = model(s, t)
        torch.cuda.synchronize()
    for k in on:
        assert torch.equal(on[k], off[k]), k


@pytest.mark.parametrize("N,expect", [(512, True), (1024, True), (2048, False)])
def test_module_keyword_honours_the_points_gate(dev, monkeypatch, N, expect):
    """PointnetSAModuleVotes.forward(compact=True): 2048 balls in every case, compact only up to STREAM_COMPACT_MAX_POINTS points
    per cloud; same values either way."""
    from ptt_amd.models.backbones_3d.pointnet2.pointnet2_modules import PointnetSAModuleVotes
    m = randomize_(PointnetSAModuleVotes(mlp=[128, 128, 128, 256], radius=0.5, nsample=32, normalize_xyz=True,
                                         sample_method='sequence'), seed=5).to(dev).eval()
    s, _ = synth.frames(9, 16, N, 64)
    xyz = torch.from_numpy(s).to(dev)
    feats = torch.from_numpy(np.random.RandomState(N).standard_normal((16, 128, N)).astype(np.float32)).to(dev)
    spy = _Spy(monkeypatch)
    with torch.no_grad():
        _, a, _ = m(xyz, feats, 128, compact=True)
        _, b, _ = m(xyz, feats, 128)
    torch.cuda.synchronize()
    assert spy.calls == [(2048, expect), (2048, False)]
    assert torch.equal(a, b)
