"""PointnetSAModuleVotes with every constructor option at both values — use_xyz, normalize_xyz, bn — over its sampling modes and
with / without point features, on clouds whose balls hold distinct points (fused_ref.cube_clouds), in eval mode (every branch of
_forward_fused) and in training mode (the three routes of _forward_train the options select).

Eval mode. Each supported combination is compared with
  * the module's own unfused op sequence (`_fusable` forced off, as tests/test_hot_path_gpu.py::test_fused_equals_unfused_module_path
    does): indices and centres equal, features within that file's TOL;
  * the float64 reference fused_ref.sa_ref64 on the module's OWN index table (taken from the launch that made it), within R * Y,
    R = 4 and Y = max(e32, 4u) from the reference's float32 twin, as tests/test_fused_guard_gpu.py holds the kernels.
Which branch of _forward_fused ran is proved by counting the calls of ops.fps_ball_knn, ops.centres_ball_query (with / without a
selection), ops.row_jobs and ops.sa_fused_forward (with / without l0=); CONFIGS lists the counts each shape must give. No
supported combination may leave the hand-written kernels: warnings are errors inside the call and ops.unfused_calls must not grow.

Training mode. The two harnesses of tests/test_train_gpu.py (the clone with train_ops.usable off = the reference op sequence on
stock layers; call counters) with that file's bounds, restated here with their source lines.

Measured on an MI355X. Eval: err / Y between 0.28 and 1.32 over the 40 supported combinations (worst: inds_l0 with use_xyz on,
normalize off, bn on; the row-job branch 0.28 - 1.22), none above the 2.0 from which a case is to be investigated. Training: no
output outside 1e-4 (worst 0.010 x the tolerance), worst relative gradient error 1.75e-6 (one-launch front, layer 0's weight),
1.43e-6 (learnable coordinates), 1.72e-6 (use_xyz off) against the bound of 3e-5: the bounds of tests/test_train_gpu.py:296-317
hold on the denser clouds as they stand. No fault of the module was found.
"""
import copy
import warnings

import numpy as np
import pytest
import torch

from ptt_amd import ops, train_ops
from ptt_amd.hot_path import randomize_
from ptt_amd.models.backbones_3d.pointnet2.pointnet2_modules import PointnetSAModuleVotes
from tests import fused_ref as FR
from tests.fused_launch import R_RATIO
from tests.util import outside

pytestmark = pytest.mark.gpu

TOL = dict(atol=1e-4, rtol=1e-4)        # tests/test_hot_path_gpu.py:12: fused against unfused module path
Y_OUTSIDE_SA = 0                        # tests/test_train_gpu.py:18: training outputs allowed outside 1e-4 at an SA level
GRAD_TOL = 3e-5                         # tests/test_train_gpu.py:304: `close(p, q, name, tol=3e-5)`, every gradient


class Calls(object):
    """Counts the calls of the ops that tell the branches of the module apart, and keeps the last ball-query table."""

    def __init__(self):
        self.n = dict(fps_ball_knn=0, cbq_sel=0, cbq_prefix=0, row_jobs=0, sa_l0=0, sa_plain=0, z0=0, hoisted=0, pool=0)
        self.idx = None

    def __enter__(self):
        self.real = (ops.fps_ball_knn, ops.centres_ball_query, ops.row_jobs, ops.sa_fused_forward, ops.sa_z0_rows,
                     train_ops.sa_level_hoisted, train_ops.shared_mlp_pool)
        fbk, cbq, rj, sa, z0, hoisted, pool = self.real

        def fps_ball_knn(*a, **k):
            self.n["fps_ball_knn"] += 1
            r = fbk(*a, **k)
            self.idx = r[3]
            return r

        def centres_ball_query(xyz, sel, *a, **k):
            self.n["cbq_sel" if sel is not None else "cbq_prefix"] += 1
            r = cbq(xyz, sel, *a, **k)
            self.idx = r[2]
            return r

        def row_jobs(*a, **k):
            self.n["row_jobs"] += 1
            return rj(*a, **k)

        def sa_fused_forward(*a, **k):
            self.n["sa_l0" if k.get("l0") is not None else "sa_plain"] += 1
            return sa(*a, **k)

        def count(key, fn):
            def wrapped(*a, **k):
                self.n[key] += 1
                return fn(*a, **k)
            return wrapped

        ops.fps_ball_knn, ops.centres_ball_query, ops.row_jobs, ops.sa_fused_forward = fps_ball_knn, centres_ball_query, row_jobs, sa_fused_forward
        ops.sa_z0_rows, train_ops.sa_level_hoisted, train_ops.shared_mlp_pool = count("z0", z0), count("hoisted", hoisted), count("pool", pool)
        return self

    def __exit__(self, *exc):
        (ops.fps_ball_knn, ops.centres_ball_query, ops.row_jobs, ops.sa_fused_forward, ops.sa_z0_rows, train_ops.sa_level_hoisted,
         train_ops.shared_mlp_pool) = self.real


# ======================================================================================================================== eval
# name -> (B, N, M, C, mlp widths, radius, ns, sample_method, caller-given inds,
#          the calls with use_xyz on, the calls with use_xyz off). Feature widths stay below 192 = the K from which ops.linear
#          itself hands small launches to ops.row_jobs, so that row_jobs counts the two grouped layers alone.
CONFIGS = {
    # N <= 256, npoint <= 128, B * M * ns = 1024 rows: one index launch; three layers with c0 = 256 >= 192: two row-job launches
    "one_frame_rowjobs": (2, 128, 32, 16, [256, 256, 256], 0.4, 16, "fps", False,
                          dict(fps_ball_knn=1, row_jobs=2), dict(fps_ball_knn=1, sa_plain=1)),
    # the largest shape: 6144 rows > ops.ONE_FRAME_MAX_SA_ROWS: FPS, then centres + ball query with the selection; c0 = 64: l0=
    "fps_l0":            (3, 256, 64, 32, [64, 64, 128], 0.3, 32, "fps", False,
                          dict(cbq_sel=1, sa_l0=1), dict(cbq_sel=1, sa_plain=1)),
    # 'sequence': the first M points, no selection; two layers
    "sequence_l0":       (2, 80, 9, 5, [32, 64], 0.4, 16, "sequence", False,
                          dict(cbq_prefix=1, sa_l0=1), dict(cbq_prefix=1, sa_plain=1)),
    # caller-given indices; the stream shape (128 -> 128 -> 256 behind a hoisted 128-channel layer 0) when the layers allow it
    "inds_l0":           (2, 128, 33, 128, [128, 128, 256], 0.5, 32, "fps", True,
                          dict(cbq_sel=1, sa_l0=1), dict(cbq_sel=1, sa_plain=1)),
    # no point features (the SA0 shape): layer 0 runs inside the kernel, compact on
    "sequence_nofeat":   (3, 96, 37, 0, [64, 64, 128], 0.3, 32, "sequence", False,
                          dict(cbq_prefix=1, sa_plain=1), None),
    "fps_nofeat":        (3, 96, 37, 0, [64, 64, 128], 0.3, 32, "fps", False,
                          dict(fps_ball_knn=1, sa_plain=1), None),
}


def module_layers(m):
    """The SharedMLP of a module (on the host) as fused_ref layer dicts: conv [+ bias] [+ BatchNorm running statistics]."""
    layers = []
    for unit in m.mlp_module:
        L = {"conv_weight": unit.conv.weight.detach().clone()}
        if unit.conv.bias is not None:
            L["conv_bias"] = unit.conv.bias.detach().clone()
        if hasattr(unit, "normlayer"):
            bn = unit.normlayer.bn
            L.update(bn_weight=bn.weight.detach().clone(), bn_bias=bn.bias.detach().clone(), bn_mean=bn.running_mean.clone(),
                     bn_var=bn.running_var.clone(), eps=bn.eps)
        layers.append(L)
    return layers


def build(cfg, use_xyz, normalize, bn, seed):
    B, N, M, C, widths, radius, ns, method, given = cfg[:9]
    cin = C if (C or use_xyz) else 16       # use_xyz off without features: a module built for 16 feature channels is given none
    m = randomize_(PointnetSAModuleVotes(mlp=[cin] + list(widths), radius=radius, nsample=ns, bn=bn, use_xyz=use_xyz,
                                         normalize_xyz=normalize, sample_method=method), seed=seed)
    rs = np.random.RandomState(seed)
    xyz = torch.from_numpy(FR.cube_clouds(7, B, N))
    feats = torch.from_numpy(rs.standard_normal((B, C, N)).astype(np.float32)) if C else None
    inds = torch.from_numpy(np.stack([rs.permutation(N)[:M] for _ in range(B)]).astype(np.int32)) if given else None
    return m, xyz, feats, inds


@pytest.mark.parametrize("bn", [True, False])
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("use_xyz", [True, False])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_eval_options(dev, name, use_xyz, normalize, bn):
    cfg = CONFIGS[name]
    B, N, M, C, widths, radius, ns, method, given, calls_xyz, calls_noxyz = cfg
    want = calls_xyz if use_xyz else calls_noxyz
    m, xyz, feats, inds = build(cfg, use_xyz, normalize, bn, seed=5 + len(name))
    layers = module_layers(m)
    m = m.to(dev).eval()
    dx, df, di = xyz.to(dev), (feats.to(dev) if feats is not None else None), (inds.to(dev) if inds is not None else None)
    if want is None:
        # use_xyz = False without point features: nothing to group. The reference asserts (pointnet2_utils.py:365-367); here the
        # launch is refused (PTT_EINVAL, include/ptt_hip.h: ptt_sa_desc.use_xyz), not run on something else
        with torch.no_grad(), pytest.raises(RuntimeError, match="PTT_EINVAL"):
            m(dx, None, M, di)
        return
    before = dict(ops.unfused_calls)
    with torch.no_grad(), Calls() as calls, warnings.catch_warnings():
        warnings.simplefilter("error")
        a_xyz, a_f, a_i = m(dx, df, M, di)
    assert ops.unfused_calls == before, "an eval-mode call left the hand-written kernels"
    expect = dict.fromkeys(calls.n, 0)
    expect.update(want)
    assert calls.n == expect, (calls.n, expect)
    idx = calls.idx.cpu()
    with torch.no_grad():
        m._fusable = lambda *a: False                     # the reference op sequence on the HIP index ops + stock torch layers
        b_xyz, b_f, b_i = m(dx, df, M, di)
    assert a_i.dtype == torch.int64 and tuple(a_f.shape) == (B, widths[-1], M)
    np.testing.assert_array_equal(a_i.cpu().numpy(), b_i.cpu().numpy())
    np.testing.assert_array_equal(a_xyz.cpu().numpy(), b_xyz.cpu().numpy())
    np.testing.assert_allclose(a_f.cpu().numpy(), b_f.cpu().numpy(), **TOL)
    if given:
        np.testing.assert_array_equal(a_i.cpu().numpy(), inds.long().numpy())
    elif method == "sequence":
        np.testing.assert_array_equal(a_i.cpu().numpy(), np.tile(np.arange(M), (B, 1)))
    # the float64 reference on the module's own centres and index table
    centres = torch.gather(xyz, 1, a_i.cpu()[..., None].expand(-1, -1, 3))
    assert torch.equal(a_xyz.cpu(), centres)
    idx_ref = torch.from_numpy(np.ascontiguousarray(FR.O.ball_query(centres.numpy(), xyz.numpy(), radius, ns)))
    assert torch.equal(idx, idx_ref), "the module's index table is not the oracle's"
    ref64 = FR.sa_ref64(xyz, centres, feats, idx, layers, radius, ns, use_xyz, normalize)
    ref32 = FR.sa_ref(xyz, centres, feats, idx, layers, radius, ns, use_xyz, normalize, dtype=torch.float32)
    Y = FR.yardstick(ref32, ref64)
    r = FR.rel_err(a_f, ref64) / Y
    print("RATIO module %s use_xyz=%d normalize=%d bn=%d  Y %.3e  err/Y %.2f" % (name, use_xyz, normalize, bn, Y, r))
    assert R_RATIO <= 8 and r <= R_RATIO, "%.2f x the float32 twin's own distance from float64 (R = %g)" % (r, R_RATIO)
    np.testing.assert_allclose(a_f.cpu().numpy(), ref32.numpy(), **FR.TOL)


# ==================================================================================================================== training
def _train_pair(dev, B, N, M, C, spec, radius, ns, xyz_grad, seed, **options):
    """A module and its clone in train mode on cube clouds -> ((outputs, inputs) of the row-kernel path, the same of the clone
    run with train_ops.usable off = the reference op sequence on stock layers, the calls the first one made)."""
    torch.manual_seed(seed)
    a = PointnetSAModuleVotes(mlp=list(spec), radius=radius, nsample=ns, sample_method='fps', **options).to(dev).train()
    b = copy.deepcopy(a)
    xyz1 = torch.from_numpy(FR.cube_clouds(7, B, N)).to(dev).requires_grad_(xyz_grad)
    f1 = torch.randn(B, C, N, device=dev, requires_grad=True) if C else None
    xyz2 = xyz1.detach().clone().requires_grad_(xyz_grad)
    f2 = f1.detach().clone().requires_grad_(True) if C else None
    with Calls() as calls:
        out1 = a(xyz1, f1, M)
    orig = train_ops.usable
    train_ops.usable = lambda *k: False
    try:
        out2 = b(xyz2, f2, M)
    finally:
        train_ops.usable = orig
    return (a, out1, xyz1, f1), (b, out2, xyz2, f2), calls.n


def _same_training_step(one, two, what):
    """tests/test_train_gpu.py:295-317: indices and centres equal, no output outside 1e-4 and the worst at 0.1 x the tolerance,
    every gradient within GRAD_TOL = 3e-5 of the largest reference entry, the BatchNorm buffers within rtol 1e-3 / atol 1e-5."""
    (a, (nx1, y1, i1), xyz1, f1), (b, (nx2, y2, i2), xyz2, f2) = one, two
    assert torch.equal(i1, i2) and i1.dtype == torch.int64 and torch.equal(nx1, nx2)                       # :295
    n_out, worst_y = outside(y1, y2)                                                                        # :296
    up = torch.randn_like(y2)
    (y1 * up).sum().backward()
    (y2 * up).sum().backward()
    pairs = [(p1.grad, p2.grad, n1) for (n1, p1), (_, p2) in zip(a.named_parameters(), b.named_parameters())]
    if f1 is not None:
        pairs.append((f1.grad, f2.grad, "feature grad"))
    if xyz1.requires_grad and xyz2.grad is not None:
        pairs.append((xyz1.grad, xyz2.grad, "xyz grad"))
    errs = {name: float((p - q).abs().max()) / (float(q.abs().max()) + 1e-12) for p, q, name in pairs}      # :307
    worst = max(errs, key=errs.get)
    print("measured %s: %d of %d outputs outside 1e-4, worst %.3f x the tolerance; worst relative gradient error %.2e (%s)"
          % (what, n_out, y2.numel(), worst_y, errs[worst], worst))
    assert n_out <= Y_OUTSIDE_SA and worst_y <= 0.1, (n_out, worst_y)                                       # :298
    for name, err in errs.items():
        assert err < GRAD_TOL, (name, err)                                                                  # :309
    for (n1, b1), (_, b2) in zip(a.named_buffers(), b.named_buffers()):
        torch.testing.assert_close(b1.float(), b2.float(), rtol=1e-3, atol=1e-5, msg=n1)                    # :317
    return errs


TRAIN_SHAPES = [(2, 128, 64, 128, [128, 128, 128, 256], 0.5, 32), (2, 64, 32, 0, [0, 64, 64, 128], 0.5, 32)]


@pytest.mark.parametrize("B,N,M,C,spec,radius,ns", TRAIN_SHAPES)
def test_training_without_normalize_fixed_coordinates(dev, B, N, M, C, spec, radius, ns):
    """normalize_xyz = False with fixed coordinates: the one-launch front (ops.sa_z0_rows, rmul = 1), with point features and
    without."""
    one, two, calls = _train_pair(dev, B, N, M, C, spec, radius, ns, False, 12, use_xyz=True, normalize_xyz=False)
    assert calls["z0"] == 1 and calls["hoisted"] == 1 and calls["pool"] == 0 and calls["cbq_sel"] == 1
    _same_training_step(one, two, "one-launch front, normalize off, %s" % spec)


def test_training_without_normalize_learnable_coordinates(dev):
    """normalize_xyz = False with xyz.requires_grad: train_ops.sa_level_hoisted's branch for learnable coordinates (grouping,
    `if normalize_xyz:`, gather rows), gradients to the coordinates included."""
    B, N, M, C, spec, radius, ns = TRAIN_SHAPES[0]
    one, two, calls = _train_pair(dev, B, N, M, C, spec, radius, ns, True, 11, use_xyz=True, normalize_xyz=False)
    assert calls["hoisted"] == 1 and calls["z0"] == 0 and calls["pool"] == 0 and calls["cbq_sel"] == 0
    errs = _same_training_step(one, two, "learnable coordinates, normalize off, %s" % spec)
    assert "xyz grad" in errs and float(one[2].grad.abs().max()) > 0


@pytest.mark.parametrize("normalize", [True, False])
def test_training_without_xyz_channels(dev, normalize):
    """use_xyz = False with features: no hoist (layer 0 has no coordinate half) — the grouped features go through
    train_ops.shared_mlp_pool."""
    B, N, M, C, spec, radius, ns = TRAIN_SHAPES[0]
    one, two, calls = _train_pair(dev, B, N, M, C, spec, radius, ns, False, 13, use_xyz=False, normalize_xyz=normalize)
    assert calls["pool"] == 1 and calls["hoisted"] == 0 and calls["z0"] == 0
    assert one[0].mlp_module[0].conv.weight.shape[1] == C
    _same_training_step(one, two, "use_xyz off, normalize %d" % normalize)


def test_training_without_batchnorm_leaves_the_row_kernels(dev):
    """bn = False: train_ops.usable is false (the row kernels form batch statistics), the stock layers run. Nothing else is
    new there: only that, and that forward and backward run."""
    B, N, M, C, spec, radius, ns = TRAIN_SHAPES[0]
    torch.manual_seed(14)
    m = PointnetSAModuleVotes(mlp=list(spec), radius=radius, nsample=ns, bn=False, normalize_xyz=False).to(dev).train()
    xyz = torch.from_numpy(FR.cube_clouds(7, B, N)).to(dev)
    f = torch.randn(B, C, N, device=dev, requires_grad=True)
    assert not train_ops.usable(m.mlp_module, f)
    with Calls() as calls:
        _, y, _ = m(xyz, f, M)
    assert calls.n["hoisted"] == calls.n["pool"] == calls.n["z0"] == 0
    y.square().mean().backward()
    assert tuple(y.shape) == (B, spec[-1], M) and torch.isfinite(y).all()
    assert torch.isfinite(f.grad).all() and float(f.grad.abs().sum()) > 0
