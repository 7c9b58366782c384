"""Feature-space furthest point sampling ('ffps') on the device: ptt_ffps_f32 against its numpy definition (tests/ffps_ref.py),
index for index; the layouts it reads in place; guard bands; the reference module's fixture G22; the SA module, the backbone, the
tracker and the training path with 'ffps' at the levels that carry point features."""
import os

import numpy as np
import pytest
import torch

from oracle import dense_ref as R
from ptt_amd import ops, synth
from tests import ffps_ref, guard
from tests.util import fill_state_dict_, mlp_layers

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = dict(atol=1e-4, rtol=1e-4)


def _clouds(rs, B, N):
    return np.ascontiguousarray(np.stack([synth.cloud(rs, N, max(N // 2, 8), synth.SEARCH_BOX, synth.CAR_SIGMA, 0.7)
                                          for _ in range(B)]), np.float32)


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _load_mlp(mlp, layers):
    with torch.no_grad():
        for unit, L in zip(mlp, layers):
            unit.conv.weight.copy_(L["conv_weight"])
            bn = unit.normlayer.bn
            bn.weight.copy_(L["bn_weight"]); bn.bias.copy_(L["bn_bias"])
            bn.running_mean.copy_(L["bn_mean"]); bn.running_var.copy_(L["bn_var"])


def _ffps_cfg():
    from ptt_amd.config import ptt_model_cfg
    cfg = ptt_model_cfg()
    cfg.BACKBONE_3D.SA_CONFIG.SAMPLE_METHOD = ['fps', 'ffps', 'ffps']
    cfg.BOX_HEAD.SA_CONFIG.SAMPLE_METHOD = 'ffps'
    return cfg


# (B, N, C, npoint): one wave, several waves, sizes that are no multiple of the workgroup, npoint == N, more than one point per
# thread (1025), the three shapes the model runs (SA1, SA2, the box head's 257 channels), npoint = 1, no features
SHAPES = [(2, 64, 1, 32), (3, 128, 8, 64), (2, 200, 37, 77), (1, 40, 5, 40), (2, 1025, 4, 16), (2, 512, 128, 256),
          (2, 256, 256, 128), (2, 128, 257, 64), (2, 100, 6, 1), (2, 300, 0, 150),
          # C = 128 / 256 / 257 take the register-resident kernel up to 512 / 256 / 256 points: a ragged size inside its reach and
          # the first size past it on either side (streamed again)
          (2, 200, 128, 50), (1, 513, 128, 20), (1, 257, 256, 20), (2, 70, 257, 70)]


@pytest.mark.parametrize("B,N,C,npoint", SHAPES)
def test_op_equals_the_definition_on_general_input(dev, B, N, C, npoint):
    rs = np.random.RandomState(1000 + N + C)
    xyz = _clouds(rs, B, N)
    feat = rs.standard_normal((B, C, N)).astype(np.float32) if C else None
    got = ops.feature_fps(_dev(xyz, dev), _dev(feat, dev) if C else None, npoint)
    assert got.dtype == torch.int32 and tuple(got.shape) == (B, npoint)
    np.testing.assert_array_equal(got.cpu().numpy(), ffps_ref.ffps(xyz, feat, npoint))


def test_op_on_ties_duplicates_and_an_identical_cloud(dev):
    rs = np.random.RandomState(5)
    xyz = rs.randint(-1, 2, (2, 256, 3)).astype(np.float32)                      # the tie grid: lowest index wins
    feat = rs.randint(-1, 2, (2, 3, 256)).astype(np.float32)
    np.testing.assert_array_equal(ops.feature_fps(_dev(xyz, dev), _dev(feat, dev), 64).cpu().numpy(), ffps_ref.ffps(xyz, feat, 64))
    x0, f0 = ffps_ref.exact_cloud(rs, 2, 40, 5)                                  # duplicated rows
    src = rs.randint(0, 40, (2, 120))
    xyz = np.stack([x0[b][src[b]] for b in range(2)])
    feat = np.stack([f0[b][:, src[b]] for b in range(2)])
    np.testing.assert_array_equal(ops.feature_fps(_dev(xyz, dev), _dev(feat, dev), 60).cpu().numpy(), ffps_ref.ffps(xyz, feat, 60))
    xyz = np.tile(np.float32([[0.5, -1.25, 2.0]]), (2, 33, 1))                   # all identical: zeros
    feat = np.tile(np.float32([[1.0], [2.0], [-3.0], [0.25]]), (2, 1, 33))
    assert not ops.feature_fps(_dev(xyz, dev), _dev(feat, dev), 17).cpu().numpy().any()
    assert not ops.feature_fps(_dev(xyz, dev), None, 17).cpu().numpy().any()


@pytest.mark.parametrize("B,N,C,npoint", [(2, 200, 37, 77), (2, 512, 128, 64)])
def test_layouts_are_read_in_place_and_guards_hold(dev, B, N, C, npoint):
    """(B,C,N) contiguous, the transposed view of (B,N,C) rows, and point-major rows with stride C + 4 inside NaN surroundings
    give identical indices; idx_out lies inside guard bands and nothing outside it is written; two calls are bit-identical."""
    rs = np.random.RandomState(77 + N)
    xyz_h = _clouds(rs, B, N)
    feat_h = rs.standard_normal((B, C, N)).astype(np.float32)
    want = ffps_ref.ffps(xyz_h, feat_h, npoint)
    xyz = guard.embed(_dev(xyz_h, dev))                                          # contiguous rows, NaN in front and behind
    bcn = _dev(feat_h, dev)
    rows = bcn.transpose(1, 2).contiguous()                                      # (B,N,C)
    padded = guard.embed(rows, ld=C + 4)                                         # rows with stride C + 4, NaN between them
    layouts = {"bcn": bcn, "transposed": rows.transpose(1, 2), "padded rows": padded.transpose(1, 2)}
    assert layouts["transposed"].stride() == (N * C, 1, C) and layouts["padded rows"].stride()[1:] == (1, C + 4)
    for name, f in layouts.items():
        ptr0 = f.data_ptr()
        got = ops.feature_fps(xyz, f, npoint)
        assert f.data_ptr() == ptr0
        np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=name)
        out = guard.guarded((B, npoint), torch.int32, device=dev)
        sb, sc, sn = f.stride()
        guard.launch("ptt_ffps_f32", dev, guard.ptr(xyz), guard.ptr(f), sb, sc, sn, B, N, C, npoint, guard.ptr(out))
        guard.check_guard(out)
        np.testing.assert_array_equal(out.cpu().numpy(), want, err_msg=name)
        assert torch.equal(ops.feature_fps(xyz, f, npoint), got)
    guard.assert_untouched(xyz, padded)


def test_G22_reference_module_with_ffps(dev):
    """Fixture G22: the reference's own PointnetSAModuleVotes(sample_method='ffps') on exact-arithmetic input (its missing
    extension op stubbed by the numpy matrix loop). inds exactly, features within 1e-4."""
    from ptt_amd.models.backbones_3d.pointnet2.pointnet2_modules import PointnetSAModuleVotes
    g = np.load(os.path.join(GOLD, "G22_ffps_module.npz"))
    spec = [int(c) for c in g["spec"]]
    layers = mlp_layers(int(g["seed"]), spec)
    for li, L in enumerate(layers):                                              # the seeded weights ARE the stored ones
        for k, v in L.items():
            np.testing.assert_array_equal(np.asarray(v), g["layer%d_%s" % (li, k)])
    m = PointnetSAModuleVotes(mlp=[spec[0] - 3] + spec[1:], radius=float(g["radius"]), nsample=int(g["nsample"]),
                              normalize_xyz=True, sample_method='ffps').eval()
    _load_mlp(m.mlp_module, layers)
    m = m.to(dev)
    xyz, feats = _dev(g["xyz"], dev), _dev(g["feats"], dev)
    with torch.no_grad():
        nx, nf, ii = m(xyz, feats, int(g["npoint"]))
    assert ii.dtype == torch.int64
    np.testing.assert_array_equal(ii.cpu().numpy(), g["inds"])
    np.testing.assert_array_equal(nx.cpu().numpy(), g["new_xyz"])
    np.testing.assert_allclose(nf.cpu().numpy(), g["new_features"], **TOL)
    # and the matrix the reference handed to its sampler gives the same picks through the matrix loop
    np.testing.assert_array_equal(ffps_ref.fps_with_dist(g["dist"], int(g["npoint"])), g["inds"])


def test_sa_module_eval_with_ffps(dev):
    from ptt_amd.models.backbones_3d.pointnet2.pointnet2_modules import PointnetSAModuleVotes
    B, N, M, C = 2, 512, 256, 128
    rs = np.random.RandomState(42)
    xyz_h = _clouds(rs, B, N)
    feat_h = rs.standard_normal((B, C, N)).astype(np.float32)
    layers = mlp_layers(43, [C + 3, 128, 128, 256])
    m = PointnetSAModuleVotes(mlp=[C, 128, 128, 256], radius=0.5, nsample=32, normalize_xyz=True, sample_method='ffps').eval()
    _load_mlp(m.mlp_module, layers)
    m = m.to(dev)
    xyz, feats = _dev(xyz_h, dev), _dev(feat_h, dev)
    before = dict(ops.unfused_calls)
    with torch.no_grad():
        nx, nf, ii = m(xyz, feats, M)
        nx2, nf2, ii2 = m(xyz, feats, M, inds=ii.to(torch.int32))
    assert dict(ops.unfused_calls) == before                                     # the fused path ran
    want = ffps_ref.ffps(xyz_h, feat_h, M)
    np.testing.assert_array_equal(ii.cpu().numpy(), want)
    rx, rf, _ = R.sa_module(torch.from_numpy(xyz_h), torch.from_numpy(feat_h), M, layers, 0.5, 32, use_xyz=True, normalize_xyz=True,
                            inds=torch.from_numpy(want))
    np.testing.assert_array_equal(nx.cpu().numpy(), rx.numpy())
    np.testing.assert_allclose(nf.cpu().numpy(), rf.numpy(), **TOL)
    assert torch.equal(nx, nx2) and torch.equal(nf, nf2) and torch.equal(ii, ii2)


def test_backbone_levels_sample_on_what_they_receive(dev):
    """['fps', 'ffps', 'ffps']: every level's indices are the definition's on the (xyz, features) THAT level was handed (recorded
    by forward hooks), so a level's picks are judged on its own input, not on a recomputation of the levels below; and the
    composed indices select the seeds from the raw cloud bitwise."""
    from ptt_amd.models.backbones_3d.pointnet2_backbone import PointNet2BackboneLight
    sa_cfg = _ffps_cfg().BACKBONE_3D
    bb = fill_state_dict_(PointNet2BackboneLight(sa_cfg, input_channels=3), 11).to(dev).eval()
    seen = []
    hooks = [m.register_forward_hook(lambda mod, args, kwargs, out: seen.append((mod, kwargs, out)), with_kwargs=True)
             for m in bb.SA_modules]
    s_h, t_h = synth.frames(2024, 2, 1024, 512)
    search, template = _dev(s_h, dev), _dev(t_h, dev)
    with torch.no_grad():
        out = bb.forward_branches(search, template)
    torch.cuda.synchronize()
    for h in hooks:
        h.remove()
    assert len(seen) == 6
    n_ffps = 0
    for mod, kwargs, (new_xyz, new_feats, inds) in seen:
        if mod.sample_method != 'ffps':
            continue
        xyz_in, f_in, npoint = kwargs['xyz'], kwargs['features'], kwargs['npoint']
        assert f_in is not None and f_in.shape[2] == xyz_in.shape[1] and inds.dtype == torch.int64
        want = ffps_ref.ffps(xyz_in.cpu().numpy(), f_in.cpu().numpy(), npoint)
        np.testing.assert_array_equal(inds.cpu().numpy(), want)
        np.testing.assert_array_equal(new_xyz.cpu().numpy(), np.take_along_axis(xyz_in.cpu().numpy(), want[:, :, None].astype(np.int64), 1))
        n_ffps += 1
    assert n_ffps == 4
    for pts, key in ((search, 'search'), (template, 'template')):
        inds, seeds = out[key + '_inds'], out[key + '_seeds']
        assert inds.dtype == torch.int64
        for b in range(2):
            assert torch.equal(pts[b, inds[b]], seeds[b])
            assert len(set(inds[b].tolist())) > 1


def test_tracklet_runner_graph_and_eager_agree_with_ffps(dev):
    from ptt_amd.config import StubDataset
    from ptt_amd.hot_path import randomize_
    from ptt_amd.models import build_network
    from ptt_amd.tracklet_runner import TrackletRunner
    tracker = randomize_(build_network(_ffps_cfg(), 1, StubDataset()), seed=2).to(dev).eval()
    assert [m.sample_method for m in tracker.backbone_3d.SA_modules] == ['fps', 'ffps', 'ffps']
    assert tracker.box_voting_head.vote_aggregation.sample_method == 'ffps'
    with torch.no_grad():                                  # small regression outputs, as a trained model's are
        tracker.box_voting_head.refine_layer[-1].conv.weight.mul_(0.05)
        tracker.box_voting_head.refine_layer[-1].conv.bias.mul_(0.05)
    tracklets = [synth.tracklet(321, 3)]
    graphed = TrackletRunner(tracker, dev, batch=1, use_graph=True).run(tracklets)
    eager = TrackletRunner(tracker, dev, batch=1, use_graph=False).run(tracklets)
    assert len(graphed) == len(eager) == 1 and len(graphed[0]) == len(eager[0]) == 3
    for a, b in zip(graphed[0], eager[0]):
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[2], b[2])
        assert np.isfinite(a[0]).all()
    assert float(np.abs(graphed[0][2][0] - graphed[0][0][0]).max()) > 1e-6       # the box moved with the object


def test_sa_module_training_with_ffps_equals_supplied_indices(dev):
    """Training mode: 'ffps' == the same module handed the same indices, bit for bit — output, input gradient, weight gradients.
    The sampling reads features.detach(): features.grad carries nothing from it."""
    from ptt_amd.models.backbones_3d.pointnet2.pointnet2_modules import PointnetSAModuleVotes
    B, N, M, C = 2, 256, 128, 64
    rs = np.random.RandomState(9)
    xyz = _dev(_clouds(rs, B, N), dev)
    feat_h = rs.standard_normal((B, C, N)).astype(np.float32)
    up = _dev(rs.standard_normal((B, 128, M)).astype(np.float32), dev)
    a = PointnetSAModuleVotes(mlp=[C, 64, 128], radius=0.5, nsample=16, normalize_xyz=True, sample_method='ffps').to(dev).train()
    b = PointnetSAModuleVotes(mlp=[C, 64, 128], radius=0.5, nsample=16, normalize_xyz=True, sample_method='fps').to(dev).train()
    b.load_state_dict(a.state_dict())
    f1 = _dev(feat_h, dev).requires_grad_(True)
    f2 = _dev(feat_h, dev).requires_grad_(True)
    x1, y1, i1 = a(xyz, f1, M)
    np.testing.assert_array_equal(i1.cpu().numpy(), ffps_ref.ffps(xyz.cpu().numpy(), feat_h, M))
    x2, y2, i2 = b(xyz, f2, M, inds=i1.to(torch.int32))
    assert torch.equal(x1, x2) and torch.equal(y1, y2) and torch.equal(i1, i2)
    (y1 * up).sum().backward()
    (y2 * up).sum().backward()
    assert f1.grad is not None and float(f1.grad.abs().sum()) > 0
    assert torch.equal(f1.grad, f2.grad)
    for (k, p), q in zip(a.named_parameters(), b.parameters()):
        assert p.grad is not None and torch.equal(p.grad, q.grad), k


def test_full_model_trains_a_step_with_ffps(dev):
    from ptt_amd.config import StubDataset
    from ptt_amd.models import build_network
    from ptt_amd.train_step import synthetic_train_batch
    model = fill_state_dict_(build_network(_ffps_cfg(), 1, StubDataset(training=True)), 5).to(dev).train()
    ret, _, _ = model(synthetic_train_batch(77, 4, dev))
    loss = ret['loss'].mean()
    loss.backward()
    assert np.isfinite(float(loss.detach()))
    for k, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
