"""Every module that keeps an eval-mode parameter cache (ptt_amd.param_cache.ParamCache), at the smallest shape its fused
path takes: after each way its weights can change, the module computes what a freshly built module with the same state_dict()
computes — bit for bit, the same deterministic kernels on the same numbers.
  (a) an in-place write to one weight, (b) load_state_dict of other weights, and for the modules that fold BatchNorm running
  statistics (c) train(), one train-mode forward that moves the statistics, eval(). (c) checks the result, not the mechanism:
  the forward also bumps num_batches_tracked, which is in the key, so it passes with or without the owners' train() override;
  that override is what tests/test_state_watch_cpu.py checks."""
import pytest
import torch

from ptt_amd import ops
from ptt_amd.hot_path import AttrDict, kitti_model_cfg, randomize_
from ptt_amd.models.backbones_3d.pointnet2 import pytorch_utils as pt_utils
from ptt_amd.models.backbones_3d.pointnet2.pointnet2_modules import PointnetSAModuleVotes
from ptt_amd.models.backbones_3d.pointnet2_backbone import PointNet2BackboneLight
from ptt_amd.models.similarity_modules import CosineSimAug
from ptt_amd.models.transformer_block.multitransformer import MulTransformerBlock
from ptt_amd.models.transformer_block.variants import TransformerBlock, TransformerBlockSTD

pytestmark = pytest.mark.gpu


def _rand(dev, seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dev)


def _tensors(out):
    out = out if isinstance(out, (tuple, list)) else (out,)
    return [t for t in out if isinstance(t, torch.Tensor)]


def _same(a, b):
    a, b = _tensors(a), _tensors(b)
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _check(dev, make, run, weight, train_forward=None, stats=None):
    """make() -> a new module; run(module) -> its eval-mode output on the fused path (tensor or tuple, freshly allocated);
    weight(module) -> the parameter of (a); train_forward(module): one train-mode forward; stats(module) -> a running_mean it moves."""
    build = lambda seed: randomize_(make(), seed=seed).to(dev).eval()
    unfused = dict(ops.unfused_calls)

    def fresh_output(m):
        twin = build(99)
        twin.load_state_dict(m.state_dict())
        return run(twin)

    with torch.no_grad():
        m = build(1)
        out0 = run(m)
        assert _same(out0, fresh_output(m))
        weight(m).mul_(1.5)                                             # (a)
        out1 = run(m)
        assert not _same(out1, out0)
        assert _same(out1, fresh_output(m))
        m.load_state_dict(build(2).state_dict())                        # (b)
        out2 = run(m)
        assert not _same(out2, out1)
        assert _same(out2, fresh_output(m))
        if train_forward is not None:                                   # (c)
            before = stats(m).clone()
            m.train()
            train_forward(m)
            m.eval()
            assert not torch.equal(stats(m), before)
            out3 = run(m)
            assert not _same(out3, out2)
            assert _same(out3, fresh_output(m))
    assert ops.unfused_calls == unfused                                 # every eval-mode call took the hand-written kernels


@pytest.mark.parametrize("C", [0, 32])
def test_sa_module(dev, C):
    """Without point features (C = 0) and with them (the hoisted layer 0)."""
    N, npoint = 64, 16
    xyz = torch.rand(1, N, 3, generator=torch.Generator().manual_seed(3)).to(dev)
    feats = _rand(dev, 4, 1, N, C).transpose(1, 2) if C else None       # (B,C,N) view of point-major rows
    make = lambda: PointnetSAModuleVotes(mlp=[C, 32, 32], radius=0.4, nsample=16, use_xyz=True, normalize_xyz=True)

    def run(m):
        new_xyz, new_feats, inds = m(xyz, feats, npoint)
        assert m._fused_cache.held()
        return new_xyz, new_feats, inds

    _check(dev, make, run, lambda m: m.mlp_module[1].conv.weight, lambda m: m(xyz, feats, npoint),
           lambda m: m.mlp_module[0].normlayer.bn.running_mean)


@pytest.mark.parametrize("cls", [TransformerBlock, TransformerBlockSTD])
def test_transformer_block(dev, cls):
    xyz, feats = _rand(dev, 5, 1, 16, 3), _rand(dev, 6, 1, 16, 256)
    _check(dev, lambda: cls(256, 512, 16), lambda m: m(xyz, feats), lambda m: m.fc_delta[2].weight)


def test_mul_transformer_block(dev):
    xyz, feats = _rand(dev, 5, 1, 16, 3), _rand(dev, 6, 1, 16, 256)
    _check(dev, lambda: MulTransformerBlock(256, 512, 16, heads=4, layers=1), lambda m: m(xyz, feats),
           lambda m: m.layers[0].norm1.weight)


def test_cosine_sim_aug(dev):
    cfg = AttrDict.wrap(dict(DEBUG=False, MLP=dict(CHANNELS=[260, 256, 256, 256], BN=True),
                             CONV=dict(CHANNELS=[256, 256, 256], BN=True)))
    batch = lambda: {'search_feats': _rand(dev, 7, 1, 256, 8), 'template_feats': _rand(dev, 8, 1, 256, 64),
                     'template_seeds': _rand(dev, 9, 1, 64, 3)}
    _check(dev, lambda: CosineSimAug(cfg), lambda m: m(batch())['cosine_feats'], lambda m: m.mlp[2].conv.weight,
           lambda m: m(batch()), lambda m: m.mlp[1].normlayer.bn.running_mean)


def _seq():
    return pt_utils.Seq(35).conv1d(64, bn=True).conv1d(64, bn=True).conv1d(32, activation=None)


def test_conv1d_stack_rows_forward(dev):
    rows = _rand(dev, 10, 1, 16, 35)

    def run(seq):
        assert pt_utils.rows_fusable(seq, rows)
        return pt_utils.rows_forward(seq, rows)

    _check(dev, _seq, run, lambda seq: seq[1].conv.weight, lambda seq: seq(rows.transpose(1, 2)),
           lambda seq: seq[1].normlayer.bn.running_mean)


def test_conv1d_stack_rows_layers_rotated(dev):
    """rows_layers(seq, 3): the first layer reads [feats | xyz] from two tensors. One launch of three independent jobs, one
    per layer, so that every layer's fold and the rotated pack are in the output."""
    feats, xyz = _rand(dev, 11, 16, 32), _rand(dev, 12, 16, 3)
    h1, h2 = _rand(dev, 13, 16, 64), _rand(dev, 14, 16, 64)

    def run(seq):
        L = pt_utils.rows_layers(seq, 3)
        outs = [torch.empty((16, layer.cout), dtype=torch.float32, device=dev) for layer in L]
        ops.row_jobs([pt_utils.layer_job(L[0], x=feats, x2=xyz, out=outs[0]), pt_utils.layer_job(L[1], x=h1, out=outs[1]),
                      pt_utils.layer_job(L[2], x=h2, out=outs[2])])
        return outs

    _check(dev, _seq, run, lambda seq: seq[0].conv.weight, lambda seq: seq(_rand(dev, 15, 1, 35, 16)),
           lambda seq: seq[0].normlayer.bn.running_mean)


def test_backbone_cov_final(dev):
    feats = _rand(dev, 16, 1, 16, 256).transpose(1, 2)                  # (B,256,M) view of point-major rows, M = 16
    make = lambda: PointNet2BackboneLight(kitti_model_cfg().BACKBONE_3D, input_channels=3)

    def run(m):
        out = m._cov_final(feats)
        assert m._cov_cache.held()
        return out

    _check(dev, make, run, lambda m: m.cov_final.bias)
