"""ops.StateWatch — what the captured inference graphs compare before a replay — on a CPU module: it must see every way the
weights or the eval-mode parameter caches change, and nothing else (a spurious change makes PipelinedHotPath refuse to run)."""
import torch

from ptt_amd import ops
from ptt_amd.hot_path import FrameHotPath, kitti_model_cfg


def _model():
    return FrameHotPath(kitti_model_cfg()).eval()


def test_state_watch_sees_weight_writes():
    m = _model()
    w = ops.StateWatch(m)
    assert not w.changed()
    m.eval()                                            # no cache was built: nothing dropped
    assert not w.changed()
    with torch.no_grad():
        m.box_transformer.fc2.bias.add_(0.0)            # an in-place write: the version counter moves
    assert w.changed()
    w.mark()
    m.load_state_dict(_model().state_dict())
    assert w.changed()
    w.mark()
    bn = m.backbone_3d.SA_modules[0].mlp_module[0].normlayer.bn
    bn.running_mean.data = bn.running_mean.data.clone()  # new storage, same version
    assert w.changed()
    w.mark()
    assert not w.changed()


def test_state_watch_sees_cache_rebuilds_and_drops():
    m = _model()
    w = ops.StateWatch(m)
    ops.publish_params(torch.device('cpu'), replaced=False)     # a per-shape index table: grows, replaces nothing
    assert not w.changed()
    ops.publish_params(torch.device('cpu'))                     # some module rebuilt its packed weights
    assert w.changed()
    w.mark()
    sa = m.vote_aggregation
    sa._fused_cache.get([], torch.device('cpu'), lambda: 'layers')      # as if an eval forward had built it
    w.mark()
    m.train()                                                   # ... and train() frees it
    assert w.changed() and not sa._fused_cache.held()
    w.mark()
    m.eval()
    assert not w.changed()


def test_state_watch_sees_a_voting_heads_conv1d_stack_dropped():
    from ptt_amd.config import StubDataset, ptt_model_cfg
    from ptt_amd.models import build_network
    m = build_network(ptt_model_cfg(), 1, StubDataset()).eval()
    w = ops.StateWatch(m)
    stack = m.centroid_voting_head.vote_layer
    stack._rows_cache.get([], torch.device('cpu'), lambda: 'layers')    # as if an eval forward had folded its BatchNorm
    w.mark()
    m.train()
    assert w.changed() and not stack._rows_cache.held()
    w.mark()
    m.eval()
    assert not w.changed()
