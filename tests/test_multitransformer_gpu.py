"""MulTransformerBlock on the HIP kernels: the fused eval path (per-head pair kernel for many points, the row-job chain for
one frame, the LayerNorm kernel) against fixture G19 and against a float64 copy of the block, the tracker with both blocks
swapped, TrackletRunner's graphs, and the training-mode block on the GPU."""
import os
import warnings

import numpy as np
import pytest
import torch

from oracle import index_ops as O
from ptt_amd import ops, synth
from ptt_amd.models.transformer_block.multitransformer import FUSED_HEADS, MulTransformerBlock
from tests import multitransformer_ref as M
from tests.util import outside

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = dict(atol=1e-4, rtol=1e-4)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def g19():
    return np.load(os.path.join(GOLD, "G19_multitransformer.npz"))


def _block(heads, layers, seed, dev):
    return M.seeded_(MulTransformerBlock(256, 512, 16, heads, layers), seed).to(dev).eval()


@pytest.mark.parametrize("heads,layers", [b for b in M.BLOCKS if b[0] in FUSED_HEADS])
@pytest.mark.parametrize("N", M.SIZES)
def test_fused_matches_g19_on_both_paths(dev, g19, heads, layers, N):
    seed = M.block_seed(heads, layers, N)
    blk = _block(heads, layers, seed, dev)
    xyz, f = M.block_inputs(seed, 1, N)
    tag = "h%d_l%d_n%d" % (heads, layers, N)
    ops.unfused_calls.clear()
    x, fe = torch.from_numpy(xyz).to(dev), torch.from_numpy(f).to(dev)
    with torch.no_grad():
        res1, none = blk(x, fe, want_attn=False)                    # one frame: the row-job chain
        res2, attn2 = blk(x, fe)                                    # with attn: the pair kernel
        B = ops.ONE_FRAME_MAX_POINTS // N + 1                       # many points: the pair kernel, B copies of the cloud
        res3, attn3 = blk(x.expand(B, -1, -1).contiguous(), fe.expand(B, -1, -1).contiguous())
    torch.cuda.synchronize()
    assert none is None and not ops.unfused_calls, ops.unfused_calls
    assert tuple(attn2.shape) == (heads, N, 16, 512 // heads) and tuple(attn3.shape) == (B * heads, N, 16, 512 // heads)
    for r in (res1, res2, res3[:1], res3[-1:]):
        np.testing.assert_allclose(r[..., ::4].cpu().numpy(), g19["res_" + tag], **TOL)
    for a in (attn2, attn3[:heads], attn3[-heads:]):
        np.testing.assert_allclose(a[:, ::16, :, ::8].cpu().numpy(), g19["attn_" + tag], **TOL)


@pytest.mark.parametrize("heads,layers", [(1, 1), (2, 1), (4, 1), (4, 2), (8, 1)])
@pytest.mark.parametrize("N", (128, 64))
def test_fused_b48_against_float64(dev, heads, layers, N):
    seed = 4800 + 10 * heads + layers + N
    blk = _block(heads, layers, seed, dev)
    xyz, f = synth.frames(seed, 48, N, 64, K_s=N)[0], np.random.RandomState(seed).standard_normal((48, N, 256)).astype(np.float32)
    x, fe = torch.from_numpy(xyz).to(dev), torch.from_numpy(f).to(dev)
    ops.unfused_calls.clear()
    with torch.no_grad():
        got, attn = blk(x, fe)
        got_na, _ = blk(x, fe, want_attn=False)
    torch.cuda.synchronize()
    assert not ops.unfused_calls, ops.unfused_calls
    assert torch.equal(got, got_na)
    ref64 = MulTransformerBlock(256, 512, 16, heads, layers).to(dev).double().eval()
    ref64.load_state_dict(blk.state_dict())
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref, attn64 = ref64(x.double(), fe.double())                # the stock path (float64 is outside the fused set)
    ops.unfused_calls.clear()
    # fp32 against fp64 through `layers` LayerNorms: the observed count outside 1e-4 is asserted, not a looser bar
    n_out, worst = outside(got, ref)
    # neighbours at equal distance may come in another order from the stock path's argsort: compare each point's
    # attention values as a set over its 16 neighbours (per channel)
    n_att, worst_a = outside(attn.sort(dim=2)[0], attn64.sort(dim=2)[0])
    print("B=48 N=%d heads=%d layers=%d: res %d outside 1e-4 (worst %.3f units), attn %d (worst %.3f)"
          % (N, heads, layers, n_out, worst, n_att, worst_a))
    assert n_out == 0 and n_att == 0


def test_out_of_set_heads_warn_once_and_match(dev, g19):
    heads, layers, N = 16, 1, 128
    seed = M.block_seed(heads, layers, N)
    blk = _block(heads, layers, seed, dev)
    xyz, f = M.block_inputs(seed, 1, N)
    ops.unfused_calls.clear()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        with torch.no_grad():
            for _ in range(2):
                res, attn = blk(torch.from_numpy(xyz).to(dev), torch.from_numpy(f).to(dev))
    msgs = [str(x.message) for x in w if "MulTransformerBlock" in str(x.message)]
    assert len(msgs) == 1, msgs
    assert sum(ops.unfused_calls.values()) == 2
    np.testing.assert_allclose(res[..., ::4].cpu().numpy(), g19["res_h16_l1_n128"], **TOL)
    np.testing.assert_allclose(attn[:, ::16, :, ::8].cpu().numpy(), g19["attn_h16_l1_n128"], **TOL)
    ops.unfused_calls.clear()


def _tracker(dev, seed=1919):
    from ptt_amd.config import StubDataset, ptt_model_cfg
    from ptt_amd.models import build_network
    return M.seeded_(build_network(M.tracker_cfg(ptt_model_cfg()), 1, StubDataset()), seed).to(dev).eval()


def test_g19_tracker_against_reference(dev, g19):
    """G6's comparison for the tracker whose both transformer blocks are MulTransformerBlock(4 heads, 2 layers)."""
    model = _tracker(dev, int(g19["tracker_seed"]))
    s, t = synth.frames(int(g19["tracker_seed"]), 2, 1024, 512)
    ops.unfused_calls.clear()
    with torch.no_grad():
        out = model({'search_points': torch.from_numpy(s).to(dev), 'template_points': torch.from_numpy(t).to(dev),
                     'batch_size': 2})
    assert not ops.unfused_calls, ops.unfused_calls
    g = {k[len("tracker_"):]: g19[k] for k in g19.files if k.startswith("tracker_")}
    for k in ('search_inds', 'template_inds'):
        np.testing.assert_array_equal(out[k].cpu().numpy(), g[k])
    worst, over = {}, {}
    for k in ('cosine_feats', 'pred_centroids_cls', 'pred_centroids_votes', 'votes_feats'):
        got = out[k].cpu().numpy()
        units = np.abs(got - g[k]) / (1e-4 + 1e-4 * np.abs(g[k]))
        worst[k], over[k] = float(units.max()), int((units > 1.0).sum())
        assert over[k] <= 2 and worst[k] <= 2.0, (k, over[k], worst[k])
    tol = dict(atol=2e-4, rtol=2e-4)
    with torch.no_grad():
        box = model.box_voting_head({'pred_centroids_votes': torch.from_numpy(g['pred_centroids_votes']).to(dev),
                                     'votes_feats': torch.from_numpy(g['votes_feats']).to(dev)})
    for k in ('pred_box_center', 'pred_box_data'):
        np.testing.assert_allclose(box[k].cpu().numpy(), g[k], err_msg=k + ' (box head on reference votes)', **tol)
    ours = out['pred_centroids_votes'].cpu().numpy()
    picks_ref, picks_ours = O.fps(g['pred_centroids_votes'], 64), O.fps(ours, 64)
    same = picks_ref == picks_ours
    for k in ('pred_box_center', 'pred_box_data'):
        ok = np.isclose(out[k].cpu().numpy(), g[k], **tol).all(-1)
        assert ok[same].all(), (k, int((~ok[same]).sum()))
    for b in range(same.shape[0]):
        if same[b].all():
            continue
        j = int(np.argmin(same[b]))
        pts = g['pred_centroids_votes'][b].astype(np.float32)
        md = np.full(pts.shape[0], 1e10, np.float32)
        for i in picks_ref[b, :j]:
            d = pts - pts[i]
            md = np.minimum(md, (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        top = np.sort(md)[::-1]
        assert (top[0] - top[1]) <= 1e-5 * top[0], ("FPS pick %d of frame %d differs without a near-tie" % (j, b), top[:2])
    print("G19 tracker: worst %s, outside %s, %d flipped FPS picks" % (worst, over, int((~same).sum())))


@pytest.mark.parametrize("batch,lengths", [(1, [6]), (6, [4, 3, 5, 2, 4])])
def test_tracklet_runner_replay_and_reload(dev, batch, lengths):
    from ptt_amd.tracklet_runner import TrackletRunner
    tracker = _tracker(dev, 1919)
    with torch.no_grad():                                  # small regression outputs keep the boxes on their objects
        tracker.box_voting_head.refine_layer[-1].conv.weight.mul_(0.05)
        tracker.box_voting_head.refine_layer[-1].conv.bias.mul_(0.05)
    tracklets = [synth.tracklet(300 + k, T) for k, T in enumerate(lengths)]
    ops.unfused_calls.clear()
    runner = TrackletRunner(tracker, dev, batch=batch)
    got_a = runner.run(tracklets)
    eager = TrackletRunner(tracker, dev, batch=batch, use_graph=False).run(tracklets)
    assert not ops.unfused_calls, ops.unfused_calls

    def same(a, b):
        assert len(a) == len(b)
        for ra, rb in zip(a, b):
            assert len(ra) == len(rb)
            for x, y in zip(ra, rb):
                np.testing.assert_array_equal(x[0], y[0])
                np.testing.assert_array_equal(x[2], y[2])
    same(got_a, eager)
    other = _tracker(dev, 2020)
    with torch.no_grad():
        other.box_voting_head.refine_layer[-1].conv.weight.mul_(0.05)
        other.box_voting_head.refine_layer[-1].conv.bias.mul_(0.05)
    tracker.load_state_dict(other.state_dict())
    got_b = runner.run(tracklets)
    same(got_b, TrackletRunner(tracker, dev, batch=batch).run(tracklets))
    assert any(not np.array_equal(x[0], y[0]) for ra, rb in zip(got_a, got_b) for x, y in zip(ra, rb))


def test_train_mode_block_step_matches_g19(dev, g19):
    heads, layers = M.TRAIN
    blk = M.seeded_(MulTransformerBlock(256, 512, 16, heads, layers), 1990).to(dev).train()
    xyz, f = M.block_inputs(1990, 2, 64)
    res, _ = blk(torch.from_numpy(xyz).to(dev), torch.from_numpy(f).to(dev))
    loss = (res * M.loss_weights(1990, tuple(res.shape)).to(dev)).sum()
    loss.backward()
    np.testing.assert_allclose(loss.item(), float(g19["train_loss"]), rtol=1e-4)
    norms = np.array([p.grad.double().norm().item() for p in blk.parameters()])
    # fc_gamma[2].bias cancels in the softmax: its gradient is rounding noise (~2e-6) on either side, hence the atol
    np.testing.assert_allclose(norms, g19["train_grad_norms"], rtol=1e-3, atol=1e-4)
    for i in range(layers):
        np.testing.assert_allclose(blk.layers[i].fc_gamma[0].weight.grad.cpu().numpy(), g19["train_g_fc_gamma0_w_%d" % i],
                                   **TOL)
        np.testing.assert_allclose(blk.layers[i].norm1.weight.grad.cpu().numpy(), g19["train_g_norm1_w_%d" % i], **TOL)
    np.testing.assert_allclose(blk.layers[-1].proj.weight.grad[::8].cpu().numpy(), g19["train_g_proj_w_last_rows8"], **TOL)
