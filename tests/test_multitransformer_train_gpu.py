"""MulTransformerBlock in TRAINING mode on the HIP row kernels (train_ops.mul_block_usable -> _AttnCore with heads, _RowsLayerNorm)
against fixture G20 — the reference's own forward + backward in float32 and in float64 — plus the path, determinism, GradSink and
captured-step checks.

Values: for every gradient g (each parameter, features, xyz), over the entries G20 samples,
    e_ref = |g_ref32 - g_ref64| / |g_ref64|      the reference's own float32 distance from float64
    e_hip = |g_hip   - g_ref64| / |g_ref64|
and the bar is e_hip <= 4 e_ref + 1e-6: a float32 run with another legitimate summation order lands within a small multiple of the
reference's own rounding. fc_gamma.2.bias cancels in the softmax (true gradient 0, both sides rounding noise): atol 1e-4 only."""
import os

import numpy as np
import pytest
import torch

from ptt_amd import ops, train_ops
from ptt_amd.models.transformer_block.multitransformer import MulTransformerBlock
from tests import multitransformer_ref as M
from tests import multitransformer_train_ref as T

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def g20():
    return np.load(os.path.join(GOLD, "G20_multitransformer_train.npz"))


def _run(dev, heads, layers, k=16, drop=0.0, sink=False, want_attn=True):
    """One training-mode forward + backward from G20's seeds -> (block, loss, res, xyz, features[, sink])."""
    seed = T.train_seed(heads, layers)
    blk = M.seeded_(MulTransformerBlock(256, 512, k, heads, layers), seed).to(dev).train()
    for layer in blk.layers:
        layer.proj_drop.p = drop
    xyz, f = M.block_inputs(seed, T.B, T.N)
    xyz = torch.from_numpy(xyz).to(dev).requires_grad_(True)
    f = torch.from_numpy(f).to(dev).requires_grad_(True)
    gs = train_ops.GradSink(list(blk.parameters()), dev) if sink else None
    res, attn = blk(xyz, f, want_attn=want_attn)
    loss = (res * M.loss_weights(seed, tuple(res.shape)).to(dev)).sum()
    if gs is not None:
        with gs.collecting():
            loss.backward()
        gs.flush()
    else:
        loss.backward()
    torch.cuda.synchronize()
    return blk, loss, res, xyz, f, attn, gs


class _Forbidden(RuntimeError):
    pass


def _forbid(monkeypatch):
    def boom(*a, **kw):
        raise _Forbidden("a stock torch op of the reference path ran")
    monkeypatch.setattr(torch.nn.functional, "layer_norm", boom)
    monkeypatch.setattr(torch.nn.functional, "softmax", boom)
    monkeypatch.setattr(torch.Tensor, "argsort", boom)


@pytest.mark.parametrize("heads,layers", T.BLOCKS)
def test_training_step_runs_on_the_row_kernels(dev, monkeypatch, heads, layers):
    _forbid(monkeypatch)
    blk, loss, res, xyz, f, attn, _ = _run(dev, heads, layers)
    assert bool(torch.isfinite(loss)) and all(p.grad is not None for p in blk.parameters())
    assert xyz.grad is not None and f.grad is not None
    assert tuple(attn.shape) == (T.B * heads, T.N, 16, 512 // heads) and not attn.requires_grad
    assert _run(dev, heads, layers, want_attn=False)[5] is None


@pytest.mark.parametrize("kw", (dict(heads=16), dict(drop=0.1), dict(k=8)))
def test_outside_the_envelope_the_stock_path_still_runs(dev, monkeypatch, kw):
    args = dict(heads=4, layers=1, k=16, drop=0.0)
    args.update(kw)
    blk = MulTransformerBlock(256, 512, args["k"], args["heads"], 1).to(dev).train()
    for layer in blk.layers:
        layer.proj_drop.p = args["drop"]
    xyz, f = M.block_inputs(7, T.B, T.N)
    xyz, f = torch.from_numpy(xyz).to(dev), torch.from_numpy(f).to(dev)
    assert not train_ops.mul_block_usable(blk, xyz, f)
    res, _ = blk(xyz, f)                                    # the fallback exists ...
    assert bool(torch.isfinite(res).all())
    _forbid(monkeypatch)
    with pytest.raises(_Forbidden):                         # ... and is the reference's op sequence
        blk(xyz, f)


@pytest.mark.parametrize("heads,layers", T.BLOCKS)
def test_values_against_g20(dev, g20, heads, layers):
    tag = "h%d_l%d" % (heads, layers)
    seed = T.train_seed(heads, layers)
    xyz_np, _ = M.block_inputs(seed, T.B, T.N)
    knn = ops.knn(torch.from_numpy(xyz_np).to(dev), 16)
    knn = (knn[0] if isinstance(knn, tuple) else knn).cpu().numpy().astype(np.int64)
    # the same table as the reference's argsort — up to the order of exactly tied distances: block_inputs repeats every point
    # (second half = first half), and argsort's order inside a tie is its own. Where the two tables differ the float64 distances
    # must be equal position by position, and every point's neighbour SET must be the same: a neighbour swapped at a near-tie
    # would show up as a large gradient error that has nothing to do with the kernels
    ref_knn = g20["knn_" + tag].astype(np.int64)
    x64 = xyz_np.astype(np.float64)
    d = ((x64[:, :, None] - x64[:, None]) ** 2).sum(-1)
    assert np.array_equal(np.take_along_axis(d, knn, 2), np.take_along_axis(d, ref_knn, 2)), "kNN: another distance at some rank"
    assert np.array_equal(np.sort(knn, 2), np.sort(ref_knn, 2)), "the kNN sets differ from the reference's"
    blk, loss, res, xyz, f, _, _ = _run(dev, heads, layers)
    names = list(g20["names_" + tag])
    assert [n for n, _ in blk.named_parameters()] + ["features", "xyz"] == names
    grads = [p.grad for p in blk.parameters()] + [f.grad, xyz.grad]
    shapes = [tuple(g.shape) for g in grads]
    ref32, ref64 = T.split(names, shapes, g20["g32_" + tag]), T.split(names, shapes, g20["g64_" + tag])
    l64, l32 = float(g20["loss64_" + tag]), float(g20["loss32_" + tag])
    print("\n%s loss: hip %.9g ref32 %.9g ref64 %.9g" % (tag, loss.item(), l32, l64))
    r64 = g20["res64_" + tag]
    e_res_ref = np.linalg.norm(g20["res32_" + tag] - r64) / np.linalg.norm(r64)
    e_res_hip = np.linalg.norm(res.detach()[..., ::4].cpu().numpy() - r64) / np.linalg.norm(r64)
    print("%-32s e_ref %.3e  e_hip %.3e" % ("res", e_res_ref, e_res_hip))
    norms = np.array([g.double().norm().item() for g in grads])
    bad, bars = [], {}
    print("%-32s %-10s %-10s %-8s" % ("gradient", "e_ref", "e_hip", "ratio"))
    for n, g, nrm in zip(names, grads, norms):
        got = T.sample(g.cpu().numpy()).astype(np.float64)
        if n.endswith("fc_gamma.2.bias"):
            worst = float(np.abs(got - ref64[n]).max())
            print("%-32s max |g - g_ref64| %.3e (atol 1e-4)" % (n, worst))
            if not worst <= 1e-4:
                bad.append((n, worst))
            continue
        d = np.linalg.norm(ref64[n])
        e_ref = np.linalg.norm(ref32[n].astype(np.float64) - ref64[n]) / d
        e_hip = np.linalg.norm(got - ref64[n]) / d
        print("%-32s %.3e  %.3e  %.2f" % (n, e_ref, e_hip, e_hip / max(e_ref, 1e-30)))
        bars[n] = 4.0 * e_ref + 1e-6
        if not e_hip <= bars[n]:
            bad.append((n, e_ref, e_hip))
    assert e_res_hip <= 4.0 * e_res_ref + 1e-6, (e_res_ref, e_res_hip)
    # the loss is the inner product <res, w>: |loss - loss64| <= |res - res64| |w| (Cauchy-Schwarz), with res under the bar above;
    # |res64| from its stored quarter (every fourth channel: a factor 2 in the norm)
    wnorm = float(M.loss_weights(seed, tuple(res.shape)).double().norm())
    loss_bar = (4.0 * e_res_ref + 1e-6) * 2.0 * float(np.linalg.norm(r64)) * wnorm
    print("loss: |hip - ref64| %.3e, |ref32 - ref64| %.3e, bar %.3e" % (abs(loss.item() - l64), abs(l32 - l64), loss_bar))
    assert abs(loss.item() - l64) <= loss_bar, (loss.item(), l32, l64, loss_bar)
    # a norm moves by at most the distance of the vectors (triangle inequality): the gradient's own bar bounds its norm's error
    n64 = g20["norms64_" + tag]
    for i, n in enumerate(names):
        if n in bars:
            assert abs(norms[i] - n64[i]) / n64[i] <= bars[n], (n, norms[i], n64[i], bars[n])
    assert not bad, bad


def test_one_head_takes_transformer_blocks_dt_launch(dev, monkeypatch):
    """heads = 1: the group-sum GEMM that forms dt is the very launch TransformerBlock's training step uses, never the heads form."""
    calls = []
    real1, realh = ops.rows_gemm_rsum16, ops.rows_gemm_rsum16_heads
    monkeypatch.setattr(ops, "rows_gemm_rsum16", lambda *a, **kw: (calls.append("rsum16"), real1(*a, **kw))[1])
    monkeypatch.setattr(ops, "rows_gemm_rsum16_heads", lambda *a, **kw: (calls.append("rsum16_heads"), realh(*a, **kw))[1])
    _run(dev, 1, 1)
    assert calls == ["rsum16"], calls
    from ptt_amd.models.transformer_block.variants import TransformerBlock
    del calls[:]
    blk = TransformerBlock(256, 512, 16).to(dev).train()
    xyz, f = M.block_inputs(3, T.B, T.N)
    blk(torch.from_numpy(xyz).to(dev), torch.from_numpy(f).to(dev).requires_grad_(True))[0].sum().backward()
    assert calls == ["rsum16"], calls
    for heads, want in ((2, ["rsum16_heads"]), (4, ["rsum16_heads"]), (8, [])):     # hd = 64: the three-pass form
        del calls[:]
        _run(dev, heads, 1)
        assert calls == want, (heads, calls)


@pytest.mark.parametrize("heads,layers", T.BLOCKS)
def test_two_runs_give_identical_gradients(dev, heads, layers):
    a = _run(dev, heads, layers)
    b = _run(dev, heads, layers)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    for (n, p), q in zip(a[0].named_parameters(), b[0].parameters()):
        assert torch.equal(p.grad, q.grad), n
    assert torch.equal(a[3].grad, b[3].grad) and torch.equal(a[4].grad, b[4].grad)


@pytest.mark.parametrize("heads,layers", ((4, 2), (8, 1)))
def test_grad_sink_holds_the_same_gradients(dev, heads, layers):
    """The flat buffer of a GradSink against the per-parameter gradients of a run without it, bitwise: both finishes fold a
    gradient's row-chunk partials with the same group count for the same chunk count (launch_wgrad_finish follows
    ops.GradFinishPlan._outputs_per_group)."""
    plain = _run(dev, heads, layers)
    sunk = _run(dev, heads, layers, sink=True)
    gs = sunk[6]
    assert train_ops.GradSink.active is None and not gs.jobs
    lo, hi = gs.flat.data_ptr(), gs.flat.data_ptr() + gs.flat.numel() * 4
    diff = {}
    for (n, p), q in zip(plain[0].named_parameters(), sunk[0].parameters()):
        assert lo <= q.grad.data_ptr() < hi, n
        if not torch.equal(p.grad, q.grad):
            diff[n] = (float((p.grad - q.grad).abs().max()), float(p.grad.abs().max()))
    print("\nGradSink vs per-parameter gradients, (heads, layers) = (%d, %d): %d of %d parameters differ" % (heads, layers, len(diff), len(sunk[0].state_dict())))
    for n, (e, m) in diff.items():
        print("  %-32s max |diff| %.3e (max |g| %.3e)" % (n, e, m))
    assert not diff, diff


# ------------------------------------------------------------------ the captured training step (tests/test_train_graph_gpu.py's protocol)
def _trainer(dev, graph):
    from ptt_amd.config import StubDataset, ptt_model_cfg
    from ptt_amd.models import build_network
    from ptt_amd.train_step import DataParallelTrainer
    torch.manual_seed(1)
    model = build_network(M.tracker_cfg(ptt_model_cfg()), 1, StubDataset(training=True)).to(dev).train()
    return DataParallelTrainer(model, dev, graph=graph)


def _same_state(a, b):
    bad = [k for (k, p), q in zip(a.tracker.state_dict().items(), b.tracker.state_dict().values()) if not torch.equal(p, q)]
    for p, q in zip(a.optimizer.param_groups[0]['params'], b.optimizer.param_groups[0]['params']):
        sa, sb = a.optimizer.state[p], b.optimizer.state[q]
        if not (torch.equal(sa['exp_avg'], sb['exp_avg']) and torch.equal(sa['exp_avg_sq'], sb['exp_avg_sq']) and float(sa['step']) == float(sb['step'])):
            bad.append("adam state")
            break
    if not torch.equal(a.sink.flat, b.sink.flat):
        bad.append("flat gradient buffer")
    if not torch.equal(a.optimizer.last_norm, b.optimizer.last_norm):
        bad.append("clipped norm")
    return bad


def test_replayed_tracker_step_is_bit_identical_to_the_eager_step(dev, monkeypatch):
    from ptt_amd.train_step import synthetic_train_batch
    eager, graphed = _trainer(dev, False), _trainer(dev, True)
    batches = [synthetic_train_batch(100 + k, 8, dev) for k in range(3)]
    calls, real = [], ops.layernorm_train_fwd               # both heads' blocks go through the row kernels
    monkeypatch.setattr(ops, "layernorm_train_fwd", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    for k in range(9):
        if k == 6:
            for t in (eager, graphed):
                t.optimizer.param_groups[0]['lr'] *= 0.5
        le = eager.step(batches[k % 3]).detach().clone()
        lg = graphed.step(batches[k % 3]).detach().clone()
        torch.cuda.synchronize()
        assert torch.equal(le, lg) and bool(torch.isfinite(lg)), (k, float(le), float(lg))
        assert not _same_state(eager, graphed), (k, _same_state(eager, graphed))
        assert (graphed.captured is not None) == (k >= 3) and eager.captured is None
    assert graphed.graph_steps == 6 and graphed.eager_steps == 3
    # per forward pass 2 LayerNorms x 2 layers x 2 blocks (x 2 where a head runs its block on both branches): eager 9, graphed 3 + capture
    assert len(calls) >= (9 + 4) * 8, len(calls)
