"""ClipAdamW / ClipSGD (ptt_amd/optim.py) on ptt_optim_clip_step_f32 and its device-hyper form, on the device: against
clip_grad_norm_ + the stock foreach optimizers, captured and replayed against eager, behind guard bands, on fixture G25's
trajectories, and inside DataParallelTrainer (optimizer= / scheduler= / from_optim_cfg). The bars are those of
tests/test_step_ops_gpu.py for ClipAdam against torch (parameters 1e-6 max|ref| + 2e-9, moments and .grad 2e-6 of their scale) and
bit-identity wherever two forms of the SAME arithmetic are compared (captured / eager, graph / eager trainers)."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

from ptt_amd.config import EasyDict
from tests import guard
from tests import optimization_ref as S

pytestmark = pytest.mark.gpu

SHAPES = [(64, 67), (4100,), (1,), (3, 5, 7), (256, 256), (9000,)]      # one element; one chunk + 4 elements; over two chunks
KINDS = {"adamw": dict(lr=1e-3, betas=(0.5, 0.999), eps=1e-6), "sgd_momentum": dict(lr=1e-2, momentum=0.9), "sgd_plain": dict(lr=1e-2, momentum=0)}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def g25():
    return np.load(S.GOLDEN)


def _classes(kind):
    from ptt_amd.optim import ClipAdamW, ClipSGD
    return (ClipAdamW, torch.optim.AdamW) if kind == "adamw" else (ClipSGD, torch.optim.SGD)


def _params(dev, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(*s, generator=g).to(dev)) for s in SHAPES]


def _grouped(params, kw, wd, groups):
    """The constructor arguments: one group, or two groups (tensors 0-2 | 3-5) of different lr and weight decay."""
    if groups == 1:
        return [dict(params=params)], dict(kw, weight_decay=wd)
    return ([dict(params=params[:3]), dict(params=params[3:], lr=kw['lr'] * 3.0, weight_decay=wd * 0.5 + 0.002)], dict(kw, weight_decay=wd))


def _compare(kind, oa, ob, pa, pb, gmax, step):
    for p, q in zip(pa, pb):
        assert float((p.detach() - q.detach()).abs().max()) <= 1e-6 * float(q.detach().abs().max()) + 2e-9, (step, tuple(p.shape))
        assert float((p.grad - q.grad).abs().max()) <= 2e-6 * float(q.grad.abs().max()) + 1e-12
        gmax[id(q)] = max(gmax.get(id(q), 0.0), float(q.grad.abs().max()))
        keys = ('exp_avg', 'exp_avg_sq') if kind == "adamw" else (('momentum_buffer',) if kind == "sgd_momentum" else ())
        for key in keys:
            a, b = oa.state[p][key], ob.state[q][key]
            # a moment of a single element can cancel: the bar is relative to the gradients that went into it
            ref_scale = max(float(b.abs().max()), gmax[id(q)] ** (2 if key == 'exp_avg_sq' else 1))
            assert float((a - b).abs().max()) <= 2e-6 * ref_scale + 1e-12, (step, key)
        if kind == "adamw":
            assert float(oa.state[p]['step']) == float(ob.state[q]['step']) == step + 1
        if kind == "sgd_plain":
            assert 'momentum_buffer' not in oa.state.get(p, {})


@pytest.mark.parametrize("groups,moving", [(1, False), (2, False), (2, True)])
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("max_norm,scale", [(10.0, 1.0), (10.0, 300.0), (None, 1.0), (None, 300.0), (10.0, 0.01)])
@pytest.mark.parametrize("kind", list(KINDS))
def test_fused_step_equals_clip_grad_norm_then_the_stock_optimizer(dev, kind, max_norm, scale, wd, groups, moving):
    """Three steps on identical gradients. scale 1 and 300 put the norm (about 288 scale) above max_norm = 10, scale 0.01 below it:
    the clip inactive. groups = 2: different lr and weight decay under ONE norm. moving: lr and beta1 / momentum changed before
    every step, as a OneCycle schedule does."""
    mine_cls, stock_cls = _classes(kind)
    pa, pb = _params(dev), _params(dev)
    ga, kwa = _grouped(pa, KINDS[kind], wd, groups)
    gb, kwb = _grouped(pb, KINDS[kind], wd, groups)
    oa, ob = mine_cls(ga, **kwa), stock_cls(gb, foreach=True, **kwb)
    gg = torch.Generator().manual_seed(9)
    gmax = {}
    for step in range(3):
        if moving:
            for opt in (oa, ob):
                for g in opt.param_groups:
                    g['lr'] = g['lr'] * (1.7 if step == 1 else 0.6)
                    if kind == "adamw":
                        g['betas'] = (0.95 - 0.04 * step, g['betas'][1])
                    elif kind == "sgd_momentum":
                        g['momentum'] = 0.95 - 0.04 * step
        grads = [torch.randn(*s, generator=gg).to(dev) * scale * (1 + step) for s in SHAPES]
        for p, q, gr in zip(pa, pb, grads):
            p.grad, q.grad = gr.clone(), gr.clone()
        oa.step(max_norm=max_norm)
        assert oa._table is not None and oa._table[1].n_groups == groups            # the fused path, ONE table
        if max_norm is not None:
            norm = torch.nn.utils.clip_grad_norm_(pb, max_norm)
            assert abs(float(oa.last_norm) - float(norm)) <= 2e-6 * float(norm)
            assert (float(norm) > max_norm) == (scale >= 1.0)
        ob.step()
        _compare(kind, oa, ob, pa, pb, gmax, step)
    ob.load_state_dict(oa.state_dict())
    oa.load_state_dict(ob.state_dict())


def test_what_the_table_cannot_hold_takes_the_stock_path(dev):
    """A float64 parameter, amsgrad, nesterov, dampening: clip_grad_norm_ + the stock step, no table."""
    from ptt_amd.optim import ClipAdamW, ClipSGD
    cases = [(lambda ps: ClipAdamW(ps, lr=0.1, weight_decay=0.0), torch.float64),
             (lambda ps: ClipAdamW(ps, lr=0.1, weight_decay=0.0, amsgrad=True), torch.float32),
             (lambda ps: ClipSGD(ps, lr=0.1, momentum=0.9, nesterov=True), torch.float32),
             (lambda ps: ClipSGD(ps, lr=0.1, momentum=0.9, dampening=0.5), torch.float32)]
    for make, second in cases:
        ps = [torch.nn.Parameter(torch.ones(10, device=dev)), torch.nn.Parameter(torch.ones(10, device=dev, dtype=second))]
        o = make(ps)
        for p in ps:
            p.grad = torch.ones_like(p)
        o.step(max_norm=1.0)
        assert o._table is None
        assert abs(float(o.last_norm) - 20 ** 0.5) < 1e-5
        if not o.defaults.get('nesterov'):                      # torch's foreach nesterov step adds momentum * buf INTO .grad
            assert abs(float(ps[0].grad[0]) - 1.0 / 20 ** 0.5) < 1e-6
        assert float(ps[0].detach()[0]) < 1.0 and float(ps[1].detach()[0]) < 1.0


# ------------------------------------------------------------------------------------------------------------- captured form
@pytest.mark.parametrize("kind", ["adamw", "sgd_momentum"])
def test_captured_step_replays_bit_identically_to_eager_steps(dev, kind):
    """record_graph_step under torch.cuda.graph, two groups, clipping on; six replays with OneCycle moving lr and beta1 / momentum
    between them, against six eager steps from the same start: the header promises identical arithmetic."""
    from ptt_amd.optimization import OneCycle
    mine_cls, _ = _classes(kind)
    twins = []
    for _ in range(2):
        ps = _params(dev)
        groups, kw = _grouped(ps, KINDS[kind], 0.01, 2)
        opt = mine_cls(groups, **kw)
        for p in ps:
            p.grad = torch.zeros_like(p)                       # gradients that live in one place, refilled every step
        twins.append((ps, opt, OneCycle(opt, 7, KINDS[kind]['lr'], (0.95, 0.85), 10, 0.4)))
    gg = torch.Generator().manual_seed(17)
    all_grads = [[torch.randn(*s, generator=gg).to(dev) * (30.0 if it % 2 else 0.01) for s in SHAPES] for it in range(7)]

    def fill(ps, it):
        torch._foreach_copy_([p.grad for p in ps], all_grads[it])
    for ps, opt, sched in twins:                               # step 0, eager in both: state, table and gradient addresses exist
        sched.step(0)
        fill(ps, 0)
        opt.step(max_norm=10.0)
    (pe, oe, se), (pg, og, sg) = twins
    assert og.prepare_graph_step()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        og.record_graph_step(10.0)
    pinned = og._graph
    for it in range(1, 7):
        se.step(it)
        fill(pe, it)
        oe.step(max_norm=10.0)
        norm_e = oe.last_norm.clone()
        sg.step(it)
        fill(pg, it)
        og.begin_graph_step(10.0)
        graph.replay()
        og.end_graph_step()
        torch.cuda.synchronize()
        assert torch.equal(norm_e, og.last_norm) and (float(norm_e) > 10.0) == bool(it % 2), (it, float(norm_e))
        for p, q in zip(pe, pg):
            assert torch.equal(p, q) and torch.equal(p.grad, q.grad), (it, tuple(p.shape))
            for key in (('exp_avg', 'exp_avg_sq') if kind == "adamw" else ('momentum_buffer',)):
                assert torch.equal(oe.state[p][key], og.state[q][key]), (it, key)
            if kind == "adamw":
                assert float(oe.state[p]['step']) == float(og.state[q]['step']) == it + 1
    assert og._graph is pinned and og._opt_called
    assert all(p._version > 6 for p in pg)                     # the replays told autograd and the weight caches


# --------------------------------------------------------------------------------------------------------------- guard bands
def _guarded_table(dev, kinds_of_group):
    """An ops.OptimTable over 1-D tensors that lie between guard words (parameters, gradients, state), with a guarded partial-sum
    workspace and norm output; rows 0-1 in group 0, row 2 in group 1."""
    from ptt_amd import ops
    g = torch.Generator().manual_seed(23)
    sizes, groups = [4100, 1, 8193], [0, 0, 1]
    mk = lambda n, s=1.0: guard.embed((torch.randn(n, generator=g) * s).to(dev))
    params, grads = [mk(n) for n in sizes], [mk(n, 40.0) for n in sizes]
    st1 = [mk(n, 0.1) for n in sizes]
    st2 = [guard.embed((torch.rand(n, generator=g) * 0.1).to(dev)) if kinds_of_group[gi] != "sgd" else None for n, gi in zip(sizes, groups)]
    table = ops.OptimTable(params, st1, st2, groups, 2)
    table.partial = guard.guarded((table.n_chunks,), torch.float64, device=dev)
    table.norm = guard.guarded((1,), torch.float32, device=dev)
    return table, params, grads, st1, st2


def test_nothing_outside_the_tensors_is_written_and_a_refused_call_writes_nothing(dev):
    from ptt_amd import _lib, ops
    table, params, grads, st1, st2 = _guarded_table(dev, ("adamw", "sgd"))
    views = params + grads + st1 + [s for s in st2 if s is not None]
    hypers = [ops.OptimTable.hyper("adamw", 1e-3, 3, (0.9, 0.99), 1e-8, 0.01), ops.OptimTable.hyper("sgd", 1e-2, weight_decay=0.01, momentum=0.9)]
    plain = [[v.clone() for v in grp] for grp in (params, grads, st1)]
    plain.append([s.clone() if s is not None else None for s in st2])
    ref = ops.OptimTable(plain[0], plain[2], plain[3], [0, 0, 1], 2)
    # one eager step
    table.step(grads, hypers, max_norm=10.0)
    ref.step(plain[1], hypers, max_norm=10.0)
    assert torch.equal(table.norm, ref.norm) and float(ref.norm) > 1000.0                  # the clip is active
    # one device-hyper step (on the gradients the first one left clipped: their norm is max_norm up to rounding)
    ring = ops.AdamHyperRing(dev, nbytes=ctypes.sizeof(_lib.OptimHyper) * 2)
    ring.upload(table.hyper_array(hypers))
    table.step_device_hyper(ring.dev, max_norm=10.0)
    ref.step_device_hyper(ring.dev, max_norm=10.0)
    torch.cuda.synchronize()
    for v in views:
        guard.check_guard(v, all_written=False)
    guard.check_guard(table.partial)                           # every partial sum written, nothing beyond the n_chunks doubles
    guard.check_guard(table.norm)
    assert torch.equal(table.norm, ref.norm) and abs(float(ref.norm) - 10.0) < 1e-4
    for got, want in zip(params + grads + st1 + [st2[0], st2[1]], plain[0] + plain[1] + plain[2] + plain[3][:2]):
        assert torch.equal(got, want)                          # the same bits as between ordinary allocations
    # refused calls: nothing launched, every word where it was
    before = [v._guard.words.clone() for v in views + [table.partial, table.norm]]
    args = lambda n_groups, partial_elems: (guard.ptr(table.table), table.host.data_ptr(), len(table.rows), guard.ptr(table.which),
                                            guard.ptr(table.first), table.n_chunks, table.hyper_array(hypers), n_groups, 10.0, 1,
                                            guard.ptr(table.partial), partial_elems, guard.ptr(table.norm))
    with pytest.raises(RuntimeError, match="PTT_EINVAL"):
        guard.launch("ptt_optim_clip_step_f32", dev, *args(0, table.n_chunks))
    with pytest.raises(RuntimeError, match="PTT_EINVAL"):
        guard.launch("ptt_optim_clip_step_f32", dev, *args(1, table.n_chunks))             # row 2 names group 1
    with pytest.raises(RuntimeError, match="PTT_EWORKSPACE"):
        guard.launch("ptt_optim_clip_step_f32", dev, *args(2, table.n_chunks - 1))
    dev_args = lambda n_groups, partial_elems: args(n_groups, partial_elems)[:6] + (guard.ptr(ring.dev),) + args(n_groups, partial_elems)[7:]
    with pytest.raises(RuntimeError, match="PTT_EINVAL"):
        guard.launch("ptt_optim_clip_step_dev_f32", dev, *dev_args(1, table.n_chunks))
    with pytest.raises(RuntimeError, match="PTT_EWORKSPACE"):
        guard.launch("ptt_optim_clip_step_dev_f32", dev, *dev_args(2, table.n_chunks - 1))
    torch.cuda.synchronize()
    for v, b in zip(views + [table.partial, table.norm], before):
        assert torch.equal(v._guard.words, b)


# ------------------------------------------------------------------------------------------------------- fixture on the device
@pytest.mark.parametrize("name", ["adamw", "sgd", "adam_onecycle"])
def test_G25_trajectories_on_the_device(dev, g25, name):
    from ptt_amd.optimization import build_optimizer, build_scheduler
    cfg = S.optim_cfg(name, EasyDict)
    model = S.toy().to(dev)
    opt = build_optimizer(model, cfg)
    sched = build_scheduler(opt, S.STEPS, 1, -1, cfg)[0] if name == "adam_onecycle" else None
    got = S.run_trajectory(model, opt, sched, lambda: opt.step(max_norm=cfg.GRAD_NORM_CLIP))
    assert opt._table is not None and opt._table[1].n_groups == len(opt.param_groups)
    sizes = S.param_sizes(model)
    for k in S.RECORD:
        excess, worst = S.params_excess(got[k], g25["traj_%s_p%d" % (name, k)], sizes)
        print("%s after step %d: largest parameter difference %.2e" % (name, k, worst))
        assert excess <= 0, (name, k, worst)
    assert abs(float(opt.last_norm) - g25["traj_%s_norms" % name][-1]) <= 2e-6 * g25["traj_%s_norms" % name][-1]
    for key, v in S.flat_state(model, opt, name).items():
        ref = g25["traj_%s_state_%s" % (name, key)]
        if key == "step":
            assert np.array_equal(v, ref)
        else:
            excess, worst = S.moments_excess(v, ref, S.state_sizes(model, opt))
            assert excess <= 0, (name, key, worst)


# ------------------------------------------------------------------------------------------------------------------ trainer
def _model(dev, seed=1):
    from ptt_amd.config import StubDataset, ptt_model_cfg
    from ptt_amd.models import build_network
    torch.manual_seed(seed)
    return build_network(ptt_model_cfg(), 1, StubDataset(training=True)).to(dev).train()


def _onecycle_trainer(dev, graph, total=7, pct=0.5, **kw):
    from ptt_amd.optimization import OneCycle, build_optimizer
    from ptt_amd.train_step import DataParallelTrainer
    model = _model(dev)
    opt = build_optimizer(model, S.optim_cfg("adam_onecycle", EasyDict))
    return DataParallelTrainer(model, dev, optimizer=opt, scheduler=OneCycle(opt, total, S.LR_MAX, S.MOMS, S.DIV_FACTOR, pct), graph=graph, **kw)


def test_trainer_with_adam_onecycle_replays_bit_identically_to_its_eager_twin(dev, g25):
    from ptt_amd.train_step import synthetic_train_batch
    eager, graphed = _onecycle_trainer(dev, False), _onecycle_trainer(dev, True, graph_warmup=3)
    batches = [synthetic_train_batch(300 + k, 2, dev) for k in range(3)]
    ref_lr, ref_mom = g25["sched_7_0.5_lr"], g25["sched_7_0.5_mom"]
    for k in range(7):
        le = eager.step(batches[k % 3]).detach().clone()
        lg = graphed.step(batches[k % 3]).detach().clone()
        torch.cuda.synchronize()
        assert torch.equal(le, lg) and bool(torch.isfinite(lg)), (k, float(le), float(lg))
        for (n, p), (_, q) in zip(eager.tracker.named_parameters(), graphed.tracker.named_parameters()):
            assert torch.equal(p, q), (k, n)
        assert torch.equal(eager.optimizer.last_norm, graphed.optimizer.last_norm)
        for t in (eager, graphed):
            assert abs(float(t.optimizer.lr) - ref_lr[k]) <= 1e-14 * ref_lr[k] and abs(t.optimizer.mom - ref_mom[k]) <= 1e-14 * ref_mom[k]
            assert all(g['lr'] == t.optimizer.lr for g in t.optimizer.param_groups)
    assert graphed.graph_steps == 4 and graphed.eager_steps == 3 and eager.graph_steps == 0
    assert graphed.captured is not None and graphed.captured.valid(graphed)
    for p, q in zip(eager.tracker.parameters(), graphed.tracker.parameters()):
        for key in ('exp_avg', 'exp_avg_sq'):
            assert torch.equal(eager.optimizer.state[p][key], graphed.optimizer.state[q][key])


def test_trainer_with_adam_onecycle_tracks_the_references_sequence_on_stock_torch(dev):
    """Three eager trainer steps against the reference's own sequence (fastai_optim.py:132-149 after train_utils.py:26-50) on the
    gradients the trainer's optimizer received: OneCycle sets lr and beta1; clip_grad_norm_; p.mul_(1 - wd * lr) on every trainable
    parameter; torch.optim.Adam(weight_decay=0).step(). Every parameter within 1e-6 max|ref| + 2e-9 after every step."""
    from ptt_amd.optimization import OneCycle
    from ptt_amd.train_step import synthetic_train_batch
    wd = 0.01
    trainer = _onecycle_trainer(dev, False, total=3, pct=0.4)
    seen = []
    fused_step = trainer.optimizer.step
    held = [p for g in trainer.optimizer.param_groups for p in g['params']]

    def spy(*a, **kw):
        seen.append([p.grad.detach().clone() for p in held])
        return fused_step(*a, **kw)
    trainer.optimizer.step = spy
    twin = [torch.nn.Parameter(p.detach().clone()) for p in held]
    stock = torch.optim.Adam(twin, lr=3e-3, betas=(0.9, 0.99), weight_decay=0, foreach=True)
    sched = OneCycle(stock, 3, S.LR_MAX, S.MOMS, S.DIV_FACTOR, 0.4)
    worst = 0.0
    for it in range(3):
        trainer.step(synthetic_train_batch(40 + it, 2, dev))
        sched.step(it)
        for q, g in zip(twin, seen[-1]):
            q.grad = g
        norm = torch.nn.utils.clip_grad_norm_(twin, 10.0)
        assert abs(float(trainer.optimizer.last_norm) - float(norm)) <= 2e-6 * float(norm)
        lr = stock.param_groups[0]['lr']
        assert lr == trainer.optimizer.lr and stock.param_groups[0]['betas'][0] == trainer.optimizer.mom
        with torch.no_grad():
            for q in twin:
                q.mul_(1 - wd * lr)
        stock.step()
        for p, q in zip(held, twin):
            d = float((p.detach() - q.detach()).abs().max())
            worst = max(worst, d)
            assert d <= 1e-6 * float(q.detach().abs().max()) + 2e-9, (it, tuple(p.shape), d)
    print("adam_onecycle trainer vs the reference's sequence on stock torch, three steps: largest parameter difference %.2e" % worst)
    assert len(seen) == 3 and trainer.eager_steps == 3


def test_trainer_argument_handling(dev):
    from ptt_amd.optim import ClipAdam, ClipSGD
    from ptt_amd.train_step import DataParallelTrainer, synthetic_train_batch
    batch = synthetic_train_batch(77, 2, dev)

    def trains(trainer, steps=2):
        before = [p.detach().clone() for p in trainer.tracker.parameters()]
        for _ in range(steps):
            loss = trainer.step(batch)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(loss))
        assert any(not torch.equal(a, p) for a, p in zip(before, trainer.tracker.parameters()))
    # sgd from a config: ClipSGD, GRAD_NORM_CLIP, a 'step' schedule kept for the caller's epoch loop
    t = DataParallelTrainer.from_optim_cfg(_model(dev), dev, S.optim_cfg("sgd", EasyDict), 10, 2, graph=False)
    assert type(t.optimizer) is ClipSGD and t.clip == S.CLIP and t.scheduler is None
    assert type(t.epoch_scheduler) is torch.optim.lr_scheduler.StepLR
    trains(t)
    assert t.optimizer._table is not None and t.iteration == 2
    # adam + 'step'
    t = DataParallelTrainer.from_optim_cfg(_model(dev), dev, S.optim_cfg("adam", EasyDict), 10, 2, graph=False)
    assert type(t.optimizer) is ClipAdam and type(t.epoch_scheduler) is torch.optim.lr_scheduler.StepLR
    trains(t)
    # a stock optimizer: no capture protocol, eager steps after clip_grad_norm_
    model = _model(dev)
    t = DataParallelTrainer(model, dev, optimizer=torch.optim.SGD(model.parameters(), lr=1e-3, momentum=0.9), graph_warmup=1)
    assert not t.graph_mode
    trains(t, steps=3)
    assert t.graph_steps == 0 and t.eager_steps == 3 and t.captured is None
    with pytest.raises(ValueError):
        DataParallelTrainer(model, dev, optimizer=torch.optim.SGD(model.parameters(), lr=1e-3), graph=True)
    # a callable model -> optimizer
    t = DataParallelTrainer(model, dev, optimizer=lambda m: ClipSGD(m.parameters(), lr=1e-3), graph=False)
    assert type(t.optimizer) is ClipSGD and len(t.optimizer.param_groups[0]['params']) == len(list(model.parameters()))
    # neither argument: today's ClipAdam
    t = DataParallelTrainer(model, dev)
    g = t.optimizer.param_groups[0]
    assert type(t.optimizer) is ClipAdam and (g['lr'], g['betas'], g['eps'], g['weight_decay']) == (1e-3, (0.5, 0.999), 1e-6, 0)
    assert t.scheduler is None and t.clip == 10.0


def test_steplr_attached_to_a_replaying_trainer_neither_warns_nor_miscounts(dev):
    from ptt_amd.train_step import DataParallelTrainer, synthetic_train_batch
    t = DataParallelTrainer(_model(dev), dev, graph=True, graph_warmup=3)
    batch = synthetic_train_batch(78, 2, dev)
    for _ in range(4):
        t.step(batch)
    assert t.graph_steps == 1
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        sched = torch.optim.lr_scheduler.StepLR(t.optimizer, step_size=2, gamma=0.5)
        lrs = []
        for _ in range(4):
            t.step(batch)
            sched.step()
            lrs.append(t.optimizer.param_groups[0]['lr'])
    torch.cuda.synchronize()
    assert not [w for w in caught if "optimizer.step()" in str(w.message)], [str(w.message) for w in caught]
    assert lrs == [1e-3, 5e-4, 5e-4, 2.5e-4] and sched.last_epoch == 4
    assert t.graph_steps == 5 and t.captured is not None
