"""The OPTIMIZATION block (ptt_amd/optimization.py, the optimizers of ptt_amd/optim.py) without a device: the schedules, the
builders and the parameter groups against fixture G25 (recorded from the reference's tools/train_utils/optimization by
tests/golden/make_golden_g25.py), twenty-step trajectories of the four OPTIMIZER values on the stock path the classes take on the
CPU, and the host-side refusals of ptt_optim_clip_step_f32 / ptt_optim_clip_step_dev_f32."""
import copy
import ctypes
import warnings

import numpy as np
import pytest
import torch

from ptt_amd.config import EasyDict
from tests import optimization_ref as S


@pytest.fixture(scope="module")
def g25():
    return np.load(S.GOLDEN)


# ------------------------------------------------------------------------------------------------------------------ schedules
class _Holder(object):
    """The least an optimizer is to OneCycle: parameter groups with lr and betas."""

    def __init__(self):
        self.param_groups = [dict(lr=0.0, betas=(0.9, 0.99)), dict(lr=0.0, betas=(0.9, 0.99))]


@pytest.mark.parametrize("total,pct", S.SCHEDULES)
def test_onecycle_equals_the_references_schedule(g25, total, pct):
    """The same closed form in float64: rtol 1e-14 is the margin of an expression evaluated in another order."""
    from ptt_amd.optimization import OneCycle
    h = _Holder()
    sched = OneCycle(h, total, S.LR_MAX, S.MOMS, S.DIV_FACTOR, pct)
    assert all(g['lr'] == S.LR_MAX / S.DIV_FACTOR and g['betas'] == (S.MOMS[0], 0.99) for g in h.param_groups)     # the step-0 values
    lrs, moms = [], []
    for it in range(total):
        sched.step(it)
        assert h.param_groups[0] == h.param_groups[1]
        lrs.append(h.param_groups[1]['lr'])
        moms.append(h.param_groups[1]['betas'][0])
    ref_lr, ref_mom = g25["sched_%d_%g_lr" % (total, pct)], g25["sched_%d_%g_mom" % (total, pct)]
    np.testing.assert_allclose(lrs, ref_lr, rtol=1e-14, atol=0)
    np.testing.assert_allclose(moms, ref_mom, rtol=1e-14, atol=0)
    # the phase boundary falls on the recorded step: the reference's lr peaks (= lr_max, momentum = moms[1]) exactly there
    peak = int(np.argmax(ref_lr))
    assert sched.boundary == peak == int(total * pct) and lrs[peak] == S.LR_MAX and moms[peak] == S.MOMS[1]
    assert int(np.argmax(lrs)) == peak


def test_onecycle_drives_momentum_of_sgd():
    from ptt_amd.optim import ClipSGD
    from ptt_amd.optimization import OneCycle
    opt = ClipSGD([torch.nn.Parameter(torch.zeros(3))], lr=0.1, momentum=0.9)
    sched = OneCycle(opt, 10, 1e-2, (0.95, 0.85), 10, 0.3)
    sched.step(3)
    assert opt.param_groups[0]['momentum'] == 0.85 and opt.param_groups[0]['lr'] == 1e-2


# ------------------------------------------------------------------------------------------------------------------- builders
def test_build_optimizer_classes_and_hyper_parameters():
    from ptt_amd.optim import ClipAdam, ClipAdamW, ClipSGD
    from ptt_amd.optimization import OneCycleAdamW, build_optimizer
    model = S.toy()
    n_all = len(list(model.parameters()))
    opt = build_optimizer(model, S.optim_cfg("adam", EasyDict))
    assert type(opt) is ClipAdam and isinstance(opt, torch.optim.Adam) and len(opt.param_groups) == 1
    g = opt.param_groups[0]
    assert (g['lr'], g['betas'], g['eps'], g['weight_decay'], len(g['params'])) == (0.01, (0.5, 0.999), 1e-6, 0.01, n_all)
    opt = build_optimizer(model, S.optim_cfg("adamw", EasyDict))
    assert type(opt) is ClipAdamW and isinstance(opt, torch.optim.AdamW)
    g = opt.param_groups[0]
    assert (g['lr'], g['betas'], g['eps'], g['weight_decay'], g['amsgrad'], len(g['params'])) == (0.01, (0.5, 0.999), 1e-6, 0.01, False, n_all)
    opt = build_optimizer(model, S.optim_cfg("sgd", EasyDict))
    assert type(opt) is ClipSGD and isinstance(opt, torch.optim.SGD)
    g = opt.param_groups[0]
    assert (g['lr'], g['momentum'], g['weight_decay'], g['dampening'], g['nesterov']) == (0.01, 0.9, 0.01, 0, False)
    opt = build_optimizer(model, S.optim_cfg("adam_onecycle", EasyDict))
    assert type(opt) is OneCycleAdamW and isinstance(opt, torch.optim.AdamW) and len(opt.param_groups) == 2
    for g in opt.param_groups:
        assert (g['lr'], g['betas'], g['weight_decay'], g['amsgrad']) == (3e-3, (0.9, 0.99), 0.01, False)
    for bad in ("rmsprop", "Adam", None):
        with pytest.raises(NotImplementedError):
            build_optimizer(model, EasyDict(dict(S.optim_cfg("adam", EasyDict), OPTIMIZER=bad)))


def _check_groups(g25, tag, model):
    from ptt_amd.optimization import build_optimizer
    opt = build_optimizer(model, S.optim_cfg("adam_onecycle", EasyDict))
    names = [n for n, _ in model.named_parameters()]
    assert names == [str(n) for n in g25["groups_%s_all" % tag]]
    index = S.group_indices(model, opt)
    assert len(index) == 2
    for g in range(2):
        assert index[g] == g25["groups_%s_index%d" % (tag, g)].tolist(), (tag, g)
        assert [names[i] for i in index[g]] == [str(n) for n in g25["groups_%s_names%d" % (tag, g)]]
    return index, names, opt


def test_adam_onecycle_groups_of_the_toy_model_are_the_references(g25):
    """Non-BatchNorm leaves, then BatchNorm leaves; the frozen bias and the parameter on the root (a module with children) are in
    neither group."""
    model = S.toy()
    index, names, _ = _check_groups(g25, "toy", model)
    held = {names[i] for grp in index for i in grp}
    assert "head.bias" not in held and "gain" not in held and "head.weight" in held
    assert [names[i] for i in index[1]] == ["bn1.weight", "bn1.bias", "block.2.weight", "block.2.bias"]


@pytest.mark.parametrize("tag", ["tracker", "tracker_mul"])
def test_adam_onecycle_groups_of_the_full_tracker_are_the_references(g25, tag):
    from ptt_amd.config import StubDataset, ptt_model_cfg
    from ptt_amd.models import build_network
    from tests import multitransformer_ref as M
    cfg = ptt_model_cfg()
    if tag == "tracker_mul":
        M.tracker_cfg(cfg)
    model = build_network(cfg, 1, StubDataset(training=True))
    index, _, _ = _check_groups(g25, tag, model)
    assert sorted(index[0] + index[1]) == list(range(len(list(model.parameters()))))      # every parameter of the shipped model


def test_lr_mom_wd_read_and_write_every_group():
    from ptt_amd.optimization import build_optimizer
    opt = build_optimizer(S.toy(), S.optim_cfg("adam_onecycle", EasyDict))
    assert (float(opt.lr), opt.mom, opt.wd) == (3e-3, 0.9, 0.01)
    opt.lr, opt.mom, opt.wd = 5e-4, 0.87, 0.02
    for g in opt.param_groups:
        assert (g['lr'], g['betas'], g['weight_decay']) == (5e-4, (0.87, 0.99), 0.02)
    assert (opt.lr, opt.mom, opt.wd) == (5e-4, 0.87, 0.02)


def test_build_scheduler():
    from ptt_amd.optimization import OneCycle, build_optimizer, build_scheduler
    cfg = S.optim_cfg("adam_onecycle", EasyDict)
    opt = build_optimizer(S.toy(), cfg)
    sched, warm = build_scheduler(opt, 5, 4, -1, cfg)
    assert type(sched) is OneCycle and warm is None and sched.total_step == 20 and sched.boundary == 8
    assert (sched.lr_max, sched.moms, sched.div_factor) == (S.LR_MAX, S.MOMS, S.DIV_FACTOR) and opt.lr == S.LR_MAX / S.DIV_FACTOR
    cfg = S.optim_cfg("adam", EasyDict)
    opt = build_optimizer(S.toy(), cfg)
    sched, warm = build_scheduler(opt, 5, 4, -1, cfg)
    assert type(sched) is torch.optim.lr_scheduler.StepLR and warm is None and (sched.step_size, sched.gamma) == (12, 0.2)
    with pytest.raises(NotImplementedError):
        build_scheduler(opt, 5, 4, -1, EasyDict(dict(cfg, SCHEDULER='cosine')))


# --------------------------------------------------------------------------------------------------------------- trajectories
@pytest.mark.parametrize("name", S.OPTIMIZERS)
def test_twenty_steps_reproduce_the_references_trajectory(g25, name):
    """On the CPU the classes take the stock path (clip_grad_norm_ + the stock step). Parameters after steps 1, 2, 10 and 20 and the
    final state against G25 (c): the bar of tests/test_step_ops_gpu.py for ClipAdam against torch."""
    from ptt_amd.optimization import build_optimizer, build_scheduler
    cfg = S.optim_cfg(name, EasyDict)
    model = S.toy()
    opt = build_optimizer(model, cfg)
    sched = build_scheduler(opt, S.STEPS, 1, -1, cfg)[0] if name == "adam_onecycle" else None
    norms = []

    def clip_and_step():
        opt.step(max_norm=cfg.GRAD_NORM_CLIP)
        norms.append(float(opt.last_norm))
    got = S.run_trajectory(model, opt, sched, clip_and_step)
    sizes = S.param_sizes(model)
    for k in S.RECORD:
        excess, worst = S.params_excess(got[k], g25["traj_%s_p%d" % (name, k)], sizes)
        assert excess <= 0, (name, k, worst)
    np.testing.assert_allclose(norms, g25["traj_%s_norms" % name], rtol=2e-6)
    for key, v in S.flat_state(model, opt, name).items():
        ref = g25["traj_%s_state_%s" % (name, key)]
        if key == "step":
            assert np.array_equal(v, ref)
        else:
            excess, worst = S.moments_excess(v, ref, S.state_sizes(model, opt))
            assert excess <= 0, (name, key, worst)
    if name == "adam_onecycle":
        assert torch.equal(dict(model.named_parameters())["gain"], dict(S.toy().named_parameters())["gain"])      # held by no group


@pytest.mark.parametrize("name", ["adamw", "sgd"])
def test_state_dicts_interchange_with_the_stock_classes(name):
    from ptt_amd.optim import ClipAdamW, ClipSGD
    mine_cls, stock_cls, kw = ((ClipAdamW, torch.optim.AdamW, dict(lr=0.01, weight_decay=0.01)) if name == "adamw" else
                               (ClipSGD, torch.optim.SGD, dict(lr=0.01, momentum=0.9, weight_decay=0.01)))
    models = [S.toy(), S.toy()]
    mine, stock = mine_cls(models[0].parameters(), **kw), stock_cls(models[1].parameters(), **kw)
    for step in range(2):
        for m in models:
            S.assign_grads(m, step)
        mine.step(max_norm=S.CLIP)
        torch.nn.utils.clip_grad_norm_(models[1].parameters(), S.CLIP)
        stock.step()
    assert np.array_equal(S.flat_params(models[0]), S.flat_params(models[1]))
    assert set(mine.state_dict()['state'][0]) == set(stock.state_dict()['state'][0])
    fresh = [stock_cls(S.toy().parameters(), **kw), mine_cls(S.toy().parameters(), **kw)]
    # deep copies, as a checkpoint file gives: torch's load_state_dict keeps the 'step' tensors it is handed
    fresh[0].load_state_dict(copy.deepcopy(mine.state_dict()))
    fresh[1].load_state_dict(copy.deepcopy(stock.state_dict()))
    key = 'exp_avg' if name == "adamw" else 'momentum_buffer'
    for opt, src in zip(fresh, (mine, stock)):
        for a, b in zip(opt.state_dict()['state'].values(), src.state_dict()['state'].values()):
            assert torch.equal(a[key], b[key])
    # and the reloaded optimizer goes on exactly as the one it was loaded from
    m3 = S.toy()
    with torch.no_grad():
        for p, q in zip(m3.parameters(), models[0].parameters()):
            p.copy_(q)
    again = mine_cls(m3.parameters(), **kw)
    again.load_state_dict(copy.deepcopy(stock.state_dict()))
    for m in (m3, models[1]):
        S.assign_grads(m, 2)
    again.step(max_norm=None)
    stock.step()
    assert np.array_equal(S.flat_params(m3), S.flat_params(models[1]))


# ------------------------------------------------------------------------------------------------------------ host refusals
def test_abi_declares_and_exports_the_generalised_step():
    from ptt_amd import _lib
    assert _lib.ABI_VERSION >= 33
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("ptt_optim_clip_step_f32", "ptt_optim_clip_step_dev_f32"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
        restype, argtypes = _lib.PROTOTYPES[name]
        assert restype is ctypes.c_int and len(argtypes) == 14 and argtypes[8] is ctypes.c_float
    for name in ("ptt_adam_clip_step_f32", "ptt_adam_clip_step_dev_f32"):                   # the Adam pair keeps its signatures
        assert len(_lib.PROTOTYPES[name][1]) == (9 if name.endswith("step_f32") else 10)


def test_new_structures_match_the_c_header(tmp_path):
    """sizeof / offsetof from gcc against ctypes, as tests/test_oracle_cpu.py does for the structures it lists."""
    import os
    import subprocess
    from ptt_amd import _lib
    pairs = [("ptt_optim_tensor", _lib.OptimTensor), ("ptt_optim_hyper", _lib.OptimHyper)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ptt_hip.h"', 'int main(void) {']
    for cname, st in pairs:
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, *_ in st._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines += ['return 0;', '}']
    src = tmp_path / "abi_probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "abi_probe"
    subprocess.check_call(["gcc", "-I", os.path.dirname(_lib.HEADER_PATH), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    for cname, st in pairs:
        assert int(got[cname]) == ctypes.sizeof(st), (cname, got[cname], ctypes.sizeof(st))
        for fname, *_ in st._fields_:
            assert int(got["%s.%s" % (cname, fname)]) == getattr(st, fname).offset, (cname, fname)


@pytest.mark.parametrize("entry", ["ptt_optim_clip_step_f32", "ptt_optim_clip_step_dev_f32"])
def test_refusals_come_before_any_runtime_call(entry):
    """PTT_EINVAL / PTT_EUNSUPPORTED / PTT_EWORKSPACE with a null stream and host addresses that are never dereferenced as device
    memory: every check precedes the first launch, so this needs no device."""
    from ptt_amd import _lib
    from ptt_amd.ops import OptimTable
    lib = ctypes.CDLL(_lib.LIB_PATH)
    fn = getattr(lib, entry)
    fn.restype, fn.argtypes = _lib.PROTOTYPES[entry]
    lib.ptt_last_error_string.restype = ctypes.c_char_p
    einval, eunsup, ework = -1, -2, -4                      # PTT_EINVAL, PTT_EUNSUPPORTED, PTT_EWORKSPACE (an enum of the header)
    host_hyper = entry == "ptt_optim_clip_step_f32"
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    rows = (_lib.OptimTensor * 2)()
    for r, g in zip(rows, (0, 1)):
        r.param, r.grad, r.state1, r.state2, r.n, r.group = p.value, p.value, p.value, p.value, 8, g
    adamw = OptimTable.hyper("adamw", 1e-3, 1, (0.9, 0.99), 1e-8, 0.01)
    sgd = OptimTable.hyper("sgd", 1e-2, momentum=0.9)
    hyp = lambda *h: (_lib.OptimHyper * len(h))(*h)

    def call(table=p, rows=rows, n_rows=2, which=p, first=p, n_chunks=2, hyper=hyp(adamw, sgd), n_groups=2, max_norm=10.0, partial=p, partial_elems=2):
        return fn(table, rows, n_rows, which, first, n_chunks, hyper, n_groups, max_norm, 1, partial, partial_elems, None, None)
    assert call(table=None) == einval and call(which=None) == einval and call(first=None) == einval      # null table
    assert call(hyper=None) == einval
    assert call(n_groups=0) == einval and call(n_groups=-1) == einval
    assert call(n_groups=_lib.PTT_OPTIM_MAX_GROUPS + 1) == eunsup
    assert call(n_chunks=-1) == einval
    assert call(n_groups=1) == einval and b"group 1 of 1" in lib.ptt_last_error_string()               # a row of group 1, one group
    rows[0].group = -1
    assert call() == einval
    rows[0].group = 0
    rows[1].grad = None
    assert call() == einval
    rows[1].grad = p.value
    assert call(partial=None) == ework and call(partial_elems=1) == ework                              # clipping: n_chunks doubles
    if host_hyper:
        bad = OptimTable.hyper("adamw", 1e-3, 1, (0.9, 0.99), 1e-8, 0.01)
        bad.kind = 7
        assert call(hyper=hyp(adamw, bad)) == einval and b"unknown kind 7" in lib.ptt_last_error_string()
        rows[1].state1 = None
        assert call() == einval                                                                        # SGD, momentum 0.9, no buffer
        rows[1].state1 = p.value
        rows[0].state2 = None
        assert call() == einval                                                                        # AdamW without exp_avg_sq
        rows[0].state2 = p.value
        nobias = OptimTable.hyper("adamw", 1e-3, 1, (0.9, 0.99), 1e-8, 0.01)
        nobias.bias2_sqrt = 0.0
        assert call(hyper=hyp(nobias, sgd)) == einval
    # what is allowed: an empty table launches nothing; SGD without momentum needs no buffer (seen only in the checks: the call
    # below is refused for its workspace AFTER the rows passed)
    assert call(n_chunks=0, table=None, which=None, first=None) == 0
    rows[1].state1 = None
    assert call(hyper=hyp(adamw, OptimTable.hyper("sgd", 1e-2)), partial_elems=1) == ework


def test_cpu_parameters_take_the_stock_path_and_need_no_library_call():
    from ptt_amd.optim import ClipAdamW
    p = torch.nn.Parameter(torch.ones(4))
    opt = ClipAdamW([p], lr=0.1, weight_decay=0.0)
    p.grad = torch.full((4,), 3.0)
    opt.step(max_norm=1.0)
    assert abs(float(opt.last_norm) - 6.0) < 1e-6 and opt._table is None
    assert torch.allclose(p.grad, torch.full((4,), 0.5), atol=1e-6)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
        p.grad = torch.full((4,), 3.0)
        opt.step(max_norm=1.0)
        sched.step()
    assert opt.param_groups[0]['lr'] == 0.05
