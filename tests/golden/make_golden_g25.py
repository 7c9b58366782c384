"""Fixture G25 — the OPTIMIZATION block: the reference's build_optimizer / build_scheduler / OneCycle
(tools/train_utils/optimization) run on the CPU against the reference checkout (make_golden.REF), like make_golden.py; only
arrays and name lists are committed. `fastai_optim.py` imports collections.Iterable, which this Python keeps in collections.abc:
the alias is set before the import.

  (a) sched_<T>_<pct>_lr / _mom   the lr and momentum the reference's OneCycle sets at it = 0 .. T - 1, for optimization_ref.SCHEDULES
                                  with moms (0.95, 0.85), div_factor 10, lr_max 3e-3 (float64)
  (b) groups_<model>_names<g> / _index<g>   the parameter names of the two groups of the `adam_onecycle` optimizer, in order, and
                                  their positions in named_parameters() order, for the toy model (optimization_ref.Toy), the full
                                  tracker of ptt.yaml ("tracker") and the one with MulTransformerBlock (4 heads, 2 layers) in both
                                  heads ("tracker_mul"); groups_<model>_all = every named parameter
  (c) traj_<optimizer>_p<k>       the toy model's parameters (flat, named_parameters() order) after steps k = 1, 2, 10, 20 of
                                  [OneCycle.step(it);] assigned seeded gradients; clip_grad_norm_(model.parameters(), 10);
                                  optimizer.step() for each of the four OPTIMIZER values, and traj_<optimizer>_state_<key> = the
                                  final optimizer state (optimization_ref.flat_state)

    python tests/golden/make_golden_g25.py        # writes tests/golden/g25_optimization.npz
"""
import collections
import collections.abc
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests.golden import make_golden as MG          # noqa: E402
from tests import multitransformer_ref as M         # noqa: E402
from tests import optimization_ref as S             # noqa: E402


def _groups(out, tag, model, optimizer):
    names = [n for n, _ in model.named_parameters()]
    index = S.group_indices(model, optimizer)
    assert len(index) == 2
    out["groups_%s_all" % tag] = np.array(names)
    for g, idx in enumerate(index):
        out["groups_%s_index%d" % (tag, g)] = np.array(idx, dtype=np.int64)
        out["groups_%s_names%d" % (tag, g)] = np.array([names[i] for i in idx])
    return index


def main():
    EasyDict = MG._install_stubs()
    collections.Iterable = collections.abc.Iterable
    sys.path.insert(0, os.path.join(MG.REF, "tools"))
    sys.path.insert(0, MG.REF)
    from train_utils.optimization import build_optimizer, build_scheduler
    from train_utils.optimization.learning_schedules_fastai import OneCycle
    out = {}

    # (a) schedules
    class Holder(object):
        lr, mom = 0.0, 0.0
    for total, pct in S.SCHEDULES:
        h = Holder()
        sched = OneCycle(h, total, S.LR_MAX, list(S.MOMS), S.DIV_FACTOR, pct)
        lrs, moms = [], []
        for it in range(total):
            sched.step(it)
            lrs.append(float(h.lr))
            moms.append(float(h.mom))
        out["sched_%d_%g_lr" % (total, pct)] = np.array(lrs, dtype=np.float64)
        out["sched_%d_%g_mom" % (total, pct)] = np.array(moms, dtype=np.float64)

    # (b) groups
    cfg1 = S.optim_cfg("adam_onecycle", EasyDict)
    model = S.toy()
    _groups(out, "toy", model, build_optimizer(model, cfg1))
    from ptt.config import cfg_from_yaml_file as ref_cfg_from_yaml
    from ptt.models import build_network as ref_build_network
    from ptt_amd.config import StubDataset
    for tag, edit in (("tracker", lambda c: c), ("tracker_mul", M.tracker_cfg)):
        rcfg = ref_cfg_from_yaml(os.path.join(MG.REF, "tools/cfgs/kitti_models/ptt.yaml"), EasyDict())
        edit(rcfg.MODEL)
        net = ref_build_network(rcfg.MODEL, 1, StubDataset(training=True))
        index = _groups(out, tag, net, build_optimizer(net, cfg1))
        n_all = sum(1 for p in net.parameters() if p.requires_grad)
        print(tag, "groups of", [len(i) for i in index], "parameters;", n_all, "trainable in the model")

    # (c) trajectories
    for name in S.OPTIMIZERS:
        cfg = S.optim_cfg(name, EasyDict)
        model = S.toy()
        opt = build_optimizer(model, cfg)
        sched = build_scheduler(opt, S.STEPS, 1, -1, cfg)[0] if name == "adam_onecycle" else None

        def clip_and_step():
            norm = torch.nn.utils.clip_grad_norm_(model.parameters(), cfg.GRAD_NORM_CLIP)
            norms.append(float(norm))
            opt.step()
        norms = []
        for k, flat in S.run_trajectory(model, opt, sched, clip_and_step).items():
            out["traj_%s_p%d" % (name, k)] = flat
        inner = opt.opt if name == "adam_onecycle" else opt
        for key, v in S.flat_state(model, inner, name).items():
            out["traj_%s_state_%s" % (name, key)] = v
        out["traj_%s_norms" % name] = np.array(norms, dtype=np.float64)
        print(name, "norms %.2f .. %.2f, clipped on %d of %d steps" % (min(norms), max(norms), sum(n > S.CLIP for n in norms), len(norms)))
        assert 0 < sum(n > S.CLIP for n in norms) < len(norms)
    path = S.GOLDEN
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
