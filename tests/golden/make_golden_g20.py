"""Fixture G20 — one training-mode forward + backward of MulTransformerBlock (multitransformer.py:11-76), run against the
reference tree (make_golden.REF) like make_golden_g19.py, in float32 AND in float64; only arrays and key names are committed.

For every (heads, layers) in tests/multitransformer_train_ref.BLOCKS: weights from multitransformer_ref.seeded_, inputs from
block_inputs(seed, 2, 64) with requires_grad on xyz and features (the box head feeds the block proposals that carry gradient), the
seeded linear loss of G19. Per block, with tag = "h{heads}_l{layers}" and p in ("32", "64"):
  loss{p}_{tag}        the loss (float64 scalar)
  res{p}_{tag}         res[..., ::4]
  names_{tag}          parameter names; "features" and "xyz" appended for the two input gradients
  norms{p}_{tag}       the gradient norm of every entry of names (accumulated in float64)
  g{p}_{tag}           the sampled gradients of every entry of names, concatenated: entry i contributes flat[::stride_i] with
                       stride_i = ceil(numel_i / MAX_SAMPLE) (tests/multitransformer_train_ref.sample)
  knn_{tag}            the reference's neighbour table square_distance(xyz, xyz).argsort()[:, :, :16] (int32)
Inputs are not stored: the tests regenerate them from the same seeds.

    python tests/golden/make_golden_g20.py        # writes tests/golden/G20_multitransformer_train.npz
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests.golden import make_golden as MG          # noqa: E402
from tests import multitransformer_ref as M         # noqa: E402
from tests import multitransformer_train_ref as T   # noqa: E402


def run(RefMTB, heads, layers, dtype):
    seed = T.train_seed(heads, layers)
    blk = M.seeded_(RefMTB(256, 512, 16, heads, layers), seed).to(dtype).train()
    xyz, f = M.block_inputs(seed, T.B, T.N)
    xyz = torch.from_numpy(xyz).to(dtype).requires_grad_(True)
    f = torch.from_numpy(f).to(dtype).requires_grad_(True)
    res, _ = blk(xyz, f)
    loss = (res * M.loss_weights(seed, tuple(res.shape)).to(dtype)).sum()
    loss.backward()
    names = [n for n, _ in blk.named_parameters()] + ["features", "xyz"]
    grads = [p.grad for p in blk.parameters()] + [f.grad, xyz.grad]
    return (names, np.float64(loss.item()), res.detach()[..., ::4].contiguous().numpy(),
            np.array([g.double().norm().item() for g in grads]), np.concatenate([T.sample(g.numpy()) for g in grads]),
            xyz.detach())


def main():
    MG._install_stubs()                             # thop, pointnet2_ops, easydict
    sys.path.insert(0, MG.REF)
    from ptt.models.transformer_block.multitransformer import MulTransformerBlock as RefMTB
    from ptt.models.model_utils import square_distance
    torch.manual_seed(0)
    out = {}
    for heads, layers in T.BLOCKS:
        tag = "h%d_l%d" % (heads, layers)
        for p, dtype in (("32", torch.float32), ("64", torch.float64)):
            names, loss, res, norms, g, xyz = run(RefMTB, heads, layers, dtype)
            out.update({"loss%s_%s" % (p, tag): loss, "res%s_%s" % (p, tag): res, "norms%s_%s" % (p, tag): norms,
                        "g%s_%s" % (p, tag): g})
            if p == "32":
                out["names_" + tag] = np.array(names)
                out["knn_" + tag] = square_distance(xyz, xyz).argsort()[:, :, :16].numpy().astype(np.int32)
    path = os.path.join(HERE, "G20_multitransformer_train.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
