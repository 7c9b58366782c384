"""MulTransformerBlock's training step on the CPU: train_ops.mul_block_usable is False there, and the stock path still equals the
float32 columns of fixture G20 (the reference's own run); the G20 recipe regenerates the committed file bit for bit where the
reference tree is present."""
import hashlib
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from ptt_amd import train_ops
from ptt_amd.models.transformer_block.multitransformer import MulTransformerBlock
from tests import multitransformer_ref as M
from tests import multitransformer_train_ref as T

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
G20 = os.path.join(GOLD, "G20_multitransformer_train.npz")


@pytest.fixture(scope="module")
def g20():
    return np.load(G20)


@pytest.mark.parametrize("heads,layers", T.BLOCKS)
def test_cpu_training_step_matches_g20(g20, heads, layers):
    tag = "h%d_l%d" % (heads, layers)
    seed = T.train_seed(heads, layers)
    blk = M.seeded_(MulTransformerBlock(256, 512, 16, heads, layers), seed).train()
    xyz, f = M.block_inputs(seed, T.B, T.N)
    xyz, f = torch.from_numpy(xyz).requires_grad_(True), torch.from_numpy(f).requires_grad_(True)
    assert not train_ops.mul_block_usable(blk, xyz, f)
    res, _ = blk(xyz, f)
    loss = (res * M.loss_weights(seed, tuple(res.shape))).sum()
    loss.backward()
    names = list(g20["names_" + tag])
    assert [n for n, _ in blk.named_parameters()] + ["features", "xyz"] == names
    grads = [p.grad for p in blk.parameters()] + [f.grad, xyz.grad]
    np.testing.assert_allclose(loss.item(), float(g20["loss32_" + tag]), rtol=1e-5)
    np.testing.assert_allclose(res.detach()[..., ::4].numpy(), g20["res32_" + tag], atol=1e-5, rtol=1e-5)
    norms = np.array([g.double().norm().item() for g in grads])
    # fc_gamma[2].bias cancels in the softmax: its gradient is rounding noise on either side, hence the atol
    np.testing.assert_allclose(norms, g20["norms32_" + tag], rtol=1e-4, atol=1e-4)
    ref = T.split(names, [tuple(g.shape) for g in grads], g20["g32_" + tag])
    for n, g in zip(names, grads):
        np.testing.assert_allclose(T.sample(g.numpy()), ref[n], atol=1e-5, rtol=1e-4, err_msg=n)


def test_g20_holds_both_precisions_and_the_neighbour_table(g20):
    for heads, layers in T.BLOCKS:
        tag = "h%d_l%d" % (heads, layers)
        assert g20["g32_" + tag].dtype == np.float32 and g20["g64_" + tag].dtype == np.float64
        assert g20["g32_" + tag].shape == g20["g64_" + tag].shape
        assert g20["knn_" + tag].shape == (T.B, T.N, 16) and len(g20["names_" + tag]) == 20 * layers + 2
    assert os.path.getsize(G20) < (1 << 20)


def test_g20_recipe_regenerates_the_committed_file(tmp_path):
    from tests.golden import make_golden as MG
    if not os.path.isdir(MG.REF):
        pytest.skip("the reference tree is not on this machine")
    before = hashlib.sha256(open(G20, "rb").read()).hexdigest()
    keep = str(tmp_path / "G20.npz")
    shutil.copy(G20, keep)
    try:
        subprocess.check_call([sys.executable, os.path.join(GOLD, "make_golden_g20.py")], stdout=subprocess.DEVNULL)
        after = hashlib.sha256(open(G20, "rb").read()).hexdigest()
    finally:
        shutil.copy(keep, G20)
    assert before == after
