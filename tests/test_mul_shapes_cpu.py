"""MulTransformerBlock at DIM_MODEL 128 / 256 x KNN 8 / 16 / 32: what can be checked without a GPU — the stock path equals the
reference's own block (fixture G24), the module the config builds carries the reference's parameters for every new (D, heads), the
training gate is closed on the CPU, the C ABI is the one that has the shapes, the Python gates name the envelope, and the cases
tests/test_mul_shapes_gpu.py runs are well-posed."""
import os

import numpy as np
import pytest
import torch

from ptt_amd import _lib, ops, train_ops
from ptt_amd.hot_path import AttrDict
from ptt_amd.models.transformer_block import build_transformer
from ptt_amd.models.transformer_block.multitransformer import FUSED_HEADS, MulTransformerBlock
from tests import fused_ref as FR
from tests import mul_shapes_ref as S
from tests import pair_shapes_ref as PS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g24():
    return np.load(os.path.join(ROOT, "tests", "golden", "g24_multransformer_shapes.npz"))


@pytest.mark.parametrize("D,k,heads,layers", S.G24_CASES)
def test_stock_path_equals_g24(g24, D, k, heads, layers):
    blk = S.g24_seeded_(MulTransformerBlock(S.D_POINTS, D, k, heads, layers), D, k, heads, layers).eval()
    xyz, f = S.g24_inputs(D, k, heads, layers)
    with torch.no_grad():
        res, attn = blk(torch.from_numpy(xyz), torch.from_numpy(f))
    tag = S.g24_tag(D, k, heads, layers)
    assert tuple(attn.shape) == (S.G24_B * heads, S.G24_N, k, D // heads)
    np.testing.assert_allclose(res[..., ::4].numpy(), g24["res_" + tag], **FR.TOL)
    np.testing.assert_allclose(attn[:, ::16, :, ::8].numpy(), g24["attn_" + tag], **FR.TOL)


@pytest.mark.parametrize("D,heads", S.D_HEADS)
def test_build_transformer_has_the_references_parameters(g24, D, heads):
    blk = build_transformer(AttrDict(NAME='MulTransformerBlock', DIM_INPUT=S.D_POINTS, DIM_MODEL=D, KNN=16, N_HEADS=heads, N_LAYERS=2))
    assert isinstance(blk, MulTransformerBlock) and (blk.d_model, blk.heads, blk.d_points, len(blk.layers)) == (D, heads, S.D_POINTS, 2)
    sd = blk.state_dict()
    assert list(sd.keys()) == list(g24["keys_d%d_h%d" % (D, heads)])
    assert [str(tuple(v.shape)) for v in sd.values()] == list(g24["shapes_d%d_h%d" % (D, heads)])


@pytest.mark.parametrize("D,k,heads,layers", S.TRAIN_CASES)
def test_mul_block_usable_is_false_on_the_cpu(D, k, heads, layers):
    blk = MulTransformerBlock(S.D_POINTS, D, k, heads, layers).train()
    xyz, f = S.module_inputs(D, k, heads, S.TRAIN_B, S.TRAIN_N)
    assert not train_ops.mul_block_usable(blk, torch.from_numpy(xyz), torch.from_numpy(f))
    assert not blk._fusable(torch.from_numpy(xyz), torch.from_numpy(f))


def test_abi_version():
    assert _lib.ABI_VERSION >= 32


def test_the_envelope():
    """d_model 128 / 256 x k 8 / 16 / 32 x heads with hd >= 32; at 512 nothing but k 16; FUSED_HEADS still exported."""
    assert FUSED_HEADS == (1, 2, 4, 8)
    ok = {(D, k, H) for D in (64, 128, 256, 384, 512) for k in (4, 8, 16, 32) for H in (1, 2, 3, 4, 8, 16) if ops.mul_block_supported(D, k, H)}
    assert ok == {(D, k, H) for D, H in S.D_HEADS for k in S.KNNS} | {(512, 16, H) for H in FUSED_HEADS}
    assert len(S.KERNEL_SHAPES) == 15 and len(S.KERNEL_CASES) == 45
    assert all(ops.pair_heads_supported(D, k, H) for D, H, k in S.KERNEL_SHAPES)
    # the single-head kernel's shapes stay open to ops.pt_attn_pair (TransformerBlock), the multi-head form is closed at (512, 8)
    assert ops.pair_heads_supported(512, 8, 1) and not ops.pair_heads_supported(512, 8, 2) and not ops.pair_heads_supported(128, 16, 8)
    for B, N, k, D, H in S.REFUSED.values():
        assert not ops.pair_heads_supported(D, k, H) or N % (32 // k) != 0


def _clouds():
    out = [(k, S.g24_inputs(D, k, H, L)[0]) for D, k, H, L in S.G24_CASES]
    out += [(k, S.module_inputs(D, k, H, B)[0]) for D, k, H, L in S.MODULE_CASES for B in S.MODULE_BATCHES]
    out += [(k, S.module_inputs(D, k, H, S.TRAIN_B, S.TRAIN_N)[0]) for D, k, H, L in S.TRAIN_CASES]
    return out


def test_cases_are_well_posed():
    """As tests/test_pair_shapes_cpu.py::test_cases_are_well_posed holds the kernel-level clouds (shared with this file's cases): the
    tile rule, distinct points, and a k-th-neighbour gap a float32 distance cannot blur (bar 2e-6 relative, four times the 4.8e-7 two
    float32 squared distances can close) — so the stock path's argsort, the float32 oracle and the device kNN pick the same sets."""
    for k, s in _clouds():
        B, N, _ = s.shape
        assert N % (32 // k) == 0 and N >= k and s.dtype == np.float32
        assert float(PS.kth_gaps(s, k).min()) > 2e-6
        x = s.astype(np.float64)
        assert float((((x[:, :, None] - x[:, None]) ** 2).sum(-1) + np.eye(N)[None]).min()) > 0.0
