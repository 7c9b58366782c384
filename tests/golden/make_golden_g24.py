"""Fixture G24 — MulTransformerBlock (multitransformer.py:11-76) at DIM_MODEL / KNN other than the shipped (512, 16), run against
the reference checkout (make_golden.REF) in the build container like make_golden.py; only arrays and key names are committed.

  blocks  the reference's MulTransformerBlock(256, D, k, heads, layers) at tests/mul_shapes_ref.G24_CASES = (256, 8, heads 4,
          layers 2), (128, 32, heads 2, layers 1), (256, 16, heads 8, layers 1), eval mode, on one 2 x 64-point synth.frames batch
          of distinct points: res[..., ::4] and a sample (points ::16, channels ::8) of the last layer's attn (B*heads, N, k, hd);
          weights from multitransformer_ref.seeded_ (LayerNorm affine included)
  keys    for every new (D, heads) (tests/mul_shapes_ref.D_HEADS): the state_dict key list and shapes of the block the reference's
          build_transformer returns for NAME MulTransformerBlock, DIM_INPUT 256, DIM_MODEL D, N_HEADS heads, N_LAYERS 2 (k holds no
          parameter)
Inputs are not stored: the tests regenerate them from the same seeds (tests/mul_shapes_ref.py).

    python tests/golden/make_golden_g24.py        # writes tests/golden/g24_multransformer_shapes.npz
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests.golden import make_golden as MG          # noqa: E402
from tests import mul_shapes_ref as S               # noqa: E402

KEYS_LAYERS, KEYS_K = 2, 16


def main():
    EasyDict = MG._install_stubs()                  # thop, pointnet2_ops, easydict
    sys.path.insert(0, MG.REF)
    from ptt.models.transformer_block import build_transformer as ref_build
    from ptt.models.transformer_block.multitransformer import MulTransformerBlock as RefMul
    torch.manual_seed(0)
    out = {}
    for D, k, heads, layers in S.G24_CASES:
        blk = S.g24_seeded_(RefMul(S.D_POINTS, D, k, heads, layers), D, k, heads, layers).eval()
        xyz, f = S.g24_inputs(D, k, heads, layers)
        with torch.no_grad():
            res, attn = blk(torch.from_numpy(xyz), torch.from_numpy(f))
        assert tuple(attn.shape) == (S.G24_B * heads, S.G24_N, k, D // heads)
        tag = S.g24_tag(D, k, heads, layers)
        out["res_" + tag] = res[..., ::4].contiguous().numpy()
        out["attn_" + tag] = attn[:, ::16, :, ::8].contiguous().numpy()
    for D, heads in S.D_HEADS:
        cfg = EasyDict(NAME="MulTransformerBlock", DIM_INPUT=S.D_POINTS, DIM_MODEL=D, KNN=KEYS_K, N_HEADS=heads, N_LAYERS=KEYS_LAYERS)
        sd = ref_build(cfg).state_dict()
        out["keys_d%d_h%d" % (D, heads)] = np.array(list(sd.keys()))
        out["shapes_d%d_h%d" % (D, heads)] = np.array([str(tuple(v.shape)) for v in sd.values()])
    path = os.path.join(HERE, "g24_multransformer_shapes.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
