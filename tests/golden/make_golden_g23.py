"""Fixture G23 — TransformerBlock (variants.py:127-165) at DIM_MODEL / KNN other than the shipped (512, 16), run against
/root/reference in the build container like make_golden.py; only arrays and key names are committed.

  blocks  the reference's TransformerBlock(256, D, k) at (D, k) in tests/pair_shapes_ref.G23_PAIRS = (256, 8), (128, 32), (512, 32),
          eval mode, on one 2 x 64-point synth.frames batch of distinct points: res[..., ::4] and a sample (points ::16,
          channels ::8) of attn (B, N, k, D); weights from fill_state_dict_
  keys    for each of the eight new (D, k) pairs (tests/pair_shapes_ref.PAIRS): the state_dict key list and shapes of the block the
          reference's build_transformer returns for DIM_INPUT 256, DIM_MODEL D, KNN k
Inputs are not stored: the tests regenerate them from the same seeds (tests/pair_shapes_ref.py).

    python tests/golden/make_golden_g23.py        # writes tests/golden/g23_transformer_shapes.npz
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests.golden import make_golden as MG          # noqa: E402
from tests import pair_shapes_ref as S              # noqa: E402


def main():
    EasyDict = MG._install_stubs()                  # thop, pointnet2_ops, easydict
    sys.path.insert(0, MG.REF)
    from ptt.models.transformer_block import build_transformer as ref_build
    from ptt.models.transformer_block.variants import TransformerBlock as RefTB
    torch.manual_seed(0)
    out = {}
    for D, k in S.G23_PAIRS:
        blk = S.g23_seeded_(RefTB(S.D_POINTS, D, k), D, k).eval()
        xyz, f = S.g23_inputs(D, k)
        with torch.no_grad():
            res, attn = blk(torch.from_numpy(xyz), torch.from_numpy(f))
        assert tuple(attn.shape) == (S.G23_B, S.G23_N, k, D)
        tag = "d%d_k%d" % (D, k)
        out["res_" + tag] = res[..., ::4].contiguous().numpy()
        out["attn_" + tag] = attn[:, ::16, :, ::8].contiguous().numpy()
    for D, k in S.PAIRS:
        cfg = EasyDict(NAME="TransformerBlock", DIM_INPUT=S.D_POINTS, DIM_MODEL=D, KNN=k, N_HEADS=1, N_LAYERS=1)
        sd = ref_build(cfg).state_dict()
        out["keys_d%d_k%d" % (D, k)] = np.array(list(sd.keys()))
        out["shapes_d%d_k%d" % (D, k)] = np.array([str(tuple(v.shape)) for v in sd.values()])
    path = os.path.join(HERE, "g23_transformer_shapes.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
