"""TransformerBlock at DIM_MODEL 128 / 256 / 512 x KNN 8 / 16 / 32: what can be checked without a GPU — the module the
config builds carries the reference's parameters for every new pair (fixture G23), the C ABI is the one that has the shapes, and
the oracle cases tests/test_pair_shapes_gpu.py runs are well-posed."""
import os
import re

import numpy as np
import pytest

from ptt_amd import _lib
from ptt_amd.hot_path import AttrDict
from ptt_amd.models.transformer_block import build_transformer
from ptt_amd.models.transformer_block.variants import TransformerBlock
from tests import pair_shapes_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g23():
    return np.load(os.path.join(ROOT, "tests", "golden", "g23_transformer_shapes.npz"))


@pytest.mark.parametrize("D,k", S.PAIRS)
def test_build_transformer_has_the_references_parameters(g23, D, k):
    blk = build_transformer(AttrDict(NAME='TransformerBlock', DIM_INPUT=S.D_POINTS, DIM_MODEL=D, KNN=k, N_HEADS=1, N_LAYERS=1))
    assert isinstance(blk, TransformerBlock) and (blk.d_model, blk.k, blk.d_points) == (D, k, S.D_POINTS)
    sd = blk.state_dict()
    assert list(sd.keys()) == list(g23["keys_d%d_k%d" % (D, k)])
    assert [str(tuple(v.shape)) for v in sd.values()] == list(g23["shapes_d%d_k%d" % (D, k)])


def test_abi_version():
    with open(os.path.join(ROOT, "include", "ptt_hip.h")) as fh:
        m = re.search(r"^#define\s+PTT_ABI_VERSION\s+(\d+)", fh.read(), flags=re.M)
    assert m and int(m.group(1)) >= 31
    assert _lib.ABI_VERSION == int(m.group(1))


def test_the_eight_new_pairs():
    assert len(S.PAIRS) == 8 and (512, 16) not in S.PAIRS
    assert sorted(set(S.PAIRS) | {(512, 16)}) == [(D, k) for D in (128, 256, 512) for k in (8, 16, 32)]
    assert S.CLOUDS == {8: [(1, 8), (3, 12), (1, 52)], 16: [(1, 16), (3, 18), (1, 50)], 32: [(1, 32), (3, 33), (1, 70)]}
    assert len(S.CASES) == 24


@pytest.mark.parametrize("k,B,N", [(k, B, N) for k in sorted(S.CLOUDS) for B, N in S.CLOUDS[k]] +
                         [(k, S.G23_B, S.G23_N) for _, k in S.G23_PAIRS] +
                         [(k, B, S.MODULE_N) for k in sorted(S.CLOUDS) for B in S.MODULE_BATCHES + (S.TRAIN_B,)])
def test_cases_are_well_posed(k, B, N):
    """The tile rule N % (32 // k) == 0, N >= k, and no tie at the k-th neighbour: in float64 the k-th and (k+1)-th smallest
    squared distances of every point differ by more than float32 can blur. A float32 squared distance (three rounded differences,
    squared and summed) lies within about 4u = 2.4e-7 relative of the exact one, so two of them can close a relative gap of 4.8e-7 at
    most; the bar is 2e-6, four times that. Then the float32 oracle, the device kernel and a float64 argsort pick the same neighbour
    SET. (N = k: every point is a neighbour.)"""
    assert N % (32 // k) == 0 and N >= k
    if (B, N) == (S.G23_B, S.G23_N):
        clouds = [S.g23_inputs(D, kk)[0] for D, kk in S.G23_PAIRS if kk == k]
    elif N == S.MODULE_N:
        clouds = [S.module_inputs(D, kk, B)[0] for D, kk in S.PAIRS if kk == k]
    else:
        clouds = [S.cloud(k, B, N)]
    for s in clouds:
        assert s.shape == (B, N, 3) and s.dtype == np.float32
        if N > k:
            gap = S.kth_gaps(s, k)
            assert float(gap.min()) > 2e-6, float(gap.min())
        # and no two points coincide (a zero distance beside the point's own)
        x = s.astype(np.float64)
        d = ((x[:, :, None] - x[:, None]) ** 2).sum(-1) + np.eye(N)[None]
        assert float(d.min()) > 0.0
