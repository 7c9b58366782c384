"""The split-bf16 pair kernel's arithmetic, config key and bindings, without a GPU (tests/pair_split_ref.py).

  * split2 is round-to-nearest-even and hi + lo reproduces a float32 to 2^-16 relative;
  * the emulated block (the three in-kernel GEMMs in two-piece arithmetic, float64 elsewhere) on fixture G5 meets the existing
    TOL (1e-4) for res and the attn sample at N = 128 and 64 — measured max |res - fixture| 2.0e-6 / 2.1e-6, attn 1.6e-8;
  * the PRECISION key of build_transformer, TransformerBlock.precision's validation, set_precision's count and version bump;
  * ABI 37 with the new prototypes and the descriptor bound as the header declares them.
"""
import os
import re
import warnings

import numpy as np
import pytest
import torch

from oracle import index_ops as O
from ptt_amd import _lib, ops
from ptt_amd.hot_path import AttrDict
from ptt_amd.models.transformer_block import build_transformer
from ptt_amd.models.transformer_block.variants import TransformerBlock
from ptt_amd.precision import set_precision
from tests import fused_ref as FR
from tests import pair_split_ref as PS
from tests.util import transformer_params

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------- the split
def test_split2_is_round_to_nearest_even():
    # ties: 1 + 2^-8 lies half-way between the bf16 neighbours 1 and 1 + 2^-7 -> the even one (1); 1 + 3 * 2^-8 -> 1 + 2^-6
    x = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 1.0 + 2.0 ** -8 + 2.0 ** -20, 3.0e-5, 0.0], dtype=torch.float32)
    hi, lo = PS.split2(x)
    assert hi.dtype == torch.float64 and lo.dtype == torch.float64
    assert hi.tolist()[:4] == [1.0, 1.0 + 2.0 ** -6, -1.0, 1.0 + 2.0 ** -7]
    # and on random values, bit for bit the integer formula of the pack restatement
    r = torch.from_numpy(np.random.RandomState(0).standard_normal(4096).astype(np.float32) * 3.0)
    hi, lo = PS.split2(r)
    bits = lambda t: (t.float().contiguous().view(torch.int32) >> 16) & 0xffff
    assert np.array_equal(bits(hi).numpy().astype(np.uint16), PS.bf16_rne_np(r.numpy()))
    assert np.array_equal(bits(lo).numpy().astype(np.uint16), PS.bf16_rne_np(r.numpy() - hi.float().numpy()))


def test_two_pieces_reproduce_a_float32():
    rs = np.random.RandomState(1)
    x = torch.from_numpy((rs.standard_normal(1 << 16) * np.exp(rs.uniform(-20, 20, 1 << 16))).astype(np.float32))
    hi, lo = PS.split2(x)
    err = ((hi + lo) - x.double()).abs() / x.double().abs()
    print("worst |hi + lo - x| / |x| = %.3e (2^-16 = %.3e)" % (float(err.max()), 2.0 ** -16))
    assert float(err.max()) <= 2.0 ** -16
    # the residual x - hi is exact in float32 (what both the kernel and the pack rely on)
    assert torch.equal((x - hi.float()).double(), x.double() - hi)


def test_split_pack_order():
    """The restated order on a weight whose values name their own position."""
    Cout, K = 64, 32
    w = (np.arange(Cout)[:, None] * 256 + np.arange(K)[None, :]).astype(np.float32)          # up to 14 bits: hi and lo both non-zero
    p = PS.split_pack_np(w)
    assert p.shape == (2 * Cout * K,) and p.dtype == np.uint16
    val = lambda b: (np.array([b], dtype=np.uint32) << 16).view(np.float32)[0]
    # element of (kb = 1, ct = 1, lane = 37, j = 5): column 32 + 5, channel 16 + 8 + 5
    e = lambda piece: (((1 * 2 + 1) * 2 + piece) * 64 + 37) * 8 + 5
    assert val(p[e(0)]) + val(p[e(1)]) == w[37, 29]
    assert val(p[e(0)]) == float(torch.tensor(w[37, 29]).bfloat16())


# ------------------------------------------------------------------------------------------------------------- fixture G5
@pytest.mark.parametrize("N", [128, 64])
def test_emulated_block_meets_the_contract_on_g5(N):
    g = np.load(os.path.join(GOLD, "G5_transformer.npz"))
    xyz, feats = torch.from_numpy(g["xyz%d" % N]), torch.from_numpy(g["feat%d" % N])
    P = {n: v.double() for n, v in transformer_params(500 + N).items()}
    knn = torch.from_numpy(O.knn(g["xyz%d" % N], 16)).long()
    res, attn, _ = PS.block(xyz.double(), feats.double(), P, 16, knn, True)
    exact, _, _ = PS.block(xyz.double(), feats.double(), P, 16, knn, False)
    print("G5 N=%d: max |res - fixture| split %.2e, exact %.2e; attn sample %.2e" % (
        N, float((res - torch.from_numpy(g["res%d" % N]).double()).abs().max()),
        float((exact - torch.from_numpy(g["res%d" % N]).double()).abs().max()),
        float((attn[:, ::16, :, ::32] - torch.from_numpy(g["attn_sample%d" % N]).double()).abs().max())))
    np.testing.assert_allclose(res.numpy(), g["res%d" % N], **FR.TOL)
    np.testing.assert_allclose(attn[:, ::16, :, ::32].numpy(), g["attn_sample%d" % N], **FR.TOL)


# ---------------------------------------------------------------------------------------------------- the public interface
def _cfg(name='TransformerBlock', **kw):
    return AttrDict(NAME=name, DIM_INPUT=256, DIM_MODEL=512, KNN=16, N_HEADS=4 if name == 'MulTransformerBlock' else 1, N_LAYERS=1, **kw)


def test_precision_key_of_build_transformer():
    assert build_transformer(_cfg()).precision == 'fp32'
    assert build_transformer(_cfg(PRECISION='fp32')).precision == 'fp32'
    assert build_transformer(_cfg(PRECISION='bf16x2')).precision == 'bf16x2'
    with pytest.raises(ValueError):
        build_transformer(_cfg(PRECISION='fp16'))
    for name in ('TransformerBlockSTD', 'MulTransformerBlock'):
        build_transformer(_cfg(name, PRECISION='fp32'))
        with pytest.raises(ValueError, match="PRECISION"):
            build_transformer(_cfg(name, PRECISION='bf16x2'))
    with pytest.raises(NotImplementedError):                       # the names refused today stay refused
        build_transformer(_cfg('TransformerBlockALL', PRECISION='bf16x2'))


def test_precision_attribute_is_validated():
    blk = TransformerBlock(256, 128, 8)
    assert blk.precision == 'fp32'
    blk.precision = 'bf16x2'
    assert blk.precision == 'bf16x2'
    for bad in ('bf16', 'BF16X2', None, 2):
        with pytest.raises(ValueError):
            blk.precision = bad
    assert blk.precision == 'bf16x2'
    assert 'precision' not in blk.state_dict() and not any('precision' in n for n in blk.state_dict())


def test_set_precision_counts_and_bumps_versions():
    model = torch.nn.ModuleDict(dict(a=TransformerBlock(256, 128, 8), b=torch.nn.Sequential(TransformerBlock(256, 256, 16), torch.nn.ReLU()),
                                     c=torch.nn.Linear(4, 4)))
    blocks = [model['a'], model['b'][0]]
    watch = ops.StateWatch(model)
    before = [[p._version for p in b.parameters()] for b in blocks]
    values = [b.fc1.weight.detach().clone() for b in blocks]
    assert set_precision(model, 'bf16x2') == 2
    assert all(b.precision == 'bf16x2' for b in blocks)
    assert watch.changed()                                         # what makes a runner capture again
    for b, old, v in zip(blocks, before, values):
        assert sum(p._version - o for p, o in zip(b.parameters(), old)) == 1       # ONE parameter of each block
        assert torch.equal(b.fc1.weight, v)
    watch.mark()
    assert set_precision(model, 'fp32') == 2 and watch.changed()
    assert set_precision(model['c'], 'bf16x2') == 0
    assert set_precision(blocks[0], 'bf16x2') == 1                 # the model itself may be the block
    with pytest.raises(ValueError):
        set_precision(model, 'fp8')
    assert blocks[1].precision == 'fp32'


def test_cpu_forward_does_not_depend_on_precision():
    """The split kernel is the eval-mode HIP path's; the stock op sequence is untouched."""
    torch.manual_seed(0)
    blk = TransformerBlock(256, 128, 8).eval()
    xyz, f = torch.randn(1, 16, 3), torch.randn(1, 16, 256)
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("error")
        a = blk(xyz, f)[0]
        blk.precision = 'bf16x2'
        b = blk(xyz, f)[0]
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------------- ABI
def test_abi_37_binds_the_new_entry_points():
    with open(os.path.join(ROOT, "include", "ptt_hip.h")) as fh:
        header = fh.read()
    assert int(re.search(r"^#define\s+PTT_ABI_VERSION\s+(\d+)", header, flags=re.M).group(1)) == _lib.ABI_VERSION >= 37
    import ctypes
    P = _lib.PROTOTYPES
    assert P["ptt_split_weight_elems"] == (ctypes.c_int, [ctypes.c_int, ctypes.c_int])
    assert P["ptt_pack_weight_split_bf16"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p])
    assert P["ptt_pt_attn_pair_split_f32"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p])
    # the descriptor: ptt_attn_desc's fields without `heads`, in the header's order
    body = re.search(r"typedef struct ptt_attn_split_desc \{(.*?)\} ptt_attn_split_desc;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert names == [n for n, _ in _lib.AttnSplitDesc._fields_]
    assert [n for n, _ in _lib.AttnDesc._fields_ if n != "heads"] == [n.replace("Wd2s", "Wd2p").replace("Wg1s", "Wg1p").replace("Wg2s", "Wg2p")
                                                                      for n in names]
    assert ctypes.sizeof(_lib.AttnSplitDesc) == 13 * 8 + 4 * 4 + 8


def test_host_calls_of_the_split_pack():
    lib = _lib.lib()
    assert lib.ptt_version() == _lib.ABI_VERSION
    assert lib.ptt_split_weight_elems(128, 128) == 2 * 128 * 128 and lib.ptt_split_weight_elems(512, 512) == 2 * 512 * 512
    assert lib.ptt_split_weight_elems(0, 16) == 0
    # refused before any device work: no GPU is needed to see the status
    for Cout, K in ((128, 24), (48, 128)):
        assert lib.ptt_error_name(lib.ptt_pack_weight_split_bf16(None, Cout, K, None, None)) == b"PTT_EINVAL"
    assert b"K % 16 == 0" in lib.ptt_last_error_string()
