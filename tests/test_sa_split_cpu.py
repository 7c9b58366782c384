"""The split-bf16 stream kernel's arithmetic, attribute, config key and bindings, without a GPU (tests/sa_split_ref.py).

Each figure is a condition on the reference alone (measured values in parentheses, generic cases stream_33 / _1027 / _1029):
  * 0 < e32(split32, split64) <= 1e-5                                              (4.0e-6 / 4.9e-6 / 5.4e-6)
  * a variant without the a_lo . w_hi term lies >= 50 x max|split64 - exact64| from split64     (274 - 425 x)
  * split64 meets fused_ref.TOL against the case's ref64                           (at most 0.71 of the bound; split32 0.77)
and on the planted cases (index tables of stream_33 / stream_1027, operands that split exactly, all positive):
  * exact64 >= split64 everywhere
  * max|split32 - split64| <= 0.15 x max|split64 - exact64|
  * a float32 evaluation without the split lies >= 0.9 of that distance from split64
Then PointnetSAModuleVotes.precision, set_precision's scope, SA_CONFIG.PRECISION and ABI 38.
"""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest
import torch

from ptt_amd import _lib, ops
from ptt_amd.hot_path import FrameHotPath, kitti_model_cfg
from ptt_amd.models.backbones_3d.pointnet2.pointnet2_modules import PointnetSAModuleVotes
from ptt_amd.models.transformer_block.variants import TransformerBlock
from ptt_amd.precision import set_precision
from tests import fused_ref as FR
from tests import sa_split_ref as SS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("name", SS.GENERIC)
def test_generic_reference(name):
    g = SS.generic_case(name)
    base = FR.sa_case(name)
    e32 = FR.e32_of(g.split32, g.split64)
    print("%s: e32(split32, split64) = %.2e, Y = %.2e" % (name, e32, g.Y))
    assert 0 < e32 <= 1e-5
    own = float((g.split64 - g.exact64).abs().max())
    drop = float((SS.level(g.p, torch.float64, "drop") - g.split64).abs().max())
    print("%s: without a_lo . w_hi %.3e from split64 = %.0f x the split's own %.3e from exact" % (name, drop, drop / own, own))
    assert own > 0 and drop >= 50 * own
    # exact64 differs from the case's own ref64 only by the float32 fold of the BatchNorm scale into the weights
    print("%s: max|exact64 - ref64| = %.2e" % (name, float((g.exact64 - base.ref64).abs().max())))
    for what, t in (("split64", g.split64), ("split32", g.split32.double())):
        share = float(((t - base.ref64).abs() / (FR.TOL["atol"] + FR.TOL["rtol"] * base.ref64.abs())).max())
        print("%s: %s at %.2f of TOL from ref64" % (name, what, share))
    np.testing.assert_allclose(g.split64.numpy(), base.ref64.numpy(), **FR.TOL)


@pytest.mark.parametrize("name", SS.PLANTED)
def test_planted_reference(name):
    c = SS.planted_case(name)
    hi, lo = SS.split2(c.p.W1)
    assert torch.equal((hi + lo).float(), c.p.W1) and torch.equal(lo, hi * 2.0 ** -9)          # the operands split exactly
    hi, lo = SS.split2(c.p.term)
    assert torch.equal((hi + lo).float(), c.p.term) and torch.equal(lo, hi * 2.0 ** -9)
    assert bool((c.exact64 >= c.split64).all())
    own = float((c.split64 - c.exact64).abs().max())
    run32 = float((c.split32.double() - c.split64).abs().max())
    plain = float((c.plain32.double() - c.split64).abs().max())
    print("%s: |split32 - split64| %.3e = %.3f, |plain32 - split64| %.3e = %.3f of |split64 - exact64| %.3e"
          % (name, run32, run32 / own, plain, plain / own, own))
    assert run32 <= 0.15 * own
    assert plain >= 0.9 * own


# ---------------------------------------------------------------------------------------------------- the public interface
def _sa(**kw):
    return PointnetSAModuleVotes(mlp=[128, 128, 128, 256], radius=0.5, nsample=32, normalize_xyz=True, **kw)


def test_precision_attribute_is_validated():
    m = _sa()
    assert m.precision == 'fp32'
    m.precision = 'bf16x2'
    assert m.precision == 'bf16x2'
    for bad in ('bf16', 'BF16X2', None, 2):
        with pytest.raises(ValueError):
            m.precision = bad
    assert m.precision == 'bf16x2'
    assert not any('precision' in n for n in m.state_dict())
    assert sorted(m.state_dict()) == sorted(_sa().state_dict())


def test_precision_change_drops_the_parameter_cache():
    m = _sa()
    m._fused_cache.get([], torch.device('cpu'), lambda: 'layers')       # as if an eval forward had built it
    m._split_cache.get([], torch.device('cpu'), lambda: 'packs')
    m.precision = 'fp32'                                                # no change: nothing is dropped
    assert m._fused_cache.held() and m._split_cache.held()
    m.precision = 'bf16x2'
    assert not m._fused_cache.held() and not m._split_cache.held()


def test_cpu_forward_does_not_depend_on_precision():
    """The module has no CPU forward (its sampling and grouping operators are HIP kernels): a CPU call ends in the same refusal in
    both modes, with no precision warning and no fallback counted — the attribute is read by the eval-mode HIP path alone."""
    torch.manual_seed(0)
    m = _sa().eval()
    xyz, f = torch.rand(2, 64, 3), torch.randn(2, 128, 64)
    inds = torch.arange(16, dtype=torch.int32).repeat(2, 1)
    ops.precision_fallbacks.clear()
    said = []
    for precision in ('fp32', 'bf16x2'):
        m.precision = precision
        with torch.no_grad(), warnings.catch_warnings():
            warnings.simplefilter("error")
            with pytest.raises(RuntimeError, match="CPU tensors are not supported") as e:
                m(xyz, f, 16, inds=inds)
        said.append(str(e.value))
    assert said[0] == said[1] and not ops.precision_fallbacks


def _versions(m):
    return [p._version for p in m.parameters()]


def test_set_precision_scope():
    model = FrameHotPath(kitti_model_cfg())
    sas = list(model.backbone_3d.SA_modules)                   # the levels SA_CONFIG.PRECISION configures
    box = model.vote_aggregation                               # 257 -> 256 -> 256 -> 256 on 16 neighbours: no second arithmetic
    box_before = _versions(box)
    tbs = [m for m in model.modules() if isinstance(m, TransformerBlock)]
    assert len(sas) == 3 and len(tbs) == 2 and all(isinstance(m, PointnetSAModuleVotes) for m in sas + [box])
    # the default scope: today's behaviour, TransformerBlocks only
    before = [_versions(m) for m in sas]
    assert set_precision(model, 'bf16x2') == 2
    assert all(m.precision == 'fp32' for m in sas) and all(m.precision == 'bf16x2' for m in tbs)
    assert [_versions(m) for m in sas] == before
    assert set_precision(model, 'fp32') == 2
    # both scopes: 2 + 3, one parameter version per module set
    watch = ops.StateWatch(model)
    before_sa, before_tb = [_versions(m) for m in sas], [_versions(m) for m in tbs]
    values = [m.mlp_module[0].conv.weight.detach().clone() for m in sas]
    assert set_precision(model, 'bf16x2', scope=('transformer', 'sa')) == 2 + 3
    assert all(m.precision == 'bf16x2' for m in sas + tbs) and watch.changed()
    for m, old, v in zip(sas, before_sa, values):
        assert sum(a - b for a, b in zip(_versions(m), old)) == 1
        assert m.mlp_module[0].conv.weight._version == old[0] + 1 and torch.equal(m.mlp_module[0].conv.weight, v)
    for m, old in zip(tbs, before_tb):
        assert sum(a - b for a, b in zip(_versions(m), old)) == 1
    assert box.precision == 'fp32' and _versions(box) == box_before
    # 'sa' alone; a level may be the model itself
    assert set_precision(model, 'fp32', scope=('sa',)) == 3
    assert set_precision(sas[1], 'bf16x2', scope=('sa',)) == 1 and set_precision(sas[1], 'fp32', scope='sa') == 1
    assert set_precision(sas[1], 'bf16x2') == 0 and sas[1].precision == 'fp32'
    assert all(m.precision == 'fp32' for m in sas) and all(m.precision == 'bf16x2' for m in tbs)
    # a bad scope changes nothing
    before = [_versions(m) for m in sas + tbs]
    for bad in (('transformer', 'xcorr'), ('SA',), 'backbone'):
        with pytest.raises(ValueError):
            set_precision(model, 'bf16x2', scope=bad)
    with pytest.raises(ValueError):
        set_precision(model, 'fp8', scope=('sa',))
    assert [_versions(m) for m in sas + tbs] == before
    assert all(m.precision == 'fp32' for m in sas) and all(m.precision == 'bf16x2' for m in tbs)


def test_sa_config_precision_reaches_the_three_modules():
    cfg = kitti_model_cfg()
    assert [m.precision for m in FrameHotPath(cfg).backbone_3d.SA_modules] == ['fp32'] * 3
    cfg = kitti_model_cfg()
    cfg.BACKBONE_3D.SA_CONFIG['PRECISION'] = 'bf16x2'
    assert [m.precision for m in FrameHotPath(cfg).backbone_3d.SA_modules] == ['bf16x2'] * 3
    cfg = kitti_model_cfg()
    cfg.BACKBONE_3D.SA_CONFIG['PRECISION'] = 'fp16'
    with pytest.raises(ValueError):
        FrameHotPath(cfg)


# ------------------------------------------------------------------------------------------------------------------- ABI
def test_abi_38_binds_the_new_entry_point():
    with open(os.path.join(ROOT, "include", "ptt_hip.h")) as fh:
        header = fh.read()
    assert int(re.search(r"^#define\s+PTT_ABI_VERSION\s+(\d+)", header, flags=re.M).group(1)) == _lib.ABI_VERSION >= 38
    assert _lib.PROTOTYPES["ptt_sa_stream_split_f32"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p])
    body = re.search(r"typedef struct ptt_sa_split_desc \{(.*?)\} ptt_sa_split_desc;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        names = [n.strip().lstrip("*").strip() for n in decl.split(",")]
        names[0] = names[0].replace("*", " ").split()[-1]
        ctype = ctypes.c_void_p if "*" in decl else {"int": ctypes.c_int, "float": ctypes.c_float, "long long": ctypes.c_longlong}[
            " ".join(decl.replace(",", " ").split()[:-len(names)])]
        fields += [(n, ctype) for n in names]
    assert fields == list(_lib.SaSplitDesc._fields_)
    assert [n for n, _ in fields] == ["xyz", "new_xyz", "idx", "l0_point_term", "l0_xyz_weight", "l0_relu", "W1s", "shift1", "W2s", "shift2",
                                      "relu2", "out", "out_sb", "out_sc", "out_sm", "B", "N", "M", "radius", "normalize_xyz"]


def test_descriptor_matches_the_c_header(tmp_path):
    """sizeof / offsetof from gcc against ctypes, as tests/test_oracle_cpu.py does for the structures it lists."""
    import subprocess
    cname, st = "ptt_sa_split_desc", _lib.SaSplitDesc
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ptt_hip.h"', 'int main(void) {',
             'printf("%s %%zu\\n", sizeof(%s));' % (cname, cname)]
    lines += ['printf("%s %%zu\\n", offsetof(%s, %s));' % (f, cname, f) for f, _ in st._fields_]
    lines += ['return 0;', '}']
    src, exe = tmp_path / "abi_probe.c", tmp_path / "abi_probe"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-I", os.path.dirname(_lib.HEADER_PATH), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got[cname]) == ctypes.sizeof(st)
    for f, _ in st._fields_:
        assert int(got[f]) == getattr(st, f).offset, f


def test_host_refusals_of_the_new_entry_point():
    """Refused before any device work: no GPU is needed to see the status."""
    lib = _lib.lib()
    assert lib.ptt_version() == _lib.ABI_VERSION
    name = lambda rc: lib.ptt_error_name(rc)
    assert name(lib.ptt_sa_stream_split_f32(None, None)) == b"PTT_EINVAL"
    d = _lib.SaSplitDesc()
    d.B, d.N, d.M = 0, 128, 16
    assert lib.ptt_sa_stream_split_f32(ctypes.byref(d), None) == 0            # B == 0: PTT_OK, nothing launched
    d.B, d.M = 2, 0
    assert lib.ptt_sa_stream_split_f32(ctypes.byref(d), None) == 0
    d.M = 16
    assert name(lib.ptt_sa_stream_split_f32(ctypes.byref(d), None)) == b"PTT_EINVAL"       # null pointers
    for f in ("xyz", "new_xyz", "idx", "l0_point_term", "l0_xyz_weight", "W1s", "W2s", "out"):
        setattr(d, f, 4096)
    d.l0_point_term = 4096 + 4
    assert name(lib.ptt_sa_stream_split_f32(ctypes.byref(d), None)) == b"PTT_EINVAL" and b"16-byte" in lib.ptt_last_error_string()
    d.l0_point_term = 4096
    d.B, d.N, d.M = 4096, 4096, 4096                                                   # (B,N,128) floats: 8 GiB
    assert name(lib.ptt_sa_stream_split_f32(ctypes.byref(d), None)) == b"PTT_EUNSUPPORTED"
