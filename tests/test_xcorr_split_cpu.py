"""The split-bf16 xcorr kernel's arithmetic, attribute, scope, config key and bindings, without a GPU (tests/xcorr_split_ref.py).

Each figure is a condition on the reference alone. On the planted cases (operands that split exactly, all positive), as
max|. - split64| / max|split64 - exact64| (measured values in parentheses, cases (1,1,64) / (3,5,192)):
  * exact64 >= split64 everywhere
  * the float32 run of the emulation <= 0.15                                       (0.079 / 0.114)
  * a float32 evaluation without the split >= 0.9                                  (1.06 / 1.10)
  * a variant without the a_lo . w_hi term >= 10                                   (507 / 569)
These are the values that make the GPU test's bar of 0.3 mean something. On the generic cases (1,1,64) / (3,5,192) / (2,3,128):
  * split64 lies < 1 of fused_ref.TOL from the case's ref64                        (0.16 - 0.24)
Then CosineSimAug.precision, set_precision's scope 'similarity', SIMILARITY_MODULE.PRECISION and ABI 39.
"""
import ctypes
import os
import re
import warnings

import pytest
import torch

from ptt_amd import _lib, ops
from ptt_amd.config import StubDataset, ptt_model_cfg
from ptt_amd.hot_path import AttrDict
from ptt_amd.models import build_network
from ptt_amd.models.backbones_3d.pointnet2.pointnet2_modules import PointnetSAModuleVotes
from ptt_amd.models.similarity_modules.p2b_xcoor import CosineSimAug
from ptt_amd.models.transformer_block.variants import TransformerBlock
from ptt_amd.precision import SCOPES, set_precision
from tests import fused_ref as FR
from tests import xcorr_split_ref as XS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("shape", XS.PLANTED)
def test_planted_reference(shape):
    c = XS.planted_case(*shape)
    for t in (c.p.W1, c.p.W2, c.p.P):                                      # the operands split exactly
        hi, lo = XS.split2(t)
        assert torch.equal((hi + lo).float(), t) and torch.equal(lo, hi * 2.0 ** -9)
    assert bool((c.exact64 >= c.split64).all())
    own = float((c.split64 - c.exact64).abs().max())
    of_own = lambda t: float((t.double() - c.split64).abs().max()) / own
    run32, plain, drop = of_own(c.split32), of_own(c.plain32), of_own(c.drop64)
    print("%s: |split64 - exact64| %.3e; of it: split32 %.3f, plain32 %.3f, drop64 %.0f" % (c.p.name, own, run32, plain, drop))
    assert own > 0
    assert run32 <= 0.15
    assert plain >= 0.9
    assert drop >= 10


@pytest.mark.parametrize("shape", XS.GENERIC)
def test_generic_reference(shape):
    g = XS.generic_case(*shape)
    base = FR.xcorr_case(*shape, FR.XCORR_F, XS.WIDTHS)
    print("%s: Y = %.2e, e32(split32, split64) = %.2e" % (g.p.name, g.Y, FR.e32_of(g.split32, g.split64)))
    for what, t in (("split64", g.split64), ("exact64", g.exact64)):
        share = float(((t - base.ref64).abs() / (FR.TOL["atol"] + FR.TOL["rtol"] * base.ref64.abs())).max())
        print("%s: %s at %.2f of TOL from ref64" % (g.p.name, what, share))
        assert share < 1
    # the flags of the level change its result: what the GPU test's "a changed flag changes a bit" rests on
    assert not torch.equal(XS.generic_case(*shape, relu2=False).split64, g.split64)
    assert not torch.equal(XS.generic_case(*shape, shifts=False).split64, g.split64)


# ---------------------------------------------------------------------------------------------------- the public interface
def _cfg(channels=(260, 256, 256, 256), **kw):
    return AttrDict.wrap(dict(DEBUG=False, MLP=dict(CHANNELS=list(channels), BN=True), CONV=dict(CHANNELS=[256, 256, 256], BN=True), **kw))


def test_precision_attribute_is_validated():
    m = CosineSimAug(_cfg())
    assert m.precision == 'fp32'
    m.precision = 'bf16x2'
    assert m.precision == 'bf16x2'
    for bad in ('bf16', 'BF16X2', None, 2):
        with pytest.raises(ValueError):
            m.precision = bad
    assert m.precision == 'bf16x2'
    assert not any('precision' in n for n in m.state_dict())
    assert sorted(m.state_dict()) == sorted(CosineSimAug(_cfg()).state_dict())


def test_precision_change_drops_the_parameter_caches():
    m = CosineSimAug(_cfg())
    m._cache.get([], torch.device('cpu'), lambda: 'layers')            # as if an eval forward had built it
    m._split_cache.get([], torch.device('cpu'), lambda: 'packs')
    m.precision = 'fp32'                                               # no change: nothing is dropped
    assert m._cache.held() and m._split_cache.held()
    m.precision = 'bf16x2'
    assert not m._cache.held() and not m._split_cache.held()


def test_config_key():
    assert CosineSimAug(_cfg()).precision == 'fp32'
    assert CosineSimAug(_cfg(PRECISION='bf16x2')).precision == 'bf16x2'
    with pytest.raises(ValueError):
        CosineSimAug(_cfg(PRECISION='fp16'))
    cfg = ptt_model_cfg()
    cfg.SIMILARITY_MODULE['PRECISION'] = 'bf16x2'
    tracker = build_network(cfg, 1, StubDataset())
    assert [m.precision for m in tracker.modules() if isinstance(m, CosineSimAug)] == ['bf16x2']
    cfg = ptt_model_cfg()
    cfg.SIMILARITY_MODULE['PRECISION'] = 'fp16'
    with pytest.raises(ValueError):
        build_network(cfg, 1, StubDataset())


def test_cpu_and_training_calls_run_as_before_and_say_so_once():
    torch.manual_seed(0)
    m = CosineSimAug(_cfg(channels=(12, 32, 32, 256))).eval()
    batch = lambda: {'search_feats': torch.randn(2, 8, 5, generator=torch.Generator().manual_seed(1)),
                     'template_feats': torch.randn(2, 8, 64, generator=torch.Generator().manual_seed(2)),
                     'template_seeds': torch.randn(2, 64, 3, generator=torch.Generator().manual_seed(3))}
    ops.precision_fallbacks.clear()
    with torch.no_grad(), warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        y0 = m(batch())['cosine_feats']
        assert not ops.precision_fallbacks and not seen                 # 'fp32': no note, no warning
        m.precision = 'bf16x2'
        y1 = m(batch())['cosine_feats']
        y2 = m(batch())['cosine_feats']
    assert torch.equal(y0, y1) and torch.equal(y0, y2)
    assert list(ops.precision_fallbacks.items()) == [(('CosineSimAug', 'CPU: no split-bf16 form'), 2)]
    assert len([w for w in seen if "bf16x2" in str(w.message)]) == 1
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        m.train()(batch())
    assert ('CosineSimAug', 'training: the training forms are fp32 only') in ops.precision_fallbacks
    assert len([w for w in seen if "bf16x2" in str(w.message)]) == 1
    ops.precision_fallbacks.clear()


def _versions(m):
    return [p._version for p in m.parameters()]


def test_set_precision_scope_similarity():
    assert SCOPES == ('transformer', 'sa', 'similarity')
    model = build_network(ptt_model_cfg(), 1, StubDataset())
    sims = [m for m in model.modules() if isinstance(m, CosineSimAug)]
    sas = list(model.backbone_3d.SA_modules)
    tbs = [m for m in model.modules() if isinstance(m, TransformerBlock)]
    assert len(sims) == 1 and len(sas) == 3 and all(isinstance(m, PointnetSAModuleVotes) for m in sas)
    sim, everything = sims[0], sims + sas + tbs
    # the default scope and the two earlier scopes: their counts as before, the similarity module untouched
    before = _versions(sim)
    assert set_precision(model, 'bf16x2') == len(tbs)
    assert set_precision(model, 'bf16x2', scope=('transformer', 'sa')) == len(tbs) + 3
    assert sim.precision == 'fp32' and _versions(sim) == before
    assert set_precision(model, 'fp32', scope=('transformer', 'sa')) == len(tbs) + 3
    # 'similarity' alone: one module, one parameter version, values untouched, every StateWatch sees it
    watch = ops.StateWatch(model)
    others = [_versions(m) for m in sas + tbs]
    value = sim.mlp[0].conv.weight.detach().clone()
    assert set_precision(model, 'bf16x2', scope=('similarity',)) == 1
    assert sim.precision == 'bf16x2' and watch.changed()
    assert sum(a - b for a, b in zip(_versions(sim), before)) == 1
    assert sim.mlp[0].conv.weight._version == before[0] + 1 and torch.equal(sim.mlp[0].conv.weight, value)
    assert [_versions(m) for m in sas + tbs] == others and all(m.precision == 'fp32' for m in sas + tbs)
    # with the other scopes; the module may be the model itself; a string names one scope
    assert set_precision(model, 'bf16x2', scope=('transformer', 'sa', 'similarity')) == len(tbs) + 3 + 1
    assert all(m.precision == 'bf16x2' for m in everything)
    assert set_precision(model, 'fp32', scope=('transformer', 'sa')) == len(tbs) + 3 and sim.precision == 'bf16x2'
    assert set_precision(sim, 'fp32', scope='similarity') == 1 and sim.precision == 'fp32'
    assert set_precision(sim, 'bf16x2') == 0 and set_precision(sim, 'bf16x2', scope=('sa',)) == 0 and sim.precision == 'fp32'
    # a bad scope or value changes nothing
    before = [_versions(m) for m in everything]
    for bad in (('similarity', 'xcorr'), ('Similarity',), 'cosine'):
        with pytest.raises(ValueError):
            set_precision(model, 'bf16x2', scope=bad)
    with pytest.raises(ValueError):
        set_precision(model, 'fp8', scope=('similarity',))
    assert [_versions(m) for m in everything] == before and all(m.precision == 'fp32' for m in everything)


# ------------------------------------------------------------------------------------------------------------------- ABI
FIELDS = ["cos_t", "P", "w_sim", "W1s", "shift1", "W2s", "shift2", "relu2", "out", "out_sb", "out_sc", "out_sn", "B", "Ns", "Nt"]


def test_abi_39_binds_the_new_entry_point():
    with open(os.path.join(ROOT, "include", "ptt_hip.h")) as fh:
        header = fh.read()
    assert int(re.search(r"^#define\s+PTT_ABI_VERSION\s+(\d+)", header, flags=re.M).group(1)) == _lib.ABI_VERSION >= 39
    assert _lib.PROTOTYPES["ptt_xcorr_split_f32"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p])
    body = re.search(r"typedef struct ptt_xcorr_split_desc \{(.*?)\} ptt_xcorr_split_desc;", header, flags=re.S).group(1)
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
    assert fields == list(_lib.XcorrSplitDesc._fields_)
    assert [n for n, _ in fields] == FIELDS
    assert ops.XcorrSplitDesc is _lib.XcorrSplitDesc and callable(ops.xcorr_split)


def test_descriptor_matches_the_c_header(tmp_path):
    """sizeof / offsetof from gcc against ctypes, as tests/test_oracle_cpu.py does for the structures it lists."""
    import subprocess
    cname, st = "ptt_xcorr_split_desc", _lib.XcorrSplitDesc
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
    call = lambda d: lib.ptt_xcorr_split_f32(ctypes.byref(d), None)
    assert name(lib.ptt_xcorr_split_f32(None, None)) == b"PTT_EINVAL"
    d = _lib.XcorrSplitDesc()
    d.B, d.Ns, d.Nt = 0, 128, 64
    assert call(d) == 0                                                    # B == 0: PTT_OK, nothing launched
    d.B, d.Ns = 2, 0
    assert call(d) == 0                                                    # Ns == 0
    d.Ns = 128
    assert name(call(d)) == b"PTT_EINVAL"                                  # null pointers
    ptrs = ("cos_t", "P", "w_sim", "W1s", "W2s", "out")
    for f in ptrs:
        setattr(d, f, 4096)
    for f in ptrs:                                                         # each of them alone
        setattr(d, f, None)
        assert name(call(d)) == b"PTT_EINVAL" and b"null pointer" in lib.ptt_last_error_string(), f
        setattr(d, f, 4096)
    for f in ("P", "w_sim", "W1s", "W2s"):
        setattr(d, f, 4096 + 4)
        assert name(call(d)) == b"PTT_EINVAL" and b"16-byte" in lib.ptt_last_error_string(), f
        setattr(d, f, 4096)
    for f in ("out_sb", "out_sc", "out_sn"):
        setattr(d, f, -1)
        assert name(call(d)) == b"PTT_EINVAL" and b"negative" in lib.ptt_last_error_string(), f
        setattr(d, f, 1)
    for nt in (0, -64, 96, 65):
        d.Nt = nt
        assert name(call(d)) == b"PTT_EUNSUPPORTED", nt
    d.B, d.Ns, d.Nt = 4096, 4096, 64                                       # cos_t (B,Ns,Nt) floats: 4 GiB
    assert name(call(d)) == b"PTT_EUNSUPPORTED" and b"2 GiB" in lib.ptt_last_error_string()
    d.B, d.Ns, d.Nt = 2, 4, 64
    d.out_sb = 1 << 30                                                     # the last output element: past 2 GiB
    assert name(call(d)) == b"PTT_EUNSUPPORTED"
