"""ptt_sa_fused_fwd_f32 with every option of ptt_sa_desc at its OTHER value — use_xyz = 0, normalize_xyz = 0, a layer without
ReLU (last, inner, the hoisted layer 0: l0_relu = 0), shift = NULL and scale = NULL — on clouds whose balls hold distinct points,
against float64, behind guard bands. The method, the helpers (tests/fused_launch.py) and the assertions (a) - (f) are those of
tests/test_fused_guard_gpu.py, unchanged: every launch goes through guard.launch with guarded outputs, embedded inputs and a
compact workspace of exactly the queried size; (a) err <= R * Y against float64, R = 4; (b) the 1e-4 contract against the float32
twin of the reference; (c) guards of outputs, workspaces and inputs; (d) output layouts A, B, C and both feature layouts give the
same bits; (e) a second run repeats them; (f) the compact run equals the dense run bit for bit where compact_ws is honoured.

Why these cases. tests/test_fused_guard_gpu.py sets use_xyz = normalize_xyz = l0_relu = 1, every layer with ReLU and a shift, on
resampled clouds whose balls hold the centre and copies of it (rel is mostly 0): a kernel that ignored its coordinate channels
would pass two of its cases. fused_ref.SA_OPTION_CASES puts the same 13 shapes on uniform clouds in the unit cube (cloud 1 a copy
of cloud 0 and the last cloud all zero when B >= 3) with one option set each; tests/test_fused_ref_cpu.py asserts for every case
that flipping each flag it varies moves >= 20 % of the float64 reference's outputs by more than 1e-2 * (1 + |ref|), that a
ReLU-less last layer leaves >= 10 % of them below -1e-3, and that the kernel named below is the one fused_ref.sa_dispatch gives.

  option set                          case (shape of SA_CASES)   kernel reached                                    err / Y
  normalize_xyz = 0                   norm0_lds4_111             sa_lds_kernel<false|true>, 4 waves                   1.46
                                      norm0_lds12_1035           sa_lds_kernel<false|true>, 12 waves                  1.46
                                      norm0_wave32_5             sa_wave_kernel<32,1>                                 1.29
                                      norm0_wave16_21            sa_wave_kernel<16,1>                                 0.91
                                      norm0_stream_33            sa_stream_kernel<32> / sa_stream_compact_kernel      1.00
                                      norm0_stream_1027          sa_stream_kernel<32> / sa_stream_compact_kernel      0.79
                                      norm0_fused32_33           sa_fused_kernel<32,2>                                1.01
                                      norm0_fused16_21           sa_fused_kernel<16,2>                                0.74
                                      norm0_fused64_10           sa_fused_kernel<64,2>                                0.88
  use_xyz = 0, layer 0 rot = 0        noxyz_wave16_18  (C = 5)   sa_wave_kernel<16,1>                                 0.89
                                      noxyz_fused32_33 (C = 128) sa_fused_kernel<32,2>, vector gather                 0.77
                                      noxyz_fused16_21 (C = 257) sa_fused_kernel<16,2>, scalar gather                 1.00
                                      noxyz_fused64_10 (C = 12)  sa_fused_kernel<64,2>                                0.77
  last layer relu = 0                 last0_lds4_1               sa_lds_kernel<false|true>                            0.83
                                      last0_wave16_18            sa_wave_kernel<16,1>                                 0.86
                                      last0_stream_1029          sa_stream_kernel<32> / sa_stream_compact_kernel      0.78
                                      last0_fused32_33           sa_fused_kernel<32,2>                                0.71
                                      last0_fused16_21           sa_fused_kernel<16,2>                                0.99
                                      last0_fused64_10           sa_fused_kernel<64,2>                                0.77
  inner layer relu = 0                inner0_lds4_111            sa_wave_kernel<32,1>: `p.L[0].relu && ..` fails      0.67
                                      inner1_lds4_111            sa_wave_kernel<32,1>: `.. && p.L[1].relu` fails      0.71
                                      inner1_lds12_1035          sa_wave_kernel<32,1>: `.. && p.L[1].relu` fails      0.92
                                      inner0_stream_33           sa_fused_kernel<32,2>, hoist 2: `p.L[0].relu` fails  0.99
                                      inner1_fused32_33          sa_fused_kernel<32,2>, layer 0 inside: middle layer  0.96
  l0_relu = 0                         l0relu0_stream_1027        sa_stream_kernel<32> / sa_stream_compact_kernel      0.85
                                      l0relu0_fused16_21h        sa_fused_kernel<16,2>, hoist == 1                    1.17
  shift = NULL, scale = NULL          none_wave16_18             sa_wave_kernel<16,1>                                 0.50
                                      none_fused16_21            sa_fused_kernel<16,2> (layer 1: a bias, no scale)    0.97
  scale set, shift = NULL             bn0_wave32_5               sa_wave_kernel<32,1>                                 0.80
                                      bn0_fused32_33             sa_fused_kernel<32,2> (layer 1: both set)            0.94
  shift = NULL, scale folded          bn0_lds4_1                 sa_lds_kernel<false|true>                            0.67
                                      bn0_stream_33              sa_stream_kernel<32> / sa_stream_compact_kernel      0.77

(err / Y measured on an MI355X, worst over the layouts of a case — the layouts agree bit for bit. The worst is 1.46, below the
2.0 from which a case is to be investigated; R = 4 and its cap 8 are those of tests/test_fused_guard_gpu.py. No kernel fault was
found.)

Refusals (host-side argument checks, nothing is launched; fused_launch.REFUSALS names the sentence of include/ptt_hip.h each
follows from): use_xyz = 0 with C = 0, and a hoisted layer 0 with use_xyz = 0 — PTT_EINVAL, every output word untouched.
"""
import ctypes

import pytest

from tests import fused_ref as FR
from tests import guard
from tests.fused_launch import R_RATIO, Ratios, SaInputs, embed, out_view, refused, run_sa_case, sa_desc

pytestmark = pytest.mark.gpu

RATIOS = Ratios()           # case -> worst err / Y of its runs: printed by test_zz_ratio_report


def test_r_is_within_its_cap():
    assert R_RATIO <= 8


@pytest.mark.parametrize("name", list(FR.SA_OPTION_CASES))
def test_sa_option(dev, name):
    run_sa_case(dev, FR.sa_option_case(name), name, RATIOS)                  # (a) - (f)


def test_refusal_no_xyz_and_no_features(dev):
    """use_xyz = 0 with C = 0: every array has the size the launch would need with use_xyz = 1."""
    c = FR.sa_option_case("norm0_lds4_111")
    s = SaInputs(c, dev, "none")
    out, strides, _ = out_view(dev, "A", c.B, c.M, c.spec[-1])
    d = sa_desc(s, out, strides)
    d.use_xyz = 0
    refused("sa_noxyz_C0", lambda: guard.launch("ptt_sa_fused_fwd_f32", dev, ctypes.byref(d)), out)


def test_refusal_hoisted_layer0_without_xyz(dev):
    """A hoisted layer 0 with use_xyz = 0. feat / C are set as well (a hoisted launch ignores them), so that this is not the
    refusal above: the launch is turned away for the hoisted layer 0 alone."""
    c = FR.sa_option_case("l0relu0_fused16_21h")
    s = SaInputs(c, dev, "none")
    out, strides, _ = out_view(dev, "A", c.B, c.M, c.spec[-1])
    feat = embed(c.feats.to(dev).contiguous())
    d = sa_desc(s, out, strides)
    d.feat, d.C, (d.feat_sb, d.feat_sc, d.feat_sn) = feat.data_ptr(), c.C, feat.stride()
    d.use_xyz = 0
    with pytest.raises(RuntimeError, match="hoisted layer 0 needs use_xyz"):
        guard.launch("ptt_sa_fused_fwd_f32", dev, ctypes.byref(d))
    refused("sa_noxyz_hoist", lambda: guard.launch("ptt_sa_fused_fwd_f32", dev, ctypes.byref(d)), out)


def test_zz_ratio_report():
    """Not a check of its own: the err / Y table of the run (pytest -s), the source of the table above — per case, the worst
    over its layouts."""
    worst = {}
    for k, v in RATIOS.items():
        worst[k.split()[0]] = max(worst.get(k.split()[0], 0.0), v)
    for k in FR.SA_OPTION_CASES:
        if k in worst:
            print("REPORT %-24s %.2f" % (k, worst[k]))
    top = max(worst.values()) if worst else 0.0
    print("REPORT worst err/Y %.2f over %d results; R = %g" % (top, len(RATIOS), R_RATIO))
    assert top <= R_RATIO
