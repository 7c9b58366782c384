"""The fused eval-mode kernels — ptt_sa_fused_fwd_f32, ptt_xcorr_fused_fwd_f32, ptt_cosine_map_f32, ptt_pt_attn_pair_f32 — at
ragged shapes, against float64, behind guard bands (tests/guard.py, tests/fused_ref.py).

Every case launches the entry point through guard.launch with a descriptor filled here or in tests/fused_launch.py (the helpers
tests/test_sa_options_gpu.py shares): outputs are guarded(...), every input (packed weights, scale / shift vectors, idx, knn, qkv, cos_t, P, the hoisted point term included) is embed(...)-ded between NaN /
INDEX_FILL words (those that must be contiguous with lead and tail only), the compact workspace is guard.workspace(...) of
exactly ptt_sa_compact_workspace(B, M) bytes. Asserted per case:
  (a) max|got - ref64| / max|ref64| <= R * Y, Y = max(e32, 4u) the float32 oracle's own distance from float64 (fused_ref);
  (b) every value meets the existing 1e-4 contract against the float32 oracle;
  (c) check_guard on every output (all written), on every workspace and every input (nothing written);
  (d) the output layouts A (point-major dense), B (a channel slice of a wider point-major buffer: ld = Cout + 8, col_off = 4,
      batch stride > M * ld) and C (channel-major, row stride M + 3: odd, no row after the first 16-byte aligned) give the same
      bits, and so do both feature layouts of the SA cases (point-major: the vec_gather form where C % 4 == 0; channel-major
      with ld = N + 1: the scalar form) — `p.vec_gather` (mfma_ops.hip, ptt_sa_fused_fwd_f32) only selects how a row is LOADED.
      ptt_cosine_map_f32 is the exception: its two layouts run two differently compiled sums (see test_cos_map);
  (e) a second run gives the same bits;
  (f) where compact_ws is honoured, the compact run equals the dense run bit for bit.

The kernel each SA case reaches, from the dispatch in ptt_sa_fused_fwd_f32 (mfma_ops.hip, the chain of `if`s that follows
`const int total_centres = d->B * d->M;`; restated in fused_ref.sa_dispatch and pinned by tests/test_fused_ref_cpu.py):

  case          (B, N, M, C, spec, r, ns)                          kernel                      follows from
  lds4_1        (1, 64, 1, 0, [3,64,64,128], .3, 32) scale folded  sa_lds_kernel<false|true>   `d->C == 0 && ... !p.L[0].scale ...`; nw = 4:
  lds4_111      (3, 96, 37, 0, same)                               4 waves                     `total_centres * 3 <= 256 * PTT_SAL_WAVES ? 4 : ..`
  lds12_1035    (5, 512, 207, 0, same)                             12 waves, 87 workgroups     1035 * 3 > 3072; 1035 = 86 * 12 + 3
  wave32_5      (1, 64, 5, 0, same) scale separate                 sa_wave_kernel<32,1>        `wave_ok && wbytes <= 64 * 1024 && d->nsample <= 32`
  wave16_18     (2, 80, 9, 5, [8,32,64], .4, 16)                   sa_wave_kernel<16,1>        per_wg = 8: 18 = 2 * 8 + 2 (one full wave, three empty)
  wave16_21     (3, 80, 7, 5, same)                                sa_wave_kernel<16,1>        21 = 2 * 8 + 5: waves of 2, 2 and ONE centre
  stream_33     (1, 128, 33, 128, [131,128,128,256], .5, 32) l0    sa_stream_kernel<32> and    `p.hoist == 2 && d->nsample == 32 && d->n_layers == 2 ..`
  stream_1027   (13, 128, 79, same)                                sa_stream_compact_kernel    514 tiles, wgs capped at 512 -> p.chunk = 2, 257 workgroups
  stream_1029   (21, 128, 49, same)                                                            515 tiles: the last workgroup's chunk holds ONE tile
  fused32_33    (1, 128, 33, 128, same) layer 0 in the kernel      sa_fused_kernel<32,2>       PTT_SA_CASE(32, 2): nt = 4, 4, 8 is not wave_ok
  fused16_21    (3, 64, 7, 257, [260,256,256,256], .3, 16)         sa_fused_kernel<16,2>       PTT_SA_CASE(16, 2), 4 centres per workgroup, 21 centres
  fused16_21h   same, l0_channels = 256                            sa_fused_kernel<16,2>       hoist == 1 (not 128 channels): not the stream shape
  fused64_10    (2, 70, 5, 12, [15,64,128], .6, 64)                sa_fused_kernel<64,2>       `if (d->nsample == 64) RT = 2;` one centre = both row tiles
(stream_1027: 1027 centres -> 514 tiles -> chunk 2 leaves 257 whole chunks, only its last TILE is half empty. stream_1029 is the
neighbouring shape whose last chunk is short as well.)

xcorr: plain form xcorr_fused_kernel<2,false> (`if (!d->split)`), C0 in {8, 40, 256} — C0 = 40 takes layer 0's scalar form
(`256 % nq`), two remaining layers run with BatchNorm folded into P / w_sim (scale0 = shift0 = NULL, what the module passes),
three with scale0 / shift0 and per-layer scales kept; split form <1,true>; cos_map_kernel in both layouts.
Pair kernel: heads 1 (pt_attn_pair_kernel<512>) and 2 / 4 / 8 (pt_attn_pair_heads_kernel), N = k = 16 included.

Refusals: fused_launch.REFUSALS names the status and the sentence of include/ptt_hip.h each documented refusal follows from; a
refusal whose sentence is not in the header fails, a refused launch must leave every output word untouched, and no other launch may fail.

The ratio R. err / Y measured on an MI355X, worst over the layouts of a case (the layouts agree bit for bit); R = twice the
worst ratio (1.98), rounded up to one significant digit = 4, and R <= 8 is asserted. No case needed investigation.

  SA    lds4_1 0.40   lds4_111 0.64   lds12_1035 1.39   wave32_5 0.84   wave16_18 0.51   wave16_21 0.56   stream_33 0.85
        stream_1027 0.76   stream_1029 0.87   fused32_33 1.05   fused16_21 1.21   fused16_21h 0.76   fused64_10 0.91
  xcorr plain, (B,Ns,Nt) = (1,1,64) / (3,5,192), two | three remaining layers:
        C0 = 8: 0.50 | 0.30 / 0.83 | 0.68     C0 = 40: 0.87 | 1.02 / 0.78 | 1.24     C0 = 256: 1.98 | 0.79 / 0.96 | 0.91
  xcorr split (1,8,64,20) 0.70   (2,12,128,256) 1.11        cos map (1,20,9,3) 0.74   (2,300,5,130) 1.91
  pair  res / attn, worst over rel and order on / off (the same figures):
        heads 1: (1,16) 0.31 / 0.93   (3,18) 0.29 / 0.97   (1,50) 0.25 / 0.91      heads 2: 0.70 / 0.95   0.73 / 0.94   0.74 / 0.90
        heads 4: 1.09 / 0.88   0.81 / 0.99   1.06 / 0.98                            heads 8: 0.92 / 0.86   0.86 / 0.94   0.84 / 0.80
"""
import ctypes

import numpy as np
import pytest
import torch

from ptt_amd import ops
from tests import fused_ref as FR
from tests import guard
from tests.fused_launch import (F32, I32, R_RATIO, Ratios, SaInputs, embed_layers, fill_layers, fold, out_view, put, refused, run_sa_case,
                                same_bits, untouched_inputs)
from tests.guard import check_guard, embed, guarded

pytestmark = pytest.mark.gpu

RATIOS = Ratios()           # case -> worst err / Y of its runs: printed by test_zz_ratio_report
note, bound = RATIOS.note, RATIOS.bound


def test_r_is_within_its_cap():
    assert R_RATIO <= 8


# ======================================================================================================= set abstraction
@pytest.mark.parametrize("name", list(FR.SA_CASES))
def test_sa(dev, name):
    run_sa_case(dev, FR.sa_case(name), "sa %s" % name, RATIOS)


# ================================================================================================================= xcorr
def xcorr_inputs(c, dev, folded0):
    """-> (ins, dict of embedded operands) of one xcorr case. folded0: layer 0's BatchNorm folded into P and w_sim (scale0 =
    shift0 = NULL, what CosineSimAug passes) and the remaining layers' scales into their weights; else everything separate."""
    ins = []
    keep = lambda v: (ins.append(v), v)[1]
    C0 = c.widths[0]
    L0 = c.layers[0]
    w0 = L0["conv_weight"].reshape(C0, -1)                                          # (C0, 1 + 3 + f)
    s0 = L0["bn_weight"] / torch.sqrt(L0["bn_var"] + L0["eps"])
    t0 = L0["bn_bias"] - L0["bn_mean"] * s0
    # P = W0[:, 1:] . [xyz_i ; feat_i], one row per template point, formed in float32 on the host: the kernel under test is
    # the fused one, not the linear kernel that makes P in the module
    rows = torch.cat((c.txyz, c.tf.transpose(1, 2)), dim=2)                         # (B,Nt,3+f)
    P = torch.nn.functional.linear(rows, w0[:, 1:])
    o = {}
    if folded0:
        o["P"] = keep(put(P * s0 + t0, dev))
        o["w_sim"], o["scale0"], o["shift0"] = keep(put(w0[:, 0] * s0, dev)), None, None
    else:
        o["P"] = keep(put(P, dev))
        o["w_sim"], o["scale0"], o["shift0"] = keep(put(w0[:, 0], dev)), keep(put(s0, dev)), keep(put(t0, dev))
    o["layers"] = embed_layers(fold(c.layers[1:], dev, folded0), ins)
    return ins, o


def xcorr_desc(c, o, out, strides):
    d = ops.XcorrDesc()
    d.P, d.w_sim = o["P"].data_ptr(), o["w_sim"].data_ptr()
    d.scale0 = o["scale0"].data_ptr() if o["scale0"] is not None else None
    d.shift0 = o["shift0"].data_ptr() if o["shift0"] is not None else None
    d.out = out.data_ptr()
    d.out_sb, d.out_sc, d.out_sn = strides
    d.B, d.Ns, d.Nt, d.C0 = c.B, c.Ns, c.Nt, c.widths[0]
    fill_layers(d, o["layers"])
    return d


@pytest.mark.parametrize("sim_out", [False, True])
@pytest.mark.parametrize("C0,B,Ns,Nt,nrem", FR.XCORR_PLAIN)
def test_xcorr_plain(dev, C0, B, Ns, Nt, nrem, sim_out):
    widths = FR.XCORR_WIDTHS[(C0, nrem)]
    c = FR.xcorr_case(B, Ns, Nt, FR.XCORR_F, tuple(widths))
    ins, o = xcorr_inputs(c, dev, folded0=(nrem == 2))
    cos_t = ops.cosine_map(c.sf.to(dev), c.tf.to(dev), eps=1e-8)
    cos_e = embed(cos_t.contiguous())
    ins.append(cos_e)
    first = None
    name = "xcorr C0=%d (%d,%d,%d) +%d sim=%d" % (C0, B, Ns, Nt, nrem, sim_out)
    for lay in "AABC":                                                  # A twice: (e)
        out, strides, logical = out_view(dev, lay, B, Ns, widths[-1])
        d = xcorr_desc(c, o, out, strides)
        d.cos_t = cos_e.data_ptr()
        sim = guarded((B, Nt, Ns), F32, device=dev) if sim_out else None
        d.sim_out = sim.data_ptr() if sim is not None else None
        guard.launch("ptt_xcorr_fused_fwd_f32", dev, ctypes.byref(d))
        torch.cuda.synchronize()
        check_guard(out)
        untouched_inputs(ins)
        got = logical(out).cpu().contiguous()
        bound("%s out=%s" % (name, lay), got, c.ref64, c.ref32, c.Y)
        if sim is not None:                                             # a copy of the cosine map in the reference's orientation
            check_guard(sim)
            same_bits(sim.cpu(), cos_t.transpose(1, 2).cpu(), name + ": sim_out")
            np.testing.assert_allclose(sim.cpu().numpy(), c.sim32.numpy(), **FR.TOL)
        first = got if first is None else first
        same_bits(got, first, "%s: layout %s against the first run" % (name, lay))


@pytest.mark.parametrize("B,Ns,Nt,C,widths", FR.XCORR_SPLIT)
def test_xcorr_split(dev, B, Ns, Nt, C, widths):
    c = FR.xcorr_case(B, Ns, Nt, C, widths)
    ins, o = xcorr_inputs(c, dev, folded0=True)
    sfe = put(c.sf.transpose(1, 2), dev, ld=C + 4, col_off=4, batch_stride=Ns * (C + 4) + 8)        # (B,Ns,C): unit channel stride
    tfe = put(c.tf.transpose(1, 2), dev, ld=C + 8, col_off=4, batch_stride=Nt * (C + 8) + 4)
    ins += [sfe, tfe]
    first = None
    name = "xcorr split (%d,%d,%d,%d)" % (B, Ns, Nt, C)
    for lay in "AABC":
        out, strides, logical = out_view(dev, lay, B, Ns, widths[-1], planes=2, plane_gap=32)
        d = xcorr_desc(c, o, out, strides)
        d.split, d.out_sh = 1, out.stride(0)
        assert d.out_sh > B * Ns * widths[-1]
        d.search_feat, d.templ_feat = sfe.data_ptr(), tfe.data_ptr()
        d.s_sb, d.s_sn, d.t_sb, d.t_sn = sfe.stride(0), sfe.stride(1), tfe.stride(0), tfe.stride(1)
        d.C, d.eps = C, 1e-8
        guard.launch("ptt_xcorr_fused_fwd_f32", dev, ctypes.byref(d))
        torch.cuda.synchronize()
        check_guard(out)                                                # both halves behind one guard
        untouched_inputs(ins)
        halves = logical(out).cpu()
        got = torch.maximum(halves[:B], halves[B:]).contiguous()
        bound("%s out=%s" % (name, lay), got, c.ref64, c.ref32, c.Y)
        first = got if first is None else first
        same_bits(got, first, "%s: layout %s against the first run" % (name, lay))


@pytest.mark.parametrize("B,C,Ns,Nt", FR.COS_CASES)
def test_cos_map(dev, B, C, Ns, Nt):
    c = FR.cos_case(B, C, Ns, Nt)
    # (d) does not hold across the two feature layouts here, and only the bound is kept: cos_map_kernel sums the channels in
    # two loops of its own, `for (int c = 0; c < q.C; c += 4) { ... for (int k = 0; k < 4; ++k) { dot += av[k] * sv[k]; ...`
    # when `q.t_sc == 1 && q.s_sc == 1 && (q.C & 3) == 0 && ...` and `for (int c = 0; c < q.C; ++c) { ... dot += av * sv; ...`
    # otherwise: two reductions the compiler schedules and contracts independently. Measured on MI355X: the two layouts differ
    # in the last bits of small cosines (a few ulp of values near 0.01) at the same err / Y. Each form is run twice and must
    # repeat its own bits.
    first = {}
    for lay in ("point", "point", "channel", "channel"):
        if lay == "point":      # unit channel stride, C % 4 == 0, aligned rows: the float4 loop of cos_map_kernel
            sfe = put(c.sf.transpose(1, 2), dev, ld=C + 4, col_off=4, batch_stride=Ns * (C + 4) + 8)
            tfe = put(c.tf.transpose(1, 2), dev, ld=C + 8, col_off=4, batch_stride=Nt * (C + 8) + 4)
            ss, ts = (sfe.stride(0), sfe.stride(1), 1), (tfe.stride(0), tfe.stride(1), 1)              # (sb, sn, sc)
        else:                   # channel-major with an odd row stride: the scalar loop (same sums in the same order)
            sfe, tfe = put(c.sf, dev, ld=Ns + 1 + Ns % 2), put(c.tf, dev, ld=Nt + 1 + Nt % 2)
            ss, ts = (sfe.stride(0), 1, sfe.stride(1)), (tfe.stride(0), 1, tfe.stride(1))
        out = guarded((B, Ns, Nt), F32, device=dev)
        guard.launch("ptt_cosine_map_f32", dev, sfe.data_ptr(), ss[0], ss[1], ss[2], tfe.data_ptr(), ts[0], ts[1], ts[2], B, Ns, Nt, C,
                     1e-8, out.data_ptr())
        torch.cuda.synchronize()
        check_guard(out)
        untouched_inputs([sfe, tfe])
        got = out.cpu().contiguous()
        name = "cos (%d,%d,%d,%d) %s" % (B, C, Ns, Nt, lay)
        r = note(name, FR.rel_err(got, c.ref64), c.Y)
        assert r <= R_RATIO, name
        np.testing.assert_allclose(got.numpy(), c.ref32.numpy(), atol=2e-6, rtol=1e-5)      # tests/test_dense_gpu.py:203
        assert float(got[0, :, 0].abs().max()) == 0.0                                       # the all-zero template row
        same_bits(got, first.setdefault(lay, got), name + " against the first run of this form")


# =========================================================================================================== pair kernel
def pair_run(dev, c, w, qkv_e, xyz_e, knn_e, ins, heads, rel, order, want_attn):
    B, N, D, k = c.B, c.N, FR.D_MODEL, FR.KNN
    res = guarded((B, N, D), F32, device=dev)
    attn = None
    if want_attn:
        attn = guarded((B, N * k, D) if heads == 1 else (B * heads, N * k, D // heads), F32, device=dev)
    d = ops.AttnDesc()
    d.xyz, d.knn, d.qkv = xyz_e.data_ptr(), knn_e.data_ptr(), qkv_e.data_ptr()
    d.rel = rel.data_ptr() if rel is not None else None
    d.order = order.data_ptr() if order is not None else None
    for f in ("Wd1p", "Wd2p", "bd2", "Wg1p", "bg1", "Wg2p", "bg2"):
        setattr(d, f, w[f].data_ptr())
    d.res, d.attn = res.data_ptr(), attn.data_ptr() if attn is not None else None
    d.B, d.N, d.k, d.D, d.heads = B, N, k, D, heads
    guard.launch("ptt_pt_attn_pair_f32", dev, ctypes.byref(d))
    torch.cuda.synchronize()
    check_guard(res)
    if attn is not None:
        check_guard(attn)
    untouched_inputs(ins + [v for v in (rel, order) if v is not None])
    return res, attn


@pytest.mark.parametrize("heads", FR.PAIR_HEADS)
@pytest.mark.parametrize("B,N", FR.PAIR_SHAPES)
def test_pair(dev, B, N, heads):
    c = FR.pair_case(B, N, heads)
    P, D, k = c.P, FR.D_MODEL, FR.KNN
    dv = lambda n: P[n].to(dev).contiguous()
    ins = []
    keep = lambda v: (ins.append(v), v)[1]
    xyz_d = c.xyz.to(dev)
    knn_d, rel_d = ops.knn(xyz_d, k, want_rel=True)
    assert torch.equal(knn_d.cpu(), c.knn), "the device kNN table is not the oracle's"
    order_d = ops.spatial_order(xyz_d)
    assert torch.equal(order_d.view(B, N).sort(dim=1)[0].cpu(), (torch.arange(B * N, dtype=I32).view(B, N)))    # a permutation inside clouds
    if heads == 1:
        x = ops.linear(c.feats.to(dev), ops.pack_weight(dv("fc1.weight")), D, None, dv("fc1.bias"))
        wqkv = torch.cat([P["w_qs.weight"], P["w_ks.weight"], P["w_vs.weight"]], 0).to(dev)
        qkv = ops.linear(x, ops.pack_weight(wqkv), 3 * D)
    else:
        qkv = c.qkv.to(dev)
    H = heads
    w = dict(Wd1p=ops.pack_delta0(dv("fc_delta.0.weight"), dv("fc_delta.0.bias")), Wd2p=ops.pack_weight(dv("fc_delta.2.weight")),
             bd2=dv("fc_delta.2.bias"), Wg1p=ops.pack_weight(dv("fc_gamma.0.weight")), bg1=dv("fc_gamma.0.bias").repeat(H).contiguous(),
             Wg2p=ops.pack_weight(dv("fc_gamma.2.weight")), bg2=dv("fc_gamma.2.bias").repeat(H).contiguous())
    w = {n: keep(embed(t)) for n, t in w.items()}
    qkv_e, xyz_e, knn_e = keep(embed(qkv.contiguous())), keep(embed(xyz_d)), keep(embed(knn_d))
    rel_e, order_e = embed(rel_d.view(B, N * k, 3).contiguous()), embed(order_d.view(B, N).contiguous())
    name = "pair (%d,%d) heads=%d" % (B, N, heads)

    def results(res, attn):
        if heads == 1:      # the block's output: fc2 + residual on the linear kernel, as tests/test_dense_gpu.py chains it
            out = ops.linear(res, ops.pack_weight(dv("fc2.weight")), 256, None, dv("fc2.bias"), False, c.feats.to(dev))
            return out.cpu(), (attn.view(B, N, k, D).cpu() if attn is not None else None)
        return res.cpu().contiguous(), (attn.view(B * H, N, k, D // H).cpu() if attn is not None else None)

    first = None
    for use_rel in (False, True):
        for use_order in (False, True):
            tag = "%s rel=%d order=%d" % (name, use_rel, use_order)
            res, attn = pair_run(dev, c, w, qkv_e, xyz_e, knn_e, ins, heads, rel_e if use_rel else None, order_e if use_order else None, True)
            out_h, attn_h = results(res, attn)
            bound(tag + " res", out_h, c.res64, c.res32, c.Y_res)
            bound(tag + " attn", attn_h, c.attn64, c.attn32, c.Y_attn)
            res_bits = res.cpu().contiguous()
            # attn off must equal the res of attn on, bit for bit
            res_off, none = pair_run(dev, c, w, qkv_e, xyz_e, knn_e, ins, heads, rel_e if use_rel else None, order_e if use_order else None, False)
            assert none is None
            same_bits(res_off.cpu(), res_bits, tag + ": attn off against attn on")
            if first is None:
                first = (res_bits, attn_h)
                again, attn2 = pair_run(dev, c, w, qkv_e, xyz_e, knn_e, ins, heads, None, None, True)
                same_bits(again.cpu(), res_bits, tag + ": second run")
                same_bits(results(again, attn2)[1], attn_h, tag + ": second run, attn")
            if not use_rel:
                # ptt_attn_desc.order: "results do not depend on it" — which slot a point is worked on changes no arithmetic
                same_bits(res_bits, first[0], tag + ": res against order = NULL")
                same_bits(attn_h, first[1], tag + ": attn against order = NULL")


# ============================================================================================================= refusals
def _rand(dev, *shape):
    return torch.from_numpy(np.random.RandomState(sum(shape)).standard_normal(shape).astype(np.float32)).to(dev)


def test_refusal_pair_odd_n(dev):
    """Every array has the size the refused shape would need: were the launch not refused, it would run inside its buffers."""
    B, N, D, k = 1, 17, FR.D_MODEL, FR.KNN
    xyz = _rand(dev, B, N, 3)
    knn = ops.knn(xyz, k)
    res, attn = guarded((B, N, D), F32, device=dev), guarded((B, N * k, D), F32, device=dev)
    qkv, wsq, wd1, bias = _rand(dev, B, N, 3 * D), ops.pack_weight(_rand(dev, D, D)), ops.pack_weight(_rand(dev, D, 4)), _rand(dev, D)
    d = ops.AttnDesc()
    d.xyz, d.knn, d.qkv = xyz.data_ptr(), knn.data_ptr(), qkv.data_ptr()
    d.Wd1p, d.Wd2p, d.bd2 = wd1.data_ptr(), wsq.data_ptr(), bias.data_ptr()
    d.Wg1p, d.bg1, d.Wg2p, d.bg2 = wsq.data_ptr(), bias.data_ptr(), wsq.data_ptr(), bias.data_ptr()
    d.res, d.attn = res.data_ptr(), attn.data_ptr()
    d.B, d.N, d.k, d.D, d.heads = B, N, k, D, 1
    refused("pair_odd_N", lambda: guard.launch("ptt_pt_attn_pair_f32", dev, ctypes.byref(d)), res, attn)


def test_refusal_xcorr(dev):
    # Nt = 65, plain form
    B, Ns, Nt, C0 = 1, 3, 65, 8
    layers = fold(FR.xcorr_layers(3, 4, [C0, 32, 64])[1:], dev, True)
    P, cos, wsim = _rand(dev, B, Nt, C0), _rand(dev, B, Ns, Nt), _rand(dev, C0)
    out, sim = guarded((B, Ns, 64), F32, device=dev), guarded((B, Nt, Ns), F32, device=dev)
    d = ops.XcorrDesc()
    d.P, d.w_sim, d.cos_t, d.out, d.sim_out = P.data_ptr(), wsim.data_ptr(), cos.data_ptr(), out.data_ptr(), sim.data_ptr()
    d.out_sb, d.out_sc, d.out_sn = Ns * 64, 1, 64
    d.B, d.Ns, d.Nt, d.C0 = B, Ns, Nt, C0
    fill_layers(d, layers)
    refused("xcorr_Nt_65", lambda: guard.launch("ptt_xcorr_fused_fwd_f32", dev, ctypes.byref(d)), out, sim)
    # the split form with B * Ns % 8 != 0
    B, Ns, Nt, C = 1, 3, 64, 20
    P, sf, tf = _rand(dev, B, Nt, C0), _rand(dev, B, Ns, C), _rand(dev, B, Nt, C)
    out = guarded((2, B * Ns, 64), F32, batch_stride=B * Ns * 64 + 32, device=dev)
    d = ops.XcorrDesc()
    d.P, d.w_sim, d.out = P.data_ptr(), wsim.data_ptr(), out.data_ptr()
    d.out_sb, d.out_sc, d.out_sn = Ns * 64, 1, 64
    d.B, d.Ns, d.Nt, d.C0 = B, Ns, Nt, C0
    d.split, d.out_sh = 1, out.stride(0)
    d.search_feat, d.templ_feat, d.s_sb, d.s_sn, d.t_sb, d.t_sn, d.C, d.eps = sf.data_ptr(), tf.data_ptr(), Ns * C, C, Nt * C, C, C, 1e-8
    fill_layers(d, layers)
    refused("xcorr_split_BNs", lambda: guard.launch("ptt_xcorr_fused_fwd_f32", dev, ctypes.byref(d)), out)


def _sa_desc(dev, c, s, out, strides, ns=None, idx=None):
    d = ops.SaDesc()
    d.xyz, d.new_xyz, d.idx = s.xyz.data_ptr(), s.new_xyz.data_ptr(), (idx if idx is not None else s.idx).data_ptr()
    d.out, (d.out_sb, d.out_sc, d.out_sm) = out.data_ptr(), strides
    d.B, d.N, d.M, d.nsample = c.B, c.N, c.M, ns or c.ns
    d.radius, d.use_xyz, d.normalize_xyz = float(c.radius), 1, 1
    fill_layers(d, s.layers)
    return d


def test_refusal_sa(dev):
    c = FR.sa_case("lds4_111")
    s = SaInputs(c, dev, "none")
    # nsample = 8
    out, strides, _ = out_view(dev, "A", c.B, c.M, 128)
    idx8 = c.idx[..., :8].contiguous().to(dev)
    d = _sa_desc(dev, c, s, out, strides, ns=8, idx=idx8)
    refused("sa_nsample_8", lambda: guard.launch("ptt_sa_fused_fwd_f32", dev, ctypes.byref(d)), out)
    # a layer with Cout = 48
    from tests.util import fold_layers, mlp_layers
    s48 = SaInputs(c, dev, "none")
    s48.layers = embed_layers(fold_layers(mlp_layers(1, [3, 64, 48]), dev, ops, True), s48.ins)
    out, strides, _ = out_view(dev, "A", c.B, c.M, 48)
    d = _sa_desc(dev, c, s48, out, strides)
    refused("sa_Cout_48", lambda: guard.launch("ptt_sa_fused_fwd_f32", dev, ctypes.byref(d)), out)


@pytest.mark.parametrize("name", ["lds4_111", "stream_33"])
def test_refusal_compact_workspace(dev, name):
    c = FR.sa_case(name)
    s = SaInputs(c, dev, "none")
    n = int(ops._host("ptt_sa_compact_workspace", c.B, c.M))
    for what, off, nbytes in (("compact_ws_short", 0, n - 4), ("compact_ws_align", 4, n)):
        out, strides, _ = out_view(dev, "A", c.B, c.M, c.spec[-1])
        ws = guard.workspace(n + 16, device=dev)          # room for the shifted pointer: a launch that ran would stay inside
        d = _sa_desc(dev, c, s, out, strides)
        if c.hoist:
            d.l0_point_term, d.l0_xyz_weight, d.l0_channels, d.l0_relu = s.term.data_ptr(), s.wx.data_ptr(), c.spec[1], 1
        d.compact_ws, d.compact_ws_bytes = ws.data_ptr() + off, nbytes
        refused(what, lambda: guard.launch("ptt_sa_fused_fwd_f32", dev, ctypes.byref(d)), out, ws)


def test_zz_ratio_report():
    """Not a check of its own: the err / Y table of the run (pytest -s), the source of R and of the table above."""
    worst = RATIOS.report()
    assert worst <= R_RATIO
