"""The yardstick of tests/test_fused_guard_gpu.py is sound, checked without a GPU (tests/fused_ref.py).

For every case: 0 < e32 <= 2e-6 (a condition on the reference pair ref32 / ref64, not on code under test: a float64 run that is
not float64, or a float32 oracle that drifted, shows here), ref32 meets the existing 1e-4 contract against ref64, and the
case really has the ragged property it is listed for — B * M % (centres per wave / workgroup), tile counts and chunk
remainders recomputed from the dispatch constants of ptt_sa_fused_fwd_f32 (restated in fused_ref.sa_dispatch), so a later
change of a shape cannot silently make a case tile-aligned."""
import numpy as np
import pytest
import torch

from oracle import dense_ref as R
from tests import fused_ref as FR


def _pair_ok(ref32, ref64):
    e = FR.e32_of(ref32, ref64)
    assert ref64.dtype == torch.float64 and ref32.dtype == torch.float32
    assert 0.0 < e <= FR.E32_CAP, e
    np.testing.assert_allclose(ref32.numpy(), ref64.float().numpy(), **FR.TOL)
    return e


# what every SA case is listed for: (key of sa_dispatch's facts, expected value) pairs
RAGGED = {
    "lds4_1":      dict(total=1, nw=4, wgs=1, last_wg=1),                   # one centre: three of the four waves idle
    "lds4_111":    dict(total=111, nw=4, last_wg=3),                        # 111 = 27 * 4 + 3
    "lds12_1035":  dict(total=1035, nw=12, chunk=1, wgs=87, last_wg=3),     # 1035 * 3 > 3072: 12 waves; 1035 = 86 * 12 + 3
    "wave32_5":    dict(total=5, cpw=1, per_wg=4, wgs=2, last_wg=1),
    "wave16_18":   dict(total=18, cpw=2, per_wg=8, wgs=3, last_wg=2),       # last workgroup: one full wave, three empty
    "wave16_21":   dict(total=21, cpw=2, per_wg=8, wgs=3, last_wg=5),       # last workgroup: waves of 2, 2 and ONE centre
    "stream_33":   dict(total=33, tiles=17, last_tile=1),
    "stream_1027": dict(total=1027, tiles=514, chunk=2, wgs=257, last_tile=1),    # wgs capped at 512 -> chunk 2; whole last chunk
    "stream_1029": dict(total=1029, tiles=515, chunk=2, wgs=258, last_chunk=1, last_tile=1),   # the short last chunk
    "fused32_33":  dict(total=33, cpw=2, last_wg=1),
    "fused16_21":  dict(total=21, cpw=4, last_wg=1),
    "fused16_21h": dict(total=21, cpw=4, last_wg=1),
    "fused64_10":  dict(total=10, cpw=1),                                   # nsample 64: one centre spans both row tiles
}


def test_every_sa_case_has_a_ragged_entry():
    assert set(RAGGED) == set(FR.SA_CASES)
    reached = {c[9] for c in FR.SA_CASES.values()}
    assert reached == {"sa_lds_kernel/4", "sa_lds_kernel/12", "sa_wave_kernel<32,1>", "sa_wave_kernel<16,1>", "sa_stream_kernel<32>",
                       "sa_fused_kernel<32,2>", "sa_fused_kernel<16,2>", "sa_fused_kernel<64,2>"}
    assert sum(1 for c in FR.SA_CASES.values() if c[10]) >= 5           # compact: sa_lds_kernel<true>, sa_stream_compact_kernel


@pytest.mark.parametrize("name", list(FR.SA_CASES))
def test_sa_case(name):
    B, N, M, C, spec, radius, ns, siw, hoist, kernel, compact = FR.SA_CASES[name]
    got_kernel, facts = FR.sa_dispatch(B, M, C, spec, ns, siw, hoist)
    assert got_kernel == kernel
    for k, v in RAGGED[name].items():
        assert facts[k] == v, (k, facts)
    if kernel.startswith(("sa_lds", "sa_wave", "sa_fused")) and name != "fused64_10":
        per = facts.get("per_wg", facts.get("cpw")) if not kernel.startswith("sa_lds") else facts["nw"] * facts["chunk"]
        assert facts["total"] % per != 0                                  # the last workgroup is partly filled
    if kernel.startswith("sa_wave_kernel<16"):
        assert facts["cpw"] == 2
    assert compact == kernel.startswith(("sa_lds", "sa_stream"))
    c = FR.sa_case(name)
    _pair_ok(c.ref32, c.ref64)
    assert tuple(c.ref64.shape) == (B, spec[-1], M)
    # under-filled balls (first-hit padding) and, with B >= 3, the all-zero cloud, as the existing cases have them
    idx = c.idx.numpy()
    padded = (idx[..., 1:] == idx[..., :1]).any(axis=-1)
    assert padded.any(), "no under-filled ball"
    if B >= 3:                           # every point of the all-zero cloud lies in every ball: slots 0 .. ns - 1
        assert float(c.xyz[2].abs().max()) == 0.0 and (idx[2] == np.arange(ns)).all()
    assert idx.min() >= 0 and idx.max() < N


def test_sa_ref64_is_the_oracle_sequence():
    """The float64 restatement run in float32 (same gather, same ops) gives the float32 oracle's bits: nothing but the
    dtype differs between ref32 and ref64."""
    c = FR.sa_case("fused16_21")
    import torch.nn.functional as F
    g = FR._sa_gather64(c.xyz.transpose(1, 2).contiguous(), c.idx) - c.new_xyz.transpose(1, 2).unsqueeze(-1)
    g = torch.cat([g / c.radius, FR._sa_gather64(c.feats, c.idx)], dim=1)
    again = F.max_pool2d(R.shared_mlp_eval(g, c.layers), kernel_size=[1, c.ns]).squeeze(-1)
    assert torch.equal(again, c.ref32)


@pytest.mark.parametrize("C0,B,Ns,Nt,nrem", FR.XCORR_PLAIN)
def test_xcorr_plain_case(C0, B, Ns, Nt, nrem):
    widths = FR.XCORR_WIDTHS[(C0, nrem)]
    assert widths[0] == C0 and len(widths) == nrem + 1 and C0 % 8 == 0 and Nt % 64 == 0
    assert all(w % 32 == 0 and w <= 256 for w in widths[1:])
    c = FR.xcorr_case(B, Ns, Nt, FR.XCORR_F, tuple(widths))
    _pair_ok(c.ref32, c.ref64)
    _pair_ok(c.sim32, c.sim64)
    assert float(c.tf[0, :, 0].abs().max()) == 0.0 and float(c.sim32[0, 0].abs().max()) == 0.0
    assert tuple(c.ref64.shape) == (B, widths[-1], Ns)


@pytest.mark.parametrize("B,Ns,Nt,C,widths", FR.XCORR_SPLIT)
def test_xcorr_split_case(B, Ns, Nt, C, widths):
    assert (B * Ns) % 8 == 0 and C % 4 == 0 and Nt % 64 == 0
    c = FR.xcorr_case(B, Ns, Nt, C, widths)
    _pair_ok(c.ref32, c.ref64)


def test_xcorr_core_is_cosine_sim_aug_cut_before_the_convolutions():
    """xcorr_core followed by the trailing convolutions is dense_ref.cosine_sim_aug, bit for bit."""
    import torch.nn.functional as F
    from tests.util import cosine_sim_params
    mlp, conv = cosine_sim_params(5)
    rs = np.random.RandomState(5)
    sf = torch.from_numpy(rs.standard_normal((2, 256, 3)).astype(np.float32))
    tf = torch.from_numpy(rs.standard_normal((2, 256, 64)).astype(np.float32))
    txyz = torch.from_numpy(rs.uniform(-2, 2, (2, 64, 3)).astype(np.float32))
    want, sim = R.cosine_sim_aug(sf, tf, txyz, mlp, conv)
    pooled, sim2 = FR.xcorr_core(sf, tf, txyz, mlp)
    y = F.conv1d(pooled, conv["conv0_weight"])
    y = F.relu(F.batch_norm(y, conv["bn0_mean"], conv["bn0_var"], conv["bn0_weight"], conv["bn0_bias"], False, 0.0, 1e-5))
    y = F.conv1d(y, conv["conv1_weight"], conv["conv1_bias"])
    assert torch.equal(y, want) and torch.equal(sim, sim2)


@pytest.mark.parametrize("B,C,Ns,Nt", FR.COS_CASES)
def test_cos_case(B, C, Ns, Nt):
    c = FR.cos_case(B, C, Ns, Nt)
    _pair_ok(c.ref32, c.ref64)
    assert (B * Ns) % 4 != 0            # cos_map_kernel: four search points per workgroup, the last one partly filled
    assert Nt % 64 != 0                 # and a wave's last pass over the template points partly masked


@pytest.mark.parametrize("heads", FR.PAIR_HEADS)
@pytest.mark.parametrize("B,N", FR.PAIR_SHAPES)
def test_pair_case(B, N, heads):
    c = FR.pair_case(B, N, heads)
    _pair_ok(c.res32, c.res64)
    _pair_ok(c.attn32, c.attn64)
    assert N % 2 == 0 and N >= FR.KNN
    assert tuple(c.attn64.shape) == ((B, N, FR.KNN, FR.D_MODEL) if heads == 1 else (B * heads, N, FR.KNN, FR.D_MODEL // heads))
    knn = c.knn.numpy()
    assert knn.min() >= 0 and knn.max() < N
    if N == FR.KNN:                      # N = k: every point's neighbours are the whole cloud
        assert (np.sort(knn, axis=-1) == np.arange(N)).all()


def test_heads_attention_with_one_head_is_the_transformer_block():
    """fused_ref.heads_attention (the multi-head reference) at heads = 1 reproduces dense_ref.transformer_block's attention."""
    import torch.nn.functional as F
    c = FR.pair_case(1, 16, 1)
    P = c.P
    x = F.linear(c.feats, P["fc1.weight"], P["fc1.bias"])
    qkv = F.linear(x, torch.cat([P["w_qs.weight"], P["w_ks.weight"], P["w_vs.weight"]], 0))
    res, attn = FR.heads_attention(c.xyz, qkv, c.knn, P, 1)
    np.testing.assert_allclose(attn.numpy(), c.attn32.numpy(), atol=1e-6, rtol=1e-5)
    out = F.linear(res, P["fc2.weight"], P["fc2.bias"]) + c.feats
    np.testing.assert_allclose(out.numpy(), c.res32.numpy(), atol=1e-5, rtol=1e-5)
