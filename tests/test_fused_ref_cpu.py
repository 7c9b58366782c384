"""The yardstick of tests/test_fused_guard_gpu.py is sound, checked without a GPU (tests/fused_ref.py).

For every case: 0 < e32 <= 2e-6 (a condition on the reference pair ref32 / ref64, not on code under test: a float64 run that is
not float64, or a float32 oracle that drifted, shows here), ref32 meets the existing 1e-4 contract against ref64, and the
case really has the ragged property it is listed for — B * M % (centres per wave / workgroup), tile counts and chunk
remainders recomputed from the dispatch constants of ptt_sa_fused_fwd_f32 (restated in fused_ref.sa_dispatch), so a later
change of a shape cannot silently make a case tile-aligned. For the option cases of tests/test_sa_options_gpu.py it checks, on
top of that, that their inputs discriminate: the reference moves when a flag the case varies is flipped (see the end of the file)."""
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


# ================================================================================================== the SA option cases
# Conditions on the INPUTS of tests/test_sa_options_gpu.py, not measurements of code under test: an option case whose reference
# does not move when its flag is flipped would pass with the flag ignored. A case that misses one changes its radius or seed
# (fused_ref.SA_OPTION_CASES); the conditions are not lowered.
FLIP_SHARE, FLIP_TOL = 0.20, 1e-2           # >= 20 % of the outputs move by more than 1e-2 * (1 + |ref|): 100 x the 1e-4 contract
NEG_SHARE, NEG_BELOW = 0.10, -1e-3          # a ReLU-less last layer: >= 10 % of the outputs below -1e-3
FULL_CASES, FULL_SHARE = 4, 0.10            # >= 4 cases with >= 10 % balls of ns distinct neighbours
# the cases an inner ReLU-less layer moves to another kernel; every other case reaches its shape's kernel
OPTION_KERNEL = {"inner0_lds4_111": "sa_wave_kernel<32,1>", "inner1_lds4_111": "sa_wave_kernel<32,1>",
                 "inner1_lds12_1035": "sa_wave_kernel<32,1>", "inner0_stream_33": "sa_fused_kernel<32,2>"}


def test_cube_clouds():
    s = FR.cube_clouds(7, 4, 50)
    assert s.dtype == np.float32 and s.shape == (4, 50, 3) and s.min() >= 0.0 and s.max() < 1.0
    assert (s[1] == s[0]).all() and (s[3] == 0).all() and (s[2] != 0).any() and not (s[2] == s[0]).all()
    assert len(np.unique(s[0], axis=0)) == 50                       # distinct points
    two = FR.cube_clouds(7, 2, 50)
    assert (two[1] != two[0]).any() and (two[1] != 0).any()         # B < 3: neither edge
    assert (FR.cube_clouds(7, 4, 50) == s).all() and (FR.cube_clouds(8, 4, 50)[0] != s[0]).any()


def test_sa_dispatch_reads_the_flags_the_c_dispatch_reads():
    lds = (3, 37, 0, FR.SPEC0, 32, True, False)
    assert FR.sa_dispatch(*lds)[0] == "sa_lds_kernel/4"
    assert FR.sa_dispatch(*lds, relu0=False)[0] == FR.sa_dispatch(*lds, relu1=False)[0] == "sa_wave_kernel<32,1>"
    stream = (1, 33, 128, FR.SPEC1, 32, True, True)
    assert FR.sa_dispatch(*stream)[0] == "sa_stream_kernel<32>"
    assert FR.sa_dispatch(*stream, relu0=False)[0] == "sa_fused_kernel<32,2>"
    assert FR.sa_dispatch(*stream, relu1=False)[0] == "sa_stream_kernel<32>"        # the last layer's flag is not read
    # use_xyz off needs C > 0, which the lds shape excludes by itself; the flag is restated all the same
    assert FR.sa_dispatch(3, 37, 0, FR.SPEC0, 32, True, False, use_xyz=False)[0] != "sa_lds_kernel/4"


def test_sa_option_cases_cover_the_shapes_and_the_families():
    shapes = {v[0] for v in FR.SA_OPTION_CASES.values()}
    assert shapes == set(FR.SA_CASES)                               # the 13 shapes, each with at least one option set
    fam = lambda k: k.split("<")[0].split("/")[0] + ("" if "fused" not in k and "wave" not in k else k[k.index("<"):k.index(",")])
    reached = {}
    for name in FR.SA_OPTION_CASES:
        c = FR.sa_option_case(name)
        reached.setdefault(name.split("_")[0], set()).add(fam(c.kernel) + ("+compact" if c.compact else ""))
    assert reached["norm0"] == {"sa_lds_kernel+compact", "sa_wave_kernel<16", "sa_wave_kernel<32", "sa_stream_kernel+compact",
                                "sa_fused_kernel<16", "sa_fused_kernel<32", "sa_fused_kernel<64"}
    assert reached["noxyz"] == {"sa_wave_kernel<16", "sa_fused_kernel<16", "sa_fused_kernel<32", "sa_fused_kernel<64"}
    assert reached["last0"] == {"sa_lds_kernel+compact", "sa_wave_kernel<16", "sa_stream_kernel+compact", "sa_fused_kernel<16",
                                "sa_fused_kernel<32", "sa_fused_kernel<64"}
    assert reached["inner0"] == {"sa_wave_kernel<32", "sa_fused_kernel<32"}         # L[0].relu of the lds and the stream shape
    assert reached["inner1"] == {"sa_wave_kernel<32", "sa_fused_kernel<32"}         # L[1].relu of the lds shape; the fused kernel's middle layer
    assert not FR.sa_option_case("inner1_fused32_33").hoist and FR.sa_option_case("inner0_stream_33").hoist
    assert reached["l0relu0"] == {"sa_stream_kernel+compact", "sa_fused_kernel<16"}
    assert reached["none"] == {"sa_wave_kernel<16", "sa_fused_kernel<16"}
    assert reached["bn0"] == {"sa_wave_kernel<32", "sa_fused_kernel<32", "sa_lds_kernel+compact", "sa_stream_kernel+compact"}
    full = [n for n in FR.SA_OPTION_CASES if FR.distinct_full_share(FR.sa_option_case(n)) >= FULL_SHARE]
    assert len(full) >= FULL_CASES, full


@pytest.mark.parametrize("name", list(FR.SA_OPTION_CASES))
def test_sa_option_case(name):
    c = FR.sa_option_case(name)
    shape = FR.SA_CASES[c.shape]
    assert (c.B, c.N, c.M, c.C, c.ns, c.hoist) == (shape[0], shape[1], shape[2], shape[3], shape[6], shape[8])
    assert c.kernel == OPTION_KERNEL.get(name, shape[9])
    assert c.spec[0] == (3 if c.use_xyz else 0) + c.C == c.layers[0]["conv_weight"].shape[1]
    _pair_ok(c.ref32, c.ref64)
    assert tuple(c.ref64.shape) == (c.B, c.spec[-1], c.M)
    # the clouds: distinct points, and with B >= 3 the repeated cloud and the all-zero one
    idx = c.idx.numpy()
    assert idx.min() >= 0 and idx.max() < c.N
    assert len(np.unique(c.xyz[0].numpy(), axis=0)) == c.N
    if c.B >= 3:
        assert torch.equal(c.xyz[1], c.xyz[0]) and (idx[1] == idx[0]).all()
        assert float(c.xyz[-1].abs().max()) == 0.0 and (idx[-1] == np.arange(c.ns)).all()
    # every flag the case varies moves the reference
    flips = FR.option_flips(c)
    varied = {k for k, on in (("normalize_xyz", not c.normalize_xyz), ("use_xyz", not c.use_xyz)) if on}
    varied |= {"relu[%d]" % l for l, on in enumerate(c.relu) if not on}
    assert varied <= set(flips) and (flips or any(f != "bn" for f in c.forms)), "the case varies nothing"
    for flag, kw in flips.items():
        other = FR.option_ref(c, **kw)
        share = float(((other - c.ref64).abs() > FLIP_TOL * (1 + c.ref64.abs())).double().mean())
        assert share >= FLIP_SHARE, (flag, share)
    if not c.relu[-1]:
        assert float((c.ref64 < NEG_BELOW).double().mean()) >= NEG_SHARE
    # the forms are what they are named for
    for L, form in zip(c.layers, c.forms):
        scale, shift = FR.layer_affine(L)
        assert (scale is not None) == (form in ("bn", "bn0")) and (shift is not None) == (form in ("bn", "bias"))
        if form == "bn0":
            assert float((L["bn_bias"] - L["bn_mean"] * scale).abs().max()) == 0.0


@pytest.mark.parametrize("use_xyz,normalize", [(True, True), (True, False), (False, True), (False, False)])
def test_sa_ref_float32_twin_is_the_oracle_sequence(use_xyz, normalize):
    """fused_ref.sa_ref in float32 gives the bits of oracle.dense_ref.query_and_group(..., use_xyz, normalize_xyz) +
    shared_mlp_eval + max-pool for every grouping option; its float64 run differs in the dtype alone."""
    import torch.nn.functional as F
    c = FR.sa_option_case("noxyz_wave16_18" if not use_xyz else "norm0_wave16_21")
    grouped, _, idx = R.query_and_group(c.xyz, c.new_xyz, c.feats, c.radius, c.ns, use_xyz, normalize)
    assert torch.equal(idx, c.idx)
    want = F.max_pool2d(R.shared_mlp_eval(grouped, c.layers), kernel_size=[1, c.ns]).squeeze(-1)
    got = FR.sa_ref(c.xyz, c.new_xyz, c.feats, c.idx, c.layers, c.radius, c.ns, use_xyz, normalize, dtype=torch.float32)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    r64 = FR.sa_ref64(c.xyz, c.new_xyz, c.feats, c.idx, c.layers, c.radius, c.ns, use_xyz, normalize)
    assert r64.dtype == torch.float64 and 0.0 < FR.e32_of(got, r64) <= FR.E32_CAP


def test_sa_ref_options():
    """relu flags, l0_relu and the BatchNorm-less forms against their definitions, written out once more in float64."""
    import torch.nn.functional as F
    c = FR.sa_option_case("none_fused16_21")                        # forms none, bias, none
    L = FR.double_layers(c.layers)
    g = FR._sa_gather64(c.xyz.double().transpose(1, 2).contiguous(), c.idx) - c.new_xyz.double().transpose(1, 2).unsqueeze(-1)
    g = torch.cat([g / float(np.float32(c.radius)), FR._sa_gather64(c.feats.double(), c.idx)], dim=1)
    h0 = F.conv2d(g, L[0]["conv_weight"])
    for relu in ((True, True, True), (False, True, True), (True, False, False)):
        h = F.relu(h0) if relu[0] else h0
        h = F.conv2d(h, L[1]["conv_weight"]) + L[1]["conv_bias"].view(1, -1, 1, 1)
        h = F.relu(h) if relu[1] else h
        h = F.conv2d(h, L[2]["conv_weight"])
        h = (F.relu(h) if relu[2] else h).max(dim=3)[0]
        got = FR.option_ref(c, relu=relu)
        assert float((got - h).abs().max()) <= 1e-12 * float(h.abs().max())
        assert torch.equal(FR.option_ref(c, relu=(True,) + relu[1:], l0_relu=relu[0]), got)
    with pytest.raises(ValueError):
        FR.sa_ref(c.xyz, c.new_xyz, None, c.idx, c.layers, c.radius, c.ns, use_xyz=False)


def test_sa_ref64_defaults_are_the_reference_the_guard_cases_were_measured_against():
    """With no option given, sa_ref64 is the expression it was before it took options — oracle.dense_ref.shared_mlp_eval on the
    .double() layers, rel / float32(radius) — bit for bit: the yardsticks of tests/test_fused_guard_gpu.py have not moved."""
    import torch.nn.functional as F
    for name in ("lds4_111", "fused16_21"):
        c = FR.sa_case(name)
        g = FR._sa_gather64(c.xyz.double().transpose(1, 2).contiguous(), c.idx) - c.new_xyz.double().transpose(1, 2).unsqueeze(-1)
        g = g / float(np.float32(c.radius))
        if c.feats is not None:
            g = torch.cat([g, FR._sa_gather64(c.feats.double(), c.idx)], dim=1)
        old = F.max_pool2d(R.shared_mlp_eval(g, FR.double_layers(c.layers)), kernel_size=[1, c.ns]).squeeze(-1)
        assert torch.equal(FR.sa_ref64(c.xyz, c.new_xyz, c.feats, c.idx, c.layers, c.radius, c.ns), old) and torch.equal(c.ref64, old)
