"""Case builders and the float64 yardstick for the fused eval-mode kernels (ptt_sa_fused_fwd_f32, ptt_xcorr_fused_fwd_f32,
ptt_cosine_map_f32, ptt_pt_attn_pair_f32). A plain module: no fixtures, no pytest settings, importable on the CPU.

Every case is built as tests/test_dense_gpu.py builds its inputs (synth.frames with one all-zero cloud when B >= 3,
tests.util.mlp_layers / transformer_params / cosine_sim_params-style weights, seeds derived from the shape) and carries

    the index table   idx / knn from the float32 oracle (oracle.index_ops); the device tables are pinned to these bit for bit
    ref32             the float32 oracle result (oracle.dense_ref)
    ref64             the same op sequence in float64 on the same index table: inputs and weights cast with .double(), the
                      gather written with torch.gather, nothing else changed. (The radius a float32 kernel divides by is
                      the float32 value of `radius`; its .double() is what the float64 run divides by.)

The yardstick of a case is Y = max(e32, 4u), e32 = max|ref32 - ref64| / max|ref64|, u = 2**-24: how far a correct float32
evaluation of the op lies from the float64 one. The floor 4u is there because a maximum over a handful of outputs is
dominated by the rounding of the final store (the one-centre case measures 7e-8, about one ulp). tests/test_fused_ref_cpu.py
checks the pair (0 < e32 <= 2e-6) and the ragged property every case is listed for; tests/test_fused_guard_gpu.py holds the
kernels to R * Y.

The set-abstraction reference takes every option of ptt_sa_desc (sa_ref: use_xyz, normalize_xyz, per-layer ReLU, l0_relu,
layers without BatchNorm) in float64 and in float32, and SA_OPTION_CASES puts the shapes of SA_CASES on clouds whose balls hold
distinct points (cube_clouds) with one option set each: tests/test_sa_options_gpu.py, tests/test_sa_module_options_gpu.py.

Cases are built once per process (functools.lru_cache) and shared; nothing mutates them."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import dense_ref as R
from oracle import index_ops as O
from ptt_amd import synth
from tests.util import mlp_layers, transformer_params

U = 2.0 ** -24
E32_CAP = 2e-6              # a condition on the reference pair, not on code under test: every shape here measures <= 6.1e-7
TOL = dict(atol=1e-4, rtol=1e-4)        # the existing contract of tests/test_dense_gpu.py


def e32_of(ref32, ref64):
    return float((ref32.double() - ref64).abs().max() / ref64.abs().max())


def yardstick(ref32, ref64):
    return max(e32_of(ref32, ref64), 4 * U)


def rel_err(got, ref64):
    """max|got - ref64| / max|ref64| of a float32 result (any device) against the float64 reference."""
    return float((got.detach().cpu().double() - ref64).abs().max() / ref64.abs().max())


def double_layers(layers):
    return [{k: (v.double() if torch.is_tensor(v) else v) for k, v in L.items()} for L in layers]


# ------------------------------------------------------------------------------------------------------------ set abstraction
# Constants of the dispatch in ptt_sa_fused_fwd_f32 (ptt_amd/csrc/mfma_ops.hip) the ragged properties are recomputed from.
SAL_WAVES = 12              # PTT_SAL_WAVES: waves per sa_lds_kernel workgroup of a full launch
SAL_DEVICE_WAVES = 256 * SAL_WAVES      # `waves`: resident waves of the device (PTT_SAL_WGS = 1)
SAL_CHUNK_MAX = 2           # dev_switches().sa_lds_chunk
STREAM_MAX_WGS = 512        # sa_stream_kernel: 2 workgroups per CU x 256 CUs
STREAM_CHUNK_MAX = 2        # dev_switches().sa_chunk

SPEC0 = [3, 64, 64, 128]
SPEC1 = [131, 128, 128, 256]
SPEC3 = [260, 256, 256, 256]

# id -> (B, N, M, C, spec, radius, ns, scale_in_weights, hoisted layer 0, kernel reached, compact_ws honoured)
SA_CASES = {
    "lds4_1":      (1, 64, 1, 0, SPEC0, 0.3, 32, True, False, "sa_lds_kernel/4", True),
    "lds4_111":    (3, 96, 37, 0, SPEC0, 0.3, 32, True, False, "sa_lds_kernel/4", True),
    "lds12_1035":  (5, 512, 207, 0, SPEC0, 0.3, 32, True, False, "sa_lds_kernel/12", True),
    "wave32_5":    (1, 64, 5, 0, SPEC0, 0.3, 32, False, False, "sa_wave_kernel<32,1>", False),
    "wave16_18":   (2, 80, 9, 5, [8, 32, 64], 0.4, 16, False, False, "sa_wave_kernel<16,1>", False),
    "wave16_21":   (3, 80, 7, 5, [8, 32, 64], 0.4, 16, True, False, "sa_wave_kernel<16,1>", False),
    "stream_33":   (1, 128, 33, 128, SPEC1, 0.5, 32, True, True, "sa_stream_kernel<32>", True),
    "stream_1027": (13, 128, 79, 128, SPEC1, 0.5, 32, True, True, "sa_stream_kernel<32>", True),
    "stream_1029": (21, 128, 49, 128, SPEC1, 0.5, 32, True, True, "sa_stream_kernel<32>", True),
    "fused32_33":  (1, 128, 33, 128, SPEC1, 0.5, 32, False, False, "sa_fused_kernel<32,2>", False),
    "fused16_21":  (3, 64, 7, 257, SPEC3, 0.3, 16, False, False, "sa_fused_kernel<16,2>", False),
    "fused16_21h": (3, 64, 7, 257, SPEC3, 0.3, 16, True, True, "sa_fused_kernel<16,2>", False),
    "fused64_10":  (2, 70, 5, 12, [15, 64, 128], 0.6, 64, False, False, "sa_fused_kernel<64,2>", False),
}


def sa_dispatch(B, M, C, spec, ns, scale_in_weights, hoisted, use_xyz=True, relu0=True, relu1=True):
    """The kernel ptt_sa_fused_fwd_f32 launches for a level, restated from its dispatch (mfma_ops.hip: the chain of `if`s
    after `const int total_centres = d->B * d->M;`) -> (name, facts about the launch's tiles). spec is the channel list of
    the whole SharedMLP (spec[0] = 3 * use_xyz + C); scale_in_weights: no layer the kernel runs carries a scale pointer;
    relu0 / relu1: `L[0].relu` / `L[1].relu` of the layers the KERNEL runs (with a hoisted layer 0 those are layers 1 and 2 of
    the SharedMLP) — the only activation flags the dispatch reads."""
    total = B * M
    louts = spec[1:]
    if C == 0 and use_xyz and not hoisted and ns == 32 and louts == [64, 64, 128] and scale_in_weights and relu0 and relu1:
        chunk = min(-(-total // SAL_DEVICE_WAVES), SAL_CHUNK_MAX)
        nw = 4 if total * 3 <= SAL_DEVICE_WAVES else SAL_WAVES
        wgs = -(-total // (chunk * nw))
        return "sa_lds_kernel/%d" % nw, dict(total=total, nw=nw, chunk=chunk, wgs=wgs, last_wg=total - (wgs - 1) * chunk * nw)
    rem = louts[1:] if hoisted else louts            # the layers the kernel itself runs
    cins = (spec[1:-1] if hoisted else spec[:-1])
    wbytes = sum(ci * co * 4 for ci, co in zip(cins, rem))
    if all(co // 32 in (1, 2, 4) for co in rem) and wbytes <= 64 * 1024 and ns <= 32:
        cpw = 32 // ns
        per_wg = 4 * cpw
        wgs = -(-total // per_wg)
        return "sa_wave_kernel<%d,1>" % ns, dict(total=total, cpw=cpw, per_wg=per_wg, wgs=wgs, last_wg=total - (wgs - 1) * per_wg)
    if hoisted and spec[1] == 128 and ns == 32 and rem == [128, 256] and scale_in_weights and relu0:
        tiles = (total + 1) // 2
        wgs = min(tiles, STREAM_MAX_WGS)
        chunk = min(-(-tiles // wgs), STREAM_CHUNK_MAX)
        wgs = -(-tiles // chunk)
        return "sa_stream_kernel<32>", dict(total=total, tiles=tiles, chunk=chunk, wgs=wgs, last_chunk=tiles - (wgs - 1) * chunk,
                                            last_tile=total - (tiles - 1) * 2)
    cpw = 64 // ns
    wgs = -(-total // cpw)
    return "sa_fused_kernel<%d,2>" % ns, dict(total=total, cpw=cpw, wgs=wgs, last_wg=total - (wgs - 1) * cpw)


class Case(dict):
    __getattr__ = dict.__getitem__


def _sa_gather64(t, idx):
    """(B,C,N) float64, idx (B,M,ns) -> (B,C,M,ns): QueryAndGroup's grouping as torch.gather."""
    B, M, ns = idx.shape
    flat = idx.long().reshape(B, 1, M * ns).expand(-1, t.shape[1], -1)
    return torch.gather(t, 2, flat).reshape(B, t.shape[1], M, ns)


def mlp_eval(x, layers, relu=None):
    """oracle.dense_ref.shared_mlp_eval (pytorch_utils.py:12-36) with the options of pt_utils.Conv2d spelled out: a layer
    dict without bn_* keys is a unit built with bn=False (its conv_bias, when present, is the convolution's bias), and
    relu[l] False a unit built with activation=None. relu=None on BatchNorm layers is shared_mlp_eval itself, op for op."""
    for l, L in enumerate(layers):
        x = F.conv2d(x, L["conv_weight"], L.get("conv_bias"))
        if "bn_weight" in L:
            x = F.batch_norm(x, L["bn_mean"], L["bn_var"], L["bn_weight"], L["bn_bias"], False, 0.0, L.get("eps", 1e-5))
        if relu is None or relu[l]:
            x = F.relu(x)
    return x


def sa_ref(xyz, new_xyz, feats, idx, layers, radius, ns, use_xyz=True, normalize_xyz=True, relu=None, l0_relu=None,
           dtype=torch.float64):
    """QueryAndGroup (pointnet2_utils.py:350-368: use_xyz, normalize_xyz) + SharedMLP in eval mode + max-pool on a fixed idx,
    in `dtype`: float64 is the reference, float32 its twin — the same ops on the same table, which is
    oracle.dense_ref.query_and_group + shared_mlp_eval bit for bit (tests/test_fused_ref_cpu.py). relu: one flag per layer
    (None = all on); l0_relu, when given, replaces relu[0] (ptt_sa_desc.l0_relu is layer 0's flag once that layer is hoisted).
    A float32 run divides by `radius` as torch divides a float32 tensor by a host scalar; the float64 run by its .double()."""
    cast = (lambda t: t.double()) if dtype == torch.float64 else (lambda t: t.float())
    x, c = cast(xyz), cast(new_xyz)
    g = _sa_gather64(x.transpose(1, 2).contiguous(), idx) - c.transpose(1, 2).unsqueeze(-1)
    if normalize_xyz:
        g = g / (float(np.float32(radius)) if dtype == torch.float64 else radius)
    if feats is not None:
        f = _sa_gather64(cast(feats), idx)
        g = torch.cat([g, f], dim=1) if use_xyz else f
    elif not use_xyz:
        raise ValueError("use_xyz = False without point features: nothing to group (pointnet2_utils.py:365-367)")
    if relu is not None or l0_relu is not None:
        relu = [True] * len(layers) if relu is None else list(relu)
        if l0_relu is not None:
            relu[0] = bool(l0_relu)
    lay = double_layers(layers) if dtype == torch.float64 else layers
    return F.max_pool2d(mlp_eval(g, lay, relu), kernel_size=[1, ns]).squeeze(-1)


def sa_ref64(xyz, new_xyz, feats, idx, layers, radius, ns, use_xyz=True, normalize_xyz=True, relu=None, l0_relu=None):
    """oracle.dense_ref.query_and_group (use_xyz, normalize_xyz) + shared_mlp_eval + max-pool in float64 on a fixed idx."""
    return sa_ref(xyz, new_xyz, feats, idx, layers, radius, ns, use_xyz, normalize_xyz, relu, l0_relu, torch.float64)


@functools.lru_cache(maxsize=None)
def sa_case(name):
    B, N, M, C, spec, radius, ns, siw, hoist, kernel, compact = SA_CASES[name]
    rs = np.random.RandomState(N + C)
    s, _ = synth.frames(N, B, N, 64, K_s=max(16, N // 2))
    if B >= 3:
        s[2] = 0.0
    xyz = torch.from_numpy(s)
    inds = torch.from_numpy(O.fps(s, M))
    new_xyz = torch.gather(xyz, 1, inds.long()[..., None].expand(-1, -1, 3)).contiguous()
    feats = torch.from_numpy(rs.standard_normal((B, C, N)).astype(np.float32)) if C else None
    layers = mlp_layers(N, spec)
    grouped, _, idx = R.query_and_group(xyz, new_xyz, feats, radius, ns, True, True)
    ref32 = F.max_pool2d(R.shared_mlp_eval(grouped, layers), kernel_size=[1, ns]).squeeze(-1)
    ref64 = sa_ref64(xyz, new_xyz, feats, idx, layers, radius, ns)
    return Case(name=name, B=B, N=N, M=M, C=C, spec=spec, radius=radius, ns=ns, scale_in_weights=siw, hoist=hoist, kernel=kernel,
                compact=compact, xyz=xyz, new_xyz=new_xyz, feats=feats, layers=layers, idx=idx, ref32=ref32, ref64=ref64,
                Y=yardstick(ref32, ref64), use_xyz=True, normalize_xyz=True, relu=(True,) * (len(spec) - 1))


# ------------------------------------------------------------------------------------------- set abstraction: the options
# The 13 shapes of SA_CASES again, on clouds whose balls hold DISTINCT points, one option set each. sa_case's resampled clouds
# (synth.frames with K_s = N / 2) fill most balls with the centre and copies of it: rel is mostly 0, and the reference hardly
# moves when normalize_xyz is flipped or the xyz channels are dropped (tests/test_fused_ref_cpu.py measures what these do).
def cube_clouds(seed, B, N):
    """(B,N,3) float32, uniform in [0, 1)^3 (a double just below 1 that rounds to 1.0f is put back below 1). With B >= 3 cloud 1 is a copy of cloud 0 and the LAST cloud is all zero: the
    repeated-index and every-point-in-every-ball edges of sa_case's clouds stay."""
    s = np.minimum(np.random.RandomState(seed).uniform(0, 1, (B, N, 3)).astype(np.float32), np.nextafter(np.float32(1), np.float32(0)))
    if B >= 3:
        s[1] = s[0]
        s[-1] = 0.0
    return s


# A layer's form, as pt_utils.Conv2d can be built and as ptt_sa_layer can describe it:
#   "bn"    conv + BatchNorm                                scale, shift                  (scale folded: NULL, shift)
#   "bn0"   conv + BatchNorm with running_mean = beta = 0   scale, shift = NULL           (scale folded: NULL, NULL)
#   "bias"  conv with bias, bn=False                        scale = NULL, shift = the bias
#   "none"  conv without bias, bn=False                     scale = NULL, shift = NULL
FORMS = ("bn", "bn0", "bias", "none")

# id -> (shape: a key of SA_CASES, the options that differ from sa_case's: use_xyz, normalize_xyz, relu (per SharedMLP layer),
#        forms (per layer), scale_in_weights, radius, seed)
SA_OPTION_CASES = {
    # normalize_xyz = 0 on every kernel family
    "norm0_lds4_111":      ("lds4_111", dict(normalize_xyz=False)),
    "norm0_lds12_1035":    ("lds12_1035", dict(normalize_xyz=False)),
    "norm0_wave32_5":      ("wave32_5", dict(normalize_xyz=False)),
    "norm0_wave16_21":     ("wave16_21", dict(normalize_xyz=False)),
    "norm0_stream_33":     ("stream_33", dict(normalize_xyz=False)),
    "norm0_stream_1027":   ("stream_1027", dict(normalize_xyz=False)),
    "norm0_fused32_33":    ("fused32_33", dict(normalize_xyz=False)),
    # 257 feature channels next to 3 coordinates, and a third of the outputs belong to the all-zero cloud: at the shape's own
    # radius and seed 7 the flip moves 20.2 % of the outputs, at this radius and seed 24.6 %
    "norm0_fused16_21":    ("fused16_21", dict(normalize_xyz=False, radius=0.35, seed=11)),
    "norm0_fused64_10":    ("fused64_10", dict(normalize_xyz=False)),
    # use_xyz = 0: the rows are the C feature channels alone, layer 0 packed with rot = 0
    "noxyz_wave16_18":     ("wave16_18", dict(use_xyz=False)),
    "noxyz_fused32_33":    ("fused32_33", dict(use_xyz=False)),
    "noxyz_fused16_21":    ("fused16_21", dict(use_xyz=False)),
    "noxyz_fused64_10":    ("fused64_10", dict(use_xyz=False)),
    # the last layer without ReLU: the pooled maximum may be negative. A maximum over many distinct rows seldom is: at the
    # shapes' own radii 4 - 18 % of the outputs are negative on these clouds, so the radius is lowered (the rule of
    # tests/test_fused_ref_cpu.py: a case that misses a condition changes its radius or seed) until 26 - 33 % are
    "last0_lds4_1":        ("lds4_1", dict(relu=(True, True, False))),
    "last0_wave16_18":     ("wave16_18", dict(relu=(True, False), radius=0.2)),
    "last0_stream_1029":   ("stream_1029", dict(relu=(True, True, False), radius=0.2)),
    "last0_fused32_33":    ("fused32_33", dict(relu=(True, True, False), radius=0.2)),
    "last0_fused16_21":    ("fused16_21", dict(relu=(True, True, False), radius=0.2)),
    "last0_fused64_10":    ("fused64_10", dict(relu=(True, False), radius=0.25)),
    # an inner layer without ReLU: the lds shape must fall to the wave kernel for either of `p.L[0].relu && p.L[1].relu`
    # (sa_lds_kernel has both activations built in), the stream shape to the fused kernel for `p.L[0].relu`; and the fused
    # kernel with layer 0 inside, where the flag is the middle layer's
    "inner0_lds4_111":     ("lds4_111", dict(relu=(False, True, True))),
    "inner1_lds4_111":     ("lds4_111", dict(relu=(True, False, True))),
    "inner1_lds12_1035":   ("lds12_1035", dict(relu=(True, False, True))),
    "inner0_stream_33":    ("stream_33", dict(relu=(True, False, True))),
    "inner1_fused32_33":   ("fused32_33", dict(relu=(True, False, True))),
    # the hoisted layer 0 without ReLU (ptt_sa_desc.l0_relu = 0)
    "l0relu0_stream_1027": ("stream_1027", dict(relu=(False, True, True))),
    "l0relu0_fused16_21h": ("fused16_21h", dict(relu=(False, True, True))),
    # shift = NULL and scale = NULL
    "none_wave16_18":      ("wave16_18", dict(forms=("none", "none"))),
    "none_fused16_21":     ("fused16_21", dict(forms=("none", "bias", "none"))),
    "bn0_wave32_5":        ("wave32_5", dict(forms=("bn0", "bn0", "bn0"))),            # scale set, shift = NULL
    "bn0_fused32_33":      ("fused32_33", dict(forms=("bn0", "bn", "bn0"))),
    "bn0_lds4_1":          ("lds4_1", dict(forms=("bn0", "bn0", "bn0"))),              # scale folded, shift = NULL
    "bn0_stream_33":       ("stream_33", dict(forms=("bn", "bn0", "bn0"))),
}


def option_layers(layers, forms, use_xyz):
    """The layers of a shape in the forms of an option case: the same convolution weights (use_xyz off: without their three
    xyz columns), BatchNorm kept, centred ("bn0") or replaced by a bias / by nothing."""
    out = []
    for l, (L, form) in enumerate(zip(layers, forms)):
        assert form in FORMS
        w = L["conv_weight"]
        if l == 0 and not use_xyz:
            w = w[:, 3:].contiguous()
        if form in ("bn", "bn0"):
            n = dict(L, conv_weight=w)
            if form == "bn0":
                n.update(bn_mean=torch.zeros_like(L["bn_mean"]), bn_bias=torch.zeros_like(L["bn_bias"]), shift_is_zero=True)
        else:
            n = {"conv_weight": w}
            if form == "bias":
                n["conv_bias"] = L["bn_bias"].clone()
        out.append(n)
    return out


def layer_affine(L):
    """(scale | None, shift | None) with which a layer is (W x) * scale + shift, float32 on the host, formed as
    tests.util.fold_layers forms them; shift is None where it is zero by construction (what a caller passes as NULL)."""
    if "bn_weight" not in L:
        return None, L.get("conv_bias")
    scale = L["bn_weight"] / torch.sqrt(L["bn_var"] + L["eps"])
    return scale, (None if L.get("shift_is_zero") else L["bn_bias"] - L["bn_mean"] * scale)


def option_kernel(c):
    """sa_dispatch for an (option) case: what the C dispatch sees of its flags."""
    run = c.relu[1:] if c.hoist else c.relu
    no_scale = c.scale_in_weights or all("bn_weight" not in L for L in (c.layers[1:] if c.hoist else c.layers))
    return sa_dispatch(c.B, c.M, c.C, c.spec, c.ns, no_scale, c.hoist, c.use_xyz, run[0], run[1] if len(run) > 1 else True)


def option_flips(c):
    """The single flags an option case varies -> {name: keyword arguments of sa_ref with that ONE flag put back}."""
    flips = {}
    if not c.normalize_xyz:
        flips["normalize_xyz"] = dict(normalize_xyz=True)
    if not c.use_xyz:                                   # the xyz channels back, with the weight columns the case dropped
        flips["use_xyz"] = dict(use_xyz=True, layers=c.layers_xyz)
    for l, on in enumerate(c.relu):
        if not on:
            flips["relu[%d]" % l] = dict(relu=tuple(True if k == l else r for k, r in enumerate(c.relu)))
    if "bn0" in c.forms and not c.scale_in_weights:     # a scale pointer next to shift = NULL: the scale ignored
        flips["scale"] = dict(layers=[{"conv_weight": L["conv_weight"]} if f == "bn0" else L for L, f in zip(c.layers, c.forms)])
    return flips


def option_ref(c, dtype=torch.float64, **override):
    kw = dict(use_xyz=c.use_xyz, normalize_xyz=c.normalize_xyz, relu=c.relu, layers=c.layers)
    kw.update(override)
    layers = kw.pop("layers")
    return sa_ref(c.xyz, c.new_xyz, c.feats, c.idx, layers, c.radius, c.ns, dtype=dtype, **kw)


@functools.lru_cache(maxsize=None)
def sa_option_case(name):
    shape, opt = SA_OPTION_CASES[name]
    B, N, M, C, spec, radius, ns, siw, hoist, _, _ = SA_CASES[shape]
    use_xyz, normalize = opt.get("use_xyz", True), opt.get("normalize_xyz", True)
    relu = tuple(opt.get("relu", (True,) * (len(spec) - 1)))
    forms = tuple(opt.get("forms", ("bn",) * (len(spec) - 1)))
    radius, siw = opt.get("radius", radius), opt.get("scale_in_weights", siw)
    assert len(relu) == len(forms) == len(spec) - 1 and (use_xyz or (C > 0 and not hoist))
    rs = np.random.RandomState(N + C)
    s = cube_clouds(opt.get("seed", 7), B, N)
    xyz = torch.from_numpy(s)
    inds = torch.from_numpy(O.fps(s, M))
    new_xyz = torch.gather(xyz, 1, inds.long()[..., None].expand(-1, -1, 3)).contiguous()
    feats = torch.from_numpy(rs.standard_normal((B, C, N)).astype(np.float32)) if C else None
    layers = option_layers(mlp_layers(N, spec), forms, use_xyz)          # the shape's own weights
    idx = torch.from_numpy(np.ascontiguousarray(O.ball_query(new_xyz.numpy(), s, radius, ns)))
    spec = list(spec) if use_xyz else [C] + list(spec[1:])
    c = Case(name=name, shape=shape, B=B, N=N, M=M, C=C, spec=spec, radius=radius, ns=ns, scale_in_weights=siw, hoist=hoist,
             xyz=xyz, new_xyz=new_xyz, feats=feats, layers=layers, idx=idx, use_xyz=use_xyz, normalize_xyz=normalize, relu=relu,
             forms=forms, layers_xyz=option_layers(mlp_layers(N, SA_CASES[shape][4]), forms, True))
    c["kernel"], _ = option_kernel(c)
    c["compact"] = c.kernel.startswith(("sa_lds", "sa_stream"))
    c["ref32"], c["ref64"] = option_ref(c, torch.float32), option_ref(c)
    c["Y"] = yardstick(c.ref32, c.ref64)
    return c


def distinct_full_share(c):
    """Share of a case's balls whose ns slots hold ns distinct points."""
    srt = np.sort(c.idx.numpy(), axis=-1)
    return float(((srt[..., 1:] != srt[..., :-1]).sum(axis=-1) + 1 == c.ns).mean())


# -------------------------------------------------------------------------------------------------------------------- xcorr
def xcorr_layers(seed, f, widths):
    """SharedMLP weights [1 + 3 + f, C0, ...] as tests.util.cosine_sim_params draws them (mlp_layers on the seed)."""
    return mlp_layers(seed, [4 + f] + list(widths))


def xcorr_core(sf, tf, txyz, layers):
    """oracle.dense_ref.cosine_sim_aug (p2b_xcoor.py:35-42) cut before the trailing convolutions, in the dtype of its
    inputs -> (pooled (B,Cout,n2), sim (B,n1,n2))."""
    b, f, n2 = sf.shape
    n1 = tf.shape[-1]
    sim = F.cosine_similarity(tf.unsqueeze(-1).expand(b, f, n1, n2), sf.unsqueeze(2).expand(b, f, n1, n2), dim=1)     # :35-36
    t = txyz.transpose(1, 2).contiguous().unsqueeze(-1).expand(b, 3, n1, n2)                                          # :37
    fusion = torch.cat((sim.unsqueeze(1), t), dim=1)                                                                  # :38
    fusion = torch.cat((fusion, tf.unsqueeze(-1).expand(b, f, n1, n2)), dim=1)                                        # :39
    fusion = R.shared_mlp_eval(fusion, layers)                                                                        # :40
    return F.max_pool2d(fusion, kernel_size=[fusion.size(2), 1]).squeeze(2), sim                                      # :41-42


XCORR_WIDTHS = {(8, 2): [8, 32, 64], (8, 3): [8, 64, 32, 96], (40, 2): [40, 32, 64], (40, 3): [40, 64, 32, 96],
                (256, 2): [256, 256, 256], (256, 3): [256, 256, 256, 256]}
XCORR_PLAIN = [(C0, B, Ns, Nt, nrem) for C0 in (8, 40, 256) for (B, Ns, Nt) in ((1, 1, 64), (3, 5, 192)) for nrem in (2, 3)]
XCORR_F = 20                # feature channels of the plain cases
# the split form: (B, Ns, Nt, C feature channels, widths C0 ...)
XCORR_SPLIT = [(1, 8, 64, 20, (40, 64, 96)), (2, 12, 128, 256, (256, 256, 256))]
COS_CASES = [(1, 20, 9, 3), (2, 300, 5, 130)]          # (B, C, Ns, Nt)


@functools.lru_cache(maxsize=None)
def xcorr_case(B, Ns, Nt, f, widths):
    seed = 77 + Nt + 10 * Ns + widths[0] + len(widths)
    rs = np.random.RandomState(seed)
    layers = xcorr_layers(seed, f, widths)
    sf = torch.from_numpy(rs.standard_normal((B, f, Ns)).astype(np.float32))
    tf = torch.from_numpy(rs.standard_normal((B, f, Nt)).astype(np.float32))
    tf[0, :, 0] = 0.0                                   # one all-zero template feature row: norm clamped at eps, cosine 0
    txyz = torch.from_numpy(rs.uniform(-2, 2, (B, Nt, 3)).astype(np.float32))
    ref32, sim32 = xcorr_core(sf, tf, txyz, layers)
    ref64, sim64 = xcorr_core(sf.double(), tf.double(), txyz.double(), double_layers(layers))
    return Case(B=B, Ns=Ns, Nt=Nt, f=f, widths=list(widths), layers=layers, sf=sf, tf=tf, txyz=txyz, ref32=ref32, ref64=ref64,
                sim32=sim32, sim64=sim64, Y=yardstick(ref32, ref64))


@functools.lru_cache(maxsize=None)
def cos_case(B, C, Ns, Nt):
    rs = np.random.RandomState(C + Ns)
    sf = torch.from_numpy(rs.standard_normal((B, C, Ns)).astype(np.float32))
    tf = torch.from_numpy(rs.standard_normal((B, C, Nt)).astype(np.float32))
    tf[0, :, 0] = 0.0
    cos = lambda s, t: F.cosine_similarity(s[:, :, :, None], t[:, :, None, :], dim=1, eps=1e-8)       # (B,Ns,Nt)
    ref32, ref64 = cos(sf, tf), cos(sf.double(), tf.double())
    return Case(B=B, C=C, Ns=Ns, Nt=Nt, sf=sf, tf=tf, ref32=ref32, ref64=ref64, Y=yardstick(ref32, ref64))


# -------------------------------------------------------------------------------------------------------------- pair kernel
PAIR_SHAPES = [(1, 16), (3, 18), (1, 50)]       # (B, N): N = k = 16; two points of one cloud per tile with B * N / 2 odd tiles
PAIR_HEADS = [1, 2, 4, 8]
D_MODEL, KNN = 512, 16


def _double(P):
    return {k: v.double() for k, v in P.items()}


def gamma_params(seed, hd):
    """fc_gamma of MulHeadTransformerLayer: ONE hd x hd MLP all heads share (multitransformer.py:20), nn.Linear's init range."""
    rs = np.random.RandomState(seed)
    b = 1.0 / np.sqrt(hd)
    t = lambda *s: torch.from_numpy(rs.uniform(-b, b, s).astype(np.float32))
    return {"fc_gamma.0.weight": t(hd, hd), "fc_gamma.0.bias": t(hd), "fc_gamma.2.weight": t(hd, hd), "fc_gamma.2.bias": t(hd)}


def heads_attention(xyz, qkv, knn, P, heads):
    """MulHeadTransformerLayer.forward's attention (multitransformer.py:46-56) in the dtype of its inputs, from the stacked
    q | k | v rows (B,N,3D) and a fixed kNN table -> (res (B,N,D) with the heads' channels concatenated, attn (B*heads,N,k,hd))."""
    B, N, D3 = qkv.shape
    D, H = D3 // 3, heads
    idx = knn.long()
    q, kf, vf = qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:]
    key, value = R.index_points(kf, idx), R.index_points(vf, idx)
    d = xyz[:, :, None] - R.index_points(xyz, idx)
    pos = F.linear(F.relu(F.linear(d, P["fc_delta.0.weight"], P["fc_delta.0.bias"])), P["fc_delta.2.weight"], P["fc_delta.2.bias"])
    query = q.view(B, N, H, -1).permute(0, 2, 1, 3).flatten(0, 1)
    pos, key, value = (t.view(B, N, t.shape[2], H, -1).permute(0, 3, 1, 2, 4).flatten(0, 1) for t in (pos, key, value))
    a = query[:, :, None] - key + pos
    a = F.linear(F.relu(F.linear(a, P["fc_gamma.0.weight"], P["fc_gamma.0.bias"])), P["fc_gamma.2.weight"], P["fc_gamma.2.bias"])
    attn = F.softmax(a / math.sqrt(key.size(-1)), dim=-2)
    res = (attn * (value + pos)).sum(dim=2)                                 # (B*H, N, hd)
    res = res.view(B, H, N, -1).permute(0, 2, 1, 3).reshape(B, N, D)
    return res, attn


@functools.lru_cache(maxsize=None)
def pair_case(B, N, heads):
    """heads == 1: the whole TransformerBlock (dense_ref.transformer_block: fc1, attention, fc2 + residual), as
    tests/test_dense_gpu.py::test_transformer_pair_kernel chains it. heads > 1: the attention alone, from float32 q | k | v
    rows formed on the host (the layer's LayerNorms are not this kernel's)."""
    rs = np.random.RandomState(N)
    P = transformer_params(N)
    s, _ = synth.frames(N, B, N, 64, K_s=N)
    xyz = torch.from_numpy(s)
    feats = torch.from_numpy(rs.standard_normal((B, N, 256)).astype(np.float32))
    knn = torch.from_numpy(O.knn(s, KNN))
    c = Case(B=B, N=N, heads=heads, P=P, xyz=xyz, feats=feats, knn=knn)
    if heads == 1:
        res32, attn32 = R.transformer_block(xyz, feats, P, KNN, knn_idx=knn.long())
        res64, attn64 = R.transformer_block(xyz.double(), feats.double(), _double(P), KNN, knn_idx=knn.long())
    else:
        G = gamma_params(N + heads, D_MODEL // heads)
        P = dict(P)
        P.update(G)
        x = F.linear(feats, P["fc1.weight"], P["fc1.bias"])
        qkv = F.linear(x, torch.cat([P["w_qs.weight"], P["w_ks.weight"], P["w_vs.weight"]], 0))
        res32, attn32 = heads_attention(xyz, qkv, knn, P, heads)
        res64, attn64 = heads_attention(xyz.double(), qkv.double(), knn, _double(P), heads)
        c.update(P=P, qkv=qkv)
    c.update(res32=res32, attn32=attn32, res64=res64, attn64=attn64, Y_res=yardstick(res32, res64), Y_attn=yardstick(attn32, attn64))
    return c
