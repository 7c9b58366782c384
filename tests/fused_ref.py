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


def sa_dispatch(B, M, C, spec, ns, scale_in_weights, hoisted):
    """The kernel ptt_sa_fused_fwd_f32 launches for a level, restated from its dispatch (mfma_ops.hip: the chain of `if`s
    after `const int total_centres = d->B * d->M;`) -> (name, facts about the launch's tiles)."""
    total = B * M
    louts = spec[1:]
    if C == 0 and not hoisted and ns == 32 and louts == [64, 64, 128] and scale_in_weights:
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
    if hoisted and spec[1] == 128 and ns == 32 and rem == [128, 256] and scale_in_weights:
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


def sa_ref64(xyz, new_xyz, feats, idx, layers, radius, ns):
    """oracle.dense_ref.query_and_group (use_xyz, normalize_xyz) + shared_mlp_eval + max-pool in float64 on a fixed idx."""
    x, c = xyz.double(), new_xyz.double()
    g = _sa_gather64(x.transpose(1, 2).contiguous(), idx) - c.transpose(1, 2).unsqueeze(-1)
    g = g / float(np.float32(radius))
    if feats is not None:
        g = torch.cat([g, _sa_gather64(feats.double(), idx)], dim=1)
    return F.max_pool2d(R.shared_mlp_eval(g, double_layers(layers)), kernel_size=[1, ns]).squeeze(-1)


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
                Y=yardstick(ref32, ref64))


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
