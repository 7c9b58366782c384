"""Float64 references of the training-only row kernels (xcorr_z0*, sa_z0*, the partial-sum finishers, pt_attn_train_bwd,
unit_rows / cos_bwd_rows), written from the formulas of include/ptt_hip.h; plain torch, CPU or device tensors alike.

None of these reads a kernel or ptt_amd/ops.py. Inputs are float32 (float64 partial sums excepted), the arithmetic is float64
and so are the outputs. Every function takes `dtype`: torch.float32 runs the same lines in float32 — the "plain float32 torch
formulation" whose own distance from float64 is the yardstick Y of tests/test_train_rows_guard_gpu.py. Two things are float32
in both runs because the header defines them so: the relative coordinates of sa_z0_rows (subtract, then multiply by
float32(1 / radius), each rounded) and the z0 that decides a ReLU mask (for xcorr: fma(cos, w, P) rounded once).

tests/test_train_rows_ref_cpu.py anchors every backward formula here to torch.autograd."""
import torch

F32, F64 = torch.float32, torch.float64
FLIP_MARGIN = 1e-4          # no ReLU argument z * a + b of a test may lie closer to 0 than this


def rel_err(got, ref64):
    """max|got - ref64| / max|ref64| (0 / 0 = 0): the distance every bound of the guard tests is stated in."""
    ref64 = ref64.to(F64)
    d = float((got.to(F64).reshape(ref64.shape) - ref64).abs().max()) if ref64.numel() else 0.0
    m = float(ref64.abs().max()) if ref64.numel() else 0.0
    return d / m if m > 0 else d


# ------------------------------------------------------------------------------------------------------- CosineSimAug layer 0
def xcorr_z0(P, cos, w, dtype=F64):
    """z0[b,j,i,:] = P[b,i,:] + cos[b,j,i] * w[:] -> (z0 (B*n2*n1, C) in (b, j, i) row order, its column sums, its column sums
    of squares). P (B,n1,C), cos (B,n2,n1), w (C,)."""
    P, cos, w = P.to(dtype), cos.to(dtype), w.to(dtype)
    z0 = (P[:, None, :, :] + cos[..., None] * w).reshape(-1, P.shape[-1])
    return z0, z0.sum(0), (z0 * z0).sum(0)


def xcorr_z0_f32(P, cos, w):
    """The float32 z0 the forward kernel defines — fma(cos, w, P) rounded once — formed as (P64 + cos64 * w64) cast to float32:
    the product of two float32 is exact in float64, so only the sum is rounded (to 53 bits) before the cast; the two roundings
    differ from the single one only when the exact value lies within 2^-29 ulp of a float32 tie."""
    return xcorr_z0(P, cos, w)[0].to(F32)


def xcorr_z0_bwd(dz0, cos, w, B, n2, n1, dtype=F64):
    """-> (dP (B,n1,C) = sum_j dz0, dcos (B,n2,n1) = <dz0, w>, dw (C,) = sum dz0 * cos)."""
    dz = dz0.to(dtype).reshape(B, n2, n1, -1)
    cos, w = cos.to(dtype), w.to(dtype)
    return dz.sum(1), (dz * w).sum(-1), (dz * cos[..., None]).sum((0, 1, 2))


# ---------------------------------------------------------------------------------------------------- BatchNorm + ReLU backward
def near_flips(z, a, b, margin=FLIP_MARGIN):
    """How many entries of the ReLU argument z * a + b (float64, from the float32 z) lie within `margin` of 0."""
    return int(((z.to(F64) * a.to(F64) + b.to(F64)).abs() < margin).sum())


def clear_shift(za):
    """For za = z * a (R,C): a shift b (C,) float32 that puts the ReLU threshold of every channel into the middle of the widest
    gap between neighbouring values of its column, among the central half of the sorted column (R >= 8: about half the mask is
    on); fewer rows: one below / above the whole column in turn (mask all on / all off). How the tests whose z is derived
    (xcorr: from P, cos and w) keep z * a + b away from a flip; near_flips() then counts what is left."""
    za = za.to(F64)
    R, C = za.shape
    s = za.sort(0).values
    if R >= 8:
        lo, hi = R // 4, R - R // 4
        k = (s[lo + 1:hi] - s[lo:hi - 1]).argmax(0)[None] + lo
        t = (s.gather(0, k) + s.gather(0, k + 1))[0] / 2
    else:
        t = torch.where(torch.arange(C, device=za.device) % 2 == 0, s[0] - 1, s[-1] + 1)
    return (-t).to(F32)


def bn_relu_bwd(G, z, mean, invstd, gamma, a, b, s0, s1, R, dtype=F64):
    """dy = G where z * a + b > 0, else 0; dz = gamma * invstd * (dy - s0 / R - xhat * s1 / R), xhat = (z - mean) * invstd.
    s0 / s1 (the column sums of the chunk partials: sum dy, sum dy * xhat) are inputs of the ABI and taken as given. The mask is
    decided in float64 from the float32 z, and no entry may sit within FLIP_MARGIN of a flip (asserted here): a kernel that
    rounds z * a + b differently must still agree on every mask bit."""
    assert near_flips(z, a, b) == 0, "a ReLU argument within %g of 0: the mask is not robust to rounding" % FLIP_MARGIN
    mask = (z.to(F64) * a.to(F64) + b.to(F64)) > 0
    G, z, mean, invstd, gamma, s0, s1 = (t.to(dtype) for t in (G, z, mean, invstd, gamma, s0, s1))
    dy = torch.where(mask, G, torch.zeros_like(G))
    xhat = (z - mean) * invstd
    return gamma * invstd * (dy - s0 / R - xhat * (s1 / R))


def partial_sums(part):
    """The column sums (s0, s1) of chunk partials (chunks, 2, C) in float64."""
    part = part.to(F64)
    return part[:, 0].sum(0), part[:, 1].sum(0)


def xcorr_z0_bnbwd(part, G, P, cos, w, mean, invstd, gamma, a, b, dtype=F64):
    """bn_relu_bwd on the float32 z0 of xcorr_z0_f32, then xcorr_z0_bwd -> (dP, dcos, dw, dgamma = s1, dbeta = s0)."""
    B, n1, _ = P.shape
    n2 = cos.shape[1]
    s0, s1 = partial_sums(part)
    dz0 = bn_relu_bwd(G, xcorr_z0_f32(P, cos, w), mean, invstd, gamma, a, b, s0, s1, B * n2 * n1, dtype)
    return xcorr_z0_bwd(dz0, cos, w, B, n2, n1, dtype) + (s1.to(dtype), s0.to(dtype))


def sa_z0_bnbwd(part, G, z0, rel, mean, invstd, gamma, a, b, dtype=F64):
    """bn_relu_bwd on the stored float32 z0, then the K = 3 weight gradient -> (dz0 (R,C), d_wx (C,3) = dz0^T rel, dgamma, dbeta)."""
    s0, s1 = partial_sums(part)
    dz0 = bn_relu_bwd(G, z0, mean, invstd, gamma, a, b, s0, s1, z0.shape[0], dtype)
    return dz0, dz0.t() @ rel.to(dtype), s1.to(dtype), s0.to(dtype)


def bn_bwd_consts(part, mean, invstd, gamma, R, dtype=F64):
    """-> (dgamma, dbeta, k1, c0, c1): dz = c0 + c1 (z - mean) + (mask ? k1 g : 0) with k1 = gamma * invstd,
    c1 = -k1 * invstd * dgamma / R, c0 = -k1 * dbeta / R."""
    s0, s1 = partial_sums(part)
    dbeta, dgamma, invstd, gamma = s0.to(dtype), s1.to(dtype), invstd.to(dtype), gamma.to(dtype)
    k1 = gamma * invstd
    return dgamma, dbeta, k1, -k1 * dbeta / R, -k1 * invstd * dgamma / R


def bn_stats(s1, s2, R, eps, dtype=F64):
    """(mean, biased variance, 1 / sqrt(var + eps)) from the column sums and sums of squares over R rows."""
    s1, s2 = s1.to(dtype), s2.to(dtype)
    mean = s1 / R
    var = (s2 / R - mean * mean).clamp_min(0)
    return mean, var, 1.0 / torch.sqrt(var + eps)


def bn_train_tail(mean, var, invstd, gamma, beta, running_mean, running_var, momentum, n, dtype=F64):
    """torch.nn.BatchNorm1d's training-mode bookkeeping -> (act_a = gamma * invstd, act_b = beta - mean * act_a, running_mean,
    running_var): running <- (1 - momentum) * running + momentum * batch, the variance unbiased by n / (n - 1) (n = 1: as is)."""
    mean, var, invstd, gamma, beta, rm, rv = (t.to(dtype) for t in (mean, var, invstd, gamma, beta, running_mean, running_var))
    a = gamma * invstd
    unbias = n / (n - 1.0) if n > 1 else 1.0
    return a, beta - mean * a, (1 - momentum) * rm + momentum * mean, (1 - momentum) * rv + momentum * (var * unbias)


# ------------------------------------------------------------------------------------------------------- hoisted SA layer 0
def sa_rel_f32(xyz, new_xyz, idx, radius, normalize):
    """rel (B, M*ns, 3) in float32 exactly as the header says: xyz[b, idx] - new_xyz[b, m], then (normalize) times
    float32(1 / radius), each operation rounded to float32."""
    B, M, ns = idx.shape
    nb = torch.gather(xyz.to(F32), 1, idx.long().reshape(B, M * ns, 1).expand(-1, -1, 3)).view(B, M, ns, 3)
    rel = nb - new_xyz.to(F32)[:, :, None, :]
    if normalize:
        rel = rel * (torch.ones((), dtype=F32, device=rel.device) / torch.tensor(radius, dtype=F32, device=rel.device))
    return rel.reshape(B, M * ns, 3)


def sa_z0_rows(xyz, new_xyz, idx, term, wx, radius, normalize, dtype=F64):
    """-> (z0 (B*M*ns, C) = term[b, idx] + Wx . rel from the float32 rel, rel_rows (B*M*ns, 3) float32). term (B,N,C) or None,
    wx (C,3)."""
    B, M, ns = idx.shape
    rel = sa_rel_f32(xyz, new_xyz, idx, radius, normalize)
    z0 = rel.to(dtype) @ wx.to(dtype).t()
    if term is not None:
        C = term.shape[-1]
        z0 = torch.gather(term.to(dtype), 1, idx.long().reshape(B, M * ns, 1).expand(-1, -1, C)) + z0
    return z0.reshape(B * M * ns, -1), rel.reshape(B * M * ns, 3)


# --------------------------------------------------------------------------------------------- Point-Transformer attention
def attn_bwd(attn, vf, knn, pos, dres, scale, dtype=F64):
    """From dres (B,N,D): dvp_ij = attn_ij * dres_i; da_ij = attn_ij * (dres_i . vp_ij - sum_j' attn_ij' dres_i . vp_ij') * scale
    (per channel), vp_ij = vf[knn_ij] + pos_ij. attn / pos (B,N,k,D), vf (B,N,D), knn (B,N,k) -> (da, dvp)."""
    B, N, k, D = attn.shape
    attn, vf, pos, dres = (t.to(dtype) for t in (attn, vf, pos, dres))
    vp = torch.gather(vf, 1, knn.long().reshape(B, N * k, 1).expand(-1, -1, D)).view(B, N, k, D) + pos
    g = dres[:, :, None, :]
    t = g * vp
    s = (attn * t).sum(2, keepdim=True)
    return attn * (t - s) * scale, attn * g


# --------------------------------------------------------------------------------------------------------- cosine map ends
def unit_rows(x, eps, dtype=F64):
    """x (B,C,n) -> (unit (B,n,C) = x / max(|x|, eps), nrm (B,n) = max(|x|, eps), NEGATIVE where |x| < eps)."""
    eps = float(torch.tensor(eps, dtype=F32))                       # the float32 value the ABI receives
    xr = x.to(dtype).transpose(1, 2)
    norm = torch.sqrt((xr * xr).sum(-1))
    d = norm.clamp_min(eps)
    return xr / d[..., None], torch.where(norm < eps, -d, d)


def cos_bwd_rows(A, unit, nrm, G, cos, own_is_row, dtype=F64):
    """dx (B,n,C) = (A - (sum_i G cos) unit) / |nrm|, the projection term only where nrm > 0. G / cos (B,n2,n1); own_is_row: this
    side indexes their rows (n = n2, the sum runs over n1), else their columns."""
    A, unit, nrm, G, cos = (t.to(dtype) for t in (A, unit, nrm, G, cos))
    proj = (G * cos).sum(2 if own_is_row else 1)
    proj = torch.where(nrm > 0, proj, torch.zeros_like(proj))
    return (A - proj[..., None] * unit) / nrm.abs()[..., None]
