"""tests/train_rows_ref.py against torch.autograd: every backward formula the guard tests of the training-only kernels measure
against is the gradient of its forward, to 1e-12 relative, at the smallest ragged shapes of tests/test_train_rows_guard_gpu.py.
No GPU."""
import pytest
import torch

from tests import train_rows_ref as T

F32, F64 = torch.float32, torch.float64
TOL = 1e-12


def rnd(g, *shape):
    return torch.randn(*shape, generator=g, dtype=F32)


def away_from_zero(g, *shape):
    """Random signs, magnitudes in [0.5, 1.5): a BatchNorm weight whose ReLU arguments are not all squeezed towards 0."""
    return (torch.rand(*shape, generator=g, dtype=F32) + 0.5) * (torch.randint(0, 2, shape, generator=g) * 2 - 1).to(F32)


def close(got, want, what):
    assert got.dtype == F64, what
    assert T.rel_err(got, want) <= TOL, "%s: %.3e" % (what, T.rel_err(got, want))


@pytest.mark.parametrize("B,n2,n1,C", [(1, 1, 1, 4), (2, 7, 5, 12), (3, 9, 3, 256)])
def test_xcorr_backward_is_the_gradient_of_its_forward(B, n2, n1, C):
    g = torch.Generator().manual_seed(n2 * 100 + C)
    P, cos, w, up = rnd(g, B, n1, C), rnd(g, B, n2, n1).clamp(-1, 1), rnd(g, C), rnd(g, B * n2 * n1, C)
    Pd, cd, wd = (t.double().requires_grad_() for t in (P, cos, w))
    z0 = (Pd[:, None] + cd[..., None] * wd).reshape(-1, C)
    ref_z0, s1, s2 = T.xcorr_z0(P, cos, w)
    close(ref_z0, z0.detach(), "z0")
    close(s1, z0.detach().sum(0), "column sums")
    close(s2, (z0.detach() ** 2).sum(0), "column sums of squares")
    z0.backward(up.double())
    for got, want, name in zip(T.xcorr_z0_bwd(up, cos, w, B, n2, n1), (Pd.grad, cd.grad, wd.grad), ("dP", "dcos", "dw")):
        close(got, want, name)


def _bn_relu(z, gamma, beta, eps):
    mean, var = z.mean(0), z.var(0, unbiased=False)
    invstd = 1.0 / torch.sqrt(var + eps)
    return torch.relu(gamma * (z - mean) * invstd + beta), mean, invstd


def _clear_beta(z, gamma, eps):
    """beta (float64) for which no relu argument of BatchNorm(z) lies near 0 (train_rows_ref.clear_shift), with the deferred
    activation's constants a = gamma * invstd, b = beta - mean * a."""
    mean, invstd = z.mean(0), 1.0 / torch.sqrt(z.var(0, unbiased=False) + eps)
    a = gamma.double() * invstd
    b = T.clear_shift(z * a).double()
    return b + mean * a, a, b


def _own_sums(G, z, mean, invstd, a, b):
    """One chunk of partials holding the batch's own sums: sum dy and sum dy * xhat."""
    zd = z.double()
    dy = torch.where(zd * a + b > 0, G.double(), torch.zeros((), dtype=F64))
    return torch.stack([dy.sum(0), (dy * (zd - mean) * invstd).sum(0)])[None]


@pytest.mark.parametrize("R,C", [(3, 4), (65, 4), (70, 12)])
def test_bn_relu_backward_is_the_gradient_of_batchnorm_and_relu(R, C):
    """From three rows on: with the batch's own statistics one row has variance 0 and two rows have xhat = +-1, where the
    gradient cancels to rounding noise and a relative bound says nothing."""
    g = torch.Generator().manual_seed(R + C)
    z, gamma, up = rnd(g, R, C), away_from_zero(g, C), rnd(g, R, C)
    zd = z.double().requires_grad_()
    beta, a, b = _clear_beta(z.double(), gamma, 1e-5)
    y, mean, invstd = _bn_relu(zd, gamma.double(), beta, 1e-5)
    y.backward(up.double())
    mean, invstd = mean.detach(), invstd.detach()
    part = _own_sums(up, z, mean, invstd, a, b)
    s0, s1 = T.partial_sums(part)
    close(T.bn_relu_bwd(up, z, mean, invstd, gamma, a, b, s0, s1, R), zd.grad, "dz")
    # the three-constant form of the same gradient
    dgamma, dbeta, k1, c0, c1 = T.bn_bwd_consts(part, mean, invstd, gamma, R)
    mask = (z.double() * a + b) > 0
    close(c0 + c1 * (z.double() - mean) + torch.where(mask, k1 * up.double(), torch.zeros((), dtype=F64)), zd.grad, "dz from k1, c0, c1")


def _sa_inputs(g, B, N, M, ns, C):
    xyz = rnd(g, B, N, 3)
    idx = torch.randint(0, N, (B, M, ns), generator=g).to(torch.int32)
    idx[0, 0, :] = idx[0, 0, 0]                                    # a padded group
    new_xyz = torch.gather(xyz, 1, idx[:, :, 0].long()[..., None].expand(-1, -1, 3)).contiguous()     # rel = 0 in slot 0
    return xyz, new_xyz, idx, rnd(g, B, N, C), rnd(g, C, 3)


@pytest.mark.parametrize("B,N,M,ns,C,with_term,normalize", [(1, 5, 1, 1, 4, False, False), (3, 65, 7, 16, 132, True, True)])
def test_sa_layer0_backward_is_the_gradient_of_its_forward(B, N, M, ns, C, with_term, normalize):
    g = torch.Generator().manual_seed(N + C)
    xyz, new_xyz, idx, term, wx = _sa_inputs(g, B, N, M, ns, C)
    term = term if with_term else None
    R = B * M * ns
    gamma, up = away_from_zero(g, C), rnd(g, R, C)
    z0_ref, rel = T.sa_z0_rows(xyz, new_xyz, idx, term, wx, 0.3, normalize)
    assert rel.dtype == F32 and float(rel.view(B, M, ns, 3)[:, :, 0].abs().max()) == 0.0
    # the forward again, from the float32 rel: gather and a K = 3 product
    wd = wx.double().requires_grad_()
    z0 = rel.double() @ wd.t()
    if with_term:
        td = term.double().requires_grad_()
        z0 = z0 + td[torch.arange(B)[:, None], idx.long().view(B, -1)].reshape(R, C)
    close(z0_ref, z0.detach(), "z0")
    beta, a, b = _clear_beta(z0.detach(), gamma, 1e-5)
    y, mean, invstd = _bn_relu(z0, gamma.double(), beta, 1e-5)
    y.backward(up.double())
    mean, invstd = mean.detach(), invstd.detach()
    part = _own_sums(up, z0.detach(), mean, invstd, a, b)
    dz0, dwx, dgamma, dbeta = T.sa_z0_bnbwd(part, up, z0.detach(), rel, mean, invstd, gamma, a, b)
    close(dwx, wd.grad, "d_wx")
    if with_term:                                                  # the row scatter of dz0 is the gradient of the gathered term
        dterm = torch.zeros(B, N, C, dtype=F64).index_put_((torch.arange(B)[:, None].expand(B, M * ns), idx.long().view(B, -1)),
                                                           dz0.view(B, M * ns, C), accumulate=True)
        close(dterm, td.grad, "d_term")


@pytest.mark.parametrize("B,N,k,D", [(1, 1, 8, 4), (2, 17, 16, 132)])
def test_attention_backward_is_the_gradient_of_the_softmax_weighted_sum(B, N, k, D):
    g = torch.Generator().manual_seed(N + D)
    a, vf, pos, up = rnd(g, B, N, k, D), rnd(g, B, N, D), rnd(g, B, N, k, D), rnd(g, B, N, D)
    knn = torch.randint(0, N, (B, N, k), generator=g).to(torch.int32)
    scale = 0.37
    ad = a.double().requires_grad_()
    vp = (vf.double()[torch.arange(B)[:, None], knn.long().view(B, -1)].view(B, N, k, D) + pos.double()).requires_grad_()
    attn = torch.softmax(ad * scale, dim=2)
    (attn * vp).sum(2).backward(up.double())
    da, dvp = T.attn_bwd(attn.detach(), vf, knn, pos, up, scale)
    close(da, ad.grad, "da")
    close(dvp, vp.grad, "dvp")


@pytest.mark.parametrize("C,n2,n1", [(1, 1, 1), (63, 5, 1), (65, 5, 5)])
def test_cosine_backward_is_the_gradient_of_cosine_with_clamp_min(C, n2, n1):
    g = torch.Generator().manual_seed(C + n2)
    B, eps = 2, 1e-8
    s, t, up = rnd(g, B, C, n2), rnd(g, B, C, n1), rnd(g, B, n2, n1)
    s[0, :, 0] = 0.0                                               # an all-zero row
    s[1, :, -1] *= 1e-10 / float(s[1, :, -1].norm())               # a non-zero row under the clamp
    sd, td = s.double().requires_grad_(), t.double().requires_grad_()
    e = float(torch.tensor(eps, dtype=F32))
    cos = torch.einsum("bcj,bci->bji", sd, td) / (sd.norm(dim=1).clamp_min(e)[:, :, None] * td.norm(dim=1).clamp_min(e)[:, None, :])
    cos.backward(up.double())
    us, ns = T.unit_rows(s, eps)
    ut, nt = T.unit_rows(t, eps)
    assert bool((ns[0, 0] == -e) and (ns[1, -1] == -e)) and bool((nt > 0).all())
    close(us[1, -1], s[1, :, -1].double() / e, "the clamped row is x / eps")
    close(torch.einsum("bjc,bic->bji", us, ut), cos.detach(), "the map is a product of unit rows")
    ds = T.cos_bwd_rows(torch.einsum("bji,bic->bjc", up.double(), ut), us, ns, up, cos.detach(), True)
    dt = T.cos_bwd_rows(torch.einsum("bji,bjc->bic", up.double(), us), ut, nt, up, cos.detach(), False)
    close(ds.transpose(1, 2), sd.grad, "d search")
    close(dt.transpose(1, 2), td.grad, "d template")
