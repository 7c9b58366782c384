"""nn.LayerNorm in training mode on the HIP kernels (ptt_layernorm_train_fwd_f32 / ptt_layernorm_bwd_f32) against
torch.nn.functional.layer_norm and its autograd in float64 on the CPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ptt_amd import ops

pytestmark = pytest.mark.gpu
EPS = 1e-5
ROWS = (1, 3, 128, 6144)
CS = (256, 512)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _inputs(rows, C, offset, seed=0):
    rs = np.random.RandomState(seed + 131 * rows + C)
    x = rs.standard_normal((rows, C)).astype(np.float32) * (1.0 + rs.rand(rows, 1).astype(np.float32)) + np.float32(offset)
    w = (1.0 + 0.3 * rs.standard_normal(C)).astype(np.float32)
    b = (0.5 * rs.standard_normal(C)).astype(np.float32)
    r = rs.standard_normal((rows, C)).astype(np.float32)
    dy = rs.standard_normal((rows, C)).astype(np.float32)
    return tuple(torch.from_numpy(a) for a in (x, w, b, r, dy))


@pytest.mark.parametrize("offset", (0.0, 100.0))
@pytest.mark.parametrize("residual", (False, True))
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("rows", ROWS)
def test_forward_matches_float64(dev, rows, C, residual, offset):
    x, w, b, r, _ = _inputs(rows, C, offset)
    y, mean, rstd = ops.layernorm_train_fwd(x.to(dev), w.to(dev), b.to(dev), EPS, r.to(dev) if residual else None)
    xd = x.double()
    ref = F.layer_norm(xd, (C,), w.double(), b.double(), EPS) + (r.double() if residual else 0.0)
    mu = xd.mean(1)
    rs = 1.0 / torch.sqrt(xd.var(1, unbiased=False) + EPS)
    np.testing.assert_allclose(y.cpu().numpy(), ref.numpy(), atol=1e-5, rtol=1e-5)
    # 1e-6 relative: of the row's own scale |mean| + std for the mean (a row's mean can be arbitrarily close to 0 while the rounding of
    # its sum follows the size of the terms), of the value for rstd
    err = (mean.cpu().double() - mu).abs()
    assert bool((err <= 1e-6 * (mu.abs() + 1.0 / rs)).all()), float((err / (mu.abs() + 1.0 / rs)).max())
    np.testing.assert_allclose(rstd.cpu().numpy(), rs.numpy(), rtol=1e-6)


@pytest.mark.parametrize("offset", (0.0, 100.0))
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("rows", ROWS)
def test_backward_matches_float64_autograd(dev, rows, C, offset):
    x, w, b, _, dy = _inputs(rows, C, offset)
    xd, wd, bd = (t.double().requires_grad_(True) for t in (x, w, b))
    F.layer_norm(xd, (C,), wd, bd, EPS).backward(dy.double())
    _, mean, rstd = ops.layernorm_train_fwd(x.to(dev), w.to(dev), b.to(dev), EPS)
    dx, dw, db = ops.layernorm_bwd(dy.to(dev), x.to(dev), mean, rstd, w.to(dev))
    np.testing.assert_allclose(dx.cpu().numpy(), xd.grad.numpy(), atol=1e-5, rtol=1e-5)
    # dw / db are sums over the rows: the absolute bound is 1e-5 of the column's sum of |term|
    xhat = ((xd - xd.mean(1, keepdim=True)) / torch.sqrt(xd.var(1, unbiased=False, keepdim=True) + EPS)).detach()
    for got, ref, terms in ((dw, wd.grad, (dy.double() * xhat).abs().sum(0)), (db, bd.grad, dy.double().abs().sum(0))):
        err = (got.cpu().double() - ref).abs()
        bound = 1e-5 * ref.abs() + 1e-5 * terms
        assert bool((err <= bound).all()), float((err / bound).max())


@pytest.mark.parametrize("rows", (128, 6144, 6144 - 13, 37))
def test_two_runs_are_bit_identical(dev, rows):
    C = 512
    x, w, b, r, dy = (t.to(dev) for t in _inputs(rows, C, 0.0))
    a = ops.layernorm_train_fwd(x, w, b, EPS, r)
    c = ops.layernorm_train_fwd(x, w, b, EPS, r)
    assert all(torch.equal(u, v) for u, v in zip(a, c))
    g1 = ops.layernorm_bwd(dy, x, a[1], a[2], w)
    g2 = ops.layernorm_bwd(dy, x, a[1], a[2], w)
    assert all(torch.equal(u, v) for u, v in zip(g1, g2))


def test_too_many_channels_is_the_library_error(dev):
    C = 1024 + 64
    x = torch.zeros((4, C), device=dev)
    w, b = torch.ones((C,), device=dev), torch.zeros((C,), device=dev)
    with pytest.raises(RuntimeError, match="ptt_layernorm_train_fwd_f32"):
        ops.layernorm_train_fwd(x, w, b, EPS)
    m = torch.zeros((4,), device=dev)
    with pytest.raises(RuntimeError, match="ptt_layernorm_bwd_f32"):
        ops.layernorm_bwd(x, x, m, m, w)
