"""tests/step_losses_ref.py against float64 torch: the four losses equal nn.BCEWithLogitsLoss(pos_weight) / nn.SmoothL1Loss
composed as the heads compose them (tests/test_step_ops_gpu.py::_stock_losses), and the three gradients equal autograd's, to 1e-12
relative — with an index list and with explicit labels, with no positive seed label, with no proposal label and with an empty
proposal mask. The weights are the float32 values the descriptor carries; the labels and masks come from
step_losses_ref.proposal_labels in both compositions (and equal what the stock float32 lines give on these inputs). No GPU."""
import pytest
import torch

from tests import step_losses_ref as S

F32, F64 = torch.float32, torch.float64
TOL = 1e-12
W = (0.2, 1.0, 1.5, 0.2)


def inputs(B, N, Ns, M, seed, near, positive=True):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=F32)
    reg = torch.cat((r(B, 3) * 0.5, r(B, 1), r(B, 2)), dim=1)                  # two spare columns: ld_reg = 6
    votes = reg[:, None, :3] + r(B, N, 3) * 0.8
    centres = reg[:, None, :3] + r(B, M, 3) * near
    box = torch.cat((centres + r(B, M, 3) * 0.7, reg[:, None, 3:4] + r(B, M, 1) * 1.5, r(B, M, 1) * 3), dim=2)
    cls_points = (torch.rand(B, Ns, generator=g) > 0.6).to(F32) if positive else torch.zeros(B, Ns, dtype=F32)
    inds = torch.stack([torch.randperm(Ns, generator=g)[:N] for _ in range(B)])
    return r(B, N) * 3, votes, box, centres, cls_points, inds, reg


def stock(seed_cls, votes, box, y, label, mask, reg, pw_s, pw_b, w):
    """_stock_losses of tests/test_step_ops_gpu.py in float64, the labels given."""
    bce = lambda pw, red: torch.nn.BCEWithLogitsLoss(pos_weight=pw, reduction=red)
    sl1 = torch.nn.SmoothL1Loss(reduction='none')
    reg = reg.double()
    l1 = bce(pw_s, 'mean')(seed_cls.view(-1), y.view(-1))
    l2 = (sl1(votes, reg[:, None, :3].expand_as(votes)).mean(2) * y).sum() / (y.sum() + EPS)
    l3 = torch.sum(bce(pw_b, 'none')(box[:, :, -1], label) * mask) / (torch.sum(mask) + EPS)
    pred = box[:, :, :-1]
    l4 = (sl1(pred, reg[:, None, :4].expand_as(pred)).mean(2) * label).sum() / (label.sum() + EPS)
    return (l1 * w[0] + l2 * w[1]) + (l3 * w[2] + l4 * w[3]), (l1, l2, l3, l4)


EPS = float(torch.tensor(1e-6, dtype=F32))


def close(got, want, what):
    assert got.dtype == F64, what
    assert S.rel_err(got, want) <= TOL, "%s: %.3e" % (what, S.rel_err(got, want))


CASES = {
    "ordinary":        dict(B=3, N=37, Ns=50, M=9, near=0.25, positive=True, explicit=False),
    "explicit labels": dict(B=2, N=5, Ns=5, M=4, near=0.3, positive=True, explicit=True),
    "no seed label":   dict(B=2, N=11, Ns=16, M=6, near=0.3, positive=False, explicit=False),
    "no label":        dict(B=2, N=7, Ns=9, M=8, near=5.0, positive=True, explicit=False),
    "no mask":         dict(B=2, N=7, Ns=9, M=8, near=None, positive=True, explicit=True),
}


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("pw", [(1.0, 2.0), (2.0, 1.0)])
def test_losses_and_gradients_equal_float64_torch(name, pw):
    c = CASES[name]
    seed_cls, votes, box, centres, cls_points, inds, reg = inputs(c['B'], c['N'], c['Ns'], c['M'], 7 + c['N'], c['near'] or 0.3, c['positive'])
    if c['near'] is None:                                   # every proposal at distance 0.45: between the two thresholds
        g = torch.Generator().manual_seed(3)
        u = torch.randn(c['B'], c['M'], 3, generator=g, dtype=F32)
        centres = reg[:, None, :3] + 0.45 * u / u.norm(dim=2, keepdim=True)
    if c['explicit']:
        cls_label, inds = cls_points.gather(1, inds).contiguous(), None
    else:
        cls_label = cls_points
        inds[0, 0], inds[-1, -1] = -3, c['Ns'] + 5          # clamped to point 0 and point Ns - 1
    y = S.seed_labels(cls_label, inds)
    if inds is not None:
        assert float(y[0, 0]) == float(cls_label[0, 0]) and float(y[-1, -1]) == float(cls_label[-1, -1])
    label, mask, dist = S.proposal_labels(centres, reg)
    # the stock float32 lines give the same labels on these inputs
    d_stock = torch.sqrt(torch.sum((centres - reg[:, None, 0:3]) ** 2, dim=-1) + 1e-6)
    assert torch.equal(label, (d_stock < 0.3).float()) and torch.equal(mask, ((d_stock < 0.3) | (d_stock > 0.6)).float())
    if name == "no seed label":
        assert float(y.sum()) == 0
    if name == "no label":
        assert float(label.sum()) == 0 and float(mask.sum()) > 0
    if name == "no mask":
        assert float(mask.sum()) == 0 and float(label.sum()) == 0
    if name == "ordinary":
        assert 0 < float(label.sum()) < float(mask.sum()) < label.numel() and 0 < float(y.sum()) < y.numel()
    w = [float(torch.tensor(k, dtype=F32)) for k in W]
    pw_s, pw_b = torch.tensor([pw[0]], dtype=F64), torch.tensor([pw[1]], dtype=F64)
    leaves = [t.double().requires_grad_() for t in (seed_cls, votes, box)]
    total, parts = stock(leaves[0], leaves[1], leaves[2], y.double(), label.double(), mask.double(), reg, pw_s, pw_b, w)
    (total * 0.75).backward()
    out = S.losses(seed_cls, y, votes, reg, box, label, mask, pw[0], pw[1], W)
    close(out[0], total.detach(), name + ": total")
    for k, p in enumerate(parts):
        close(out[1 + k], p.detach(), "%s: loss %d" % (name, k))
    assert float(out[5]) == float(y.sum()) and float(out[6]) == float(mask.sum()) and float(out[7]) == float(label.sum())
    grads = S.gradients(seed_cls, y, votes, reg, box, label, mask, pw[0], pw[1], W, upstream=0.75)
    for got, leaf, what in zip(grads, leaves, ("d seed_cls", "d votes", "d box_data")):
        close(got, leaf.grad, "%s: %s" % (name, what))
    if name == "no seed label":
        assert float(out[2]) == 0 and float(grads[1].abs().max()) == 0
    if name in ("no label", "no mask"):
        assert float(out[4]) == 0 and float(grads[2][..., :4].abs().max()) == 0
    if name == "no mask":
        assert float(out[3]) == 0 and float(grads[2][..., 4].abs().max()) == 0


def test_float32_run_is_float32_and_close():
    seed_cls, votes, box, centres, cls_points, inds, reg = inputs(3, 37, 50, 9, 44, 0.25)
    y = S.seed_labels(cls_points, inds)
    label, mask, _ = S.proposal_labels(centres, reg)
    a = S.losses(seed_cls, y, votes, reg, box, label, mask, 1.0, 2.0, W, dtype=F32)
    b = S.losses(seed_cls, y, votes, reg, box, label, mask, 1.0, 2.0, W)
    assert a.dtype == F32 and b.dtype == F64 and 0 < S.rel_err(a, b) < 1e-5
    for g32, g64 in zip(S.gradients(seed_cls, y, votes, reg, box, label, mask, 1.0, 2.0, W, 0.75, F32),
                        S.gradients(seed_cls, y, votes, reg, box, label, mask, 1.0, 2.0, W, 0.75)):
        assert g32.dtype == F32 and g64.dtype == F64 and 0 < S.rel_err(g32, g64) < 1e-5
