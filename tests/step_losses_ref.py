"""Float64 references of the four tracking losses of a training step and their three gradients (ptt_track_losses_f32 /
ptt_track_losses_bwd_f32), written from include/ptt_hip.h and the formulas at the top of ptt_amd/csrc/step_ops.hip; plain torch,
CPU tensors. None of this reads a kernel or ptt_amd/ops.py.

What is float32 by definition is kept apart from what is measured. seed_labels() is a gather and proposal_labels() follows the
kernel's float32 operation order — (dx dx + dy dy) + dz dz, + 1e-6f, sqrtf, compared with 0.3f / 0.6f — so a distance within
rounding of a threshold gives the reference the label the kernel has. losses() / gradients() take the labels and masks as
INPUTS: float32 logits, votes, boxes and labels in, `dtype` arithmetic and results out. dtype = torch.float32 runs the same lines
in float32: the plain float32 formulation whose own distance from float64 is the yardstick Y of tests/test_step_guard_gpu.py.

tests/test_step_losses_ref_cpu.py anchors every function here to float64 torch (BCEWithLogitsLoss, SmoothL1Loss, autograd)."""
import torch

F32, F64 = torch.float32, torch.float64


def rel_err(got, ref64):
    """max|got - ref64| / max|ref64| (0 / 0 = 0)."""
    ref64 = ref64.to(F64)
    d = float((got.to(F64).reshape(ref64.shape) - ref64).abs().max()) if ref64.numel() else 0.0
    m = float(ref64.abs().max()) if ref64.numel() else 0.0
    return d / m if m > 0 else d


def seed_labels(cls_label, search_inds):
    """cls_label (B,Ns) per search point, search_inds (B,N) int64 -> (B,N): indices below 0 read point 0, indices at or beyond Ns
    read point Ns - 1 (the header's clamp). search_inds None: cls_label is already (B,N)."""
    if search_inds is None:
        return cls_label
    return cls_label.gather(1, search_inds.clamp(0, cls_label.shape[1] - 1))


def proposal_labels(centres, reg_label):
    """box_voting_head.py:96-101 in the kernel's float32 operation order -> (label, mask, dist), all (B,M) float32:
    dist = sqrt(((dx dx + dy dy) + dz dz) + 1e-6), label = dist < 0.3, mask = dist < 0.3 or dist > 0.6."""
    assert centres.dtype == F32 and reg_label.dtype == F32
    d = centres - reg_label[:, None, :3]
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    dist = torch.sqrt(((dx * dx + dy * dy) + dz * dz) + torch.tensor(1e-6, dtype=F32))
    lo, hi = torch.tensor(0.3, dtype=F32), torch.tensor(0.6, dtype=F32)
    label = (dist < lo).to(F32)
    mask = ((dist < lo) | (dist > hi)).to(F32)
    return label, mask, dist


def _bce(x, y, pw):
    """nn.BCEWithLogitsLoss(pos_weight): (1 - y) x + (1 + (pw - 1) y) (log1p(exp(-|x|)) + max(-x, 0))."""
    return (1 - y) * x + (1 + (pw - 1) * y) * (torch.log1p(torch.exp(-x.abs())) + torch.clamp(-x, min=0))


def _bce_grad(x, y, pw):
    return (1 + (pw - 1) * y) * torch.sigmoid(x) - pw * y


def _sl1(d):
    """nn.SmoothL1Loss, beta = 1."""
    a = d.abs()
    return torch.where(a < 1, 0.5 * d * d, a - 0.5)


def _sl1_grad(d):
    return torch.where(d.abs() < 1, d, torch.sign(d))


def _cast(dtype, *ts):
    return [t.to(dtype) for t in ts]


def losses(seed_cls, y, votes, reg_label, box_data, label, mask, pw_seed, pw_box, weights, dtype=F64):
    """-> out8 (8,) of `dtype`: [0] the weighted total, [1..4] seed classification (mean over B*N), seed vote regression
    (sum(mean_3 smooth-L1 * y) / (sum y + 1e-6)), proposal score (sum(BCE * mask) / (sum mask + 1e-6)), proposal box regression
    (sum(mean_4 smooth-L1 * label) / (sum label + 1e-6)), [5..7] sum y, sum mask, sum label.
    seed_cls (B,N), y (B,N), votes (B,N,3), reg_label (B, >= 4), box_data (B,M,5), label / mask (B,M)."""
    x, y, v, r, p, lab, m = _cast(dtype, seed_cls, y, votes, reg_label[:, :4], box_data, label, mask)
    pw_s, pw_b = float(pw_seed), float(pw_box)
    w = [torch.tensor(float(torch.tensor(wk, dtype=F32)), dtype=dtype) for wk in weights]        # the descriptor's float32 weights
    eps = torch.tensor(float(torch.tensor(1e-6, dtype=F32)), dtype=dtype)
    l1 = _bce(x, y, pw_s).mean()
    l2 = (_sl1(v - r[:, None, :3]).sum(2) / 3 * y).sum() / (y.sum() + eps)
    l3 = (_bce(p[..., 4], lab, pw_b) * m).sum() / (m.sum() + eps)
    l4 = (_sl1(p[..., :4] - r[:, None, :]).sum(2) / 4 * lab).sum() / (lab.sum() + eps)
    total = (l1 * w[0] + l2 * w[1]) + (l3 * w[2] + l4 * w[3])
    return torch.stack([total, l1, l2, l3, l4, y.sum(), m.sum(), lab.sum()])


def gradients(seed_cls, y, votes, reg_label, box_data, label, mask, pw_seed, pw_box, weights, upstream=1.0, dtype=F64):
    """d total / d (seed_cls (B,N), votes (B,N,3), box_data (B,M,5)) times `upstream`, of `dtype`."""
    x, y, v, r, p, lab, m = _cast(dtype, seed_cls, y, votes, reg_label[:, :4], box_data, label, mask)
    pw_s, pw_b = float(pw_seed), float(pw_box)
    w = [torch.tensor(float(torch.tensor(wk, dtype=F32)), dtype=dtype) for wk in weights]
    eps = torch.tensor(float(torch.tensor(1e-6, dtype=F32)), dtype=dtype)
    g = torch.tensor(float(torch.tensor(upstream, dtype=F32)), dtype=dtype)
    d_cls = g * w[0] * _bce_grad(x, y, pw_s) / x.numel()
    d_votes = (g * w[1] * y / (y.sum() + eps) / 3)[..., None] * _sl1_grad(v - r[:, None, :3])
    d_box = torch.empty_like(p)
    d_box[..., :4] = (g * w[3] * lab / (lab.sum() + eps) / 4)[..., None] * _sl1_grad(p[..., :4] - r[:, None, :])
    d_box[..., 4] = g * w[2] * m / (m.sum() + eps) * _bce_grad(p[..., 4], lab, pw_b)
    return d_cls, d_votes, d_box
