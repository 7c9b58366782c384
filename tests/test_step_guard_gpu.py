"""The ends of the training step on the C ABI, behind guard bands (tests/guard.py): ptt_track_losses_f32 / _bwd_f32 against the
float64 formulas of tests/step_losses_ref.py (anchored to float64 torch by tests/test_step_losses_ref_cpu.py), and
ptt_adam_clip_step_f32 / _dev_f32 against each other and against the Adam kind of ptt_optim_clip_step_f32.

The method of tests/test_train_rows_guard_gpu.py: every launch goes through guard.launch, the descriptor is filled through
_lib.TrackLossDesc directly, every output lies in a guarded(...) buffer of exactly its size (out8: 8 words, total: 1 word, the
partial sums: n_chunks doubles, the norm: 1 word), every input is embed(...)-ded between NaN / INDEX_FILL words, check_guard runs
after each launch, a second launch gives the same bits, and the guarded result equals what the ops.* wrapper returns.

Losses. The seed labels are a gather (indices below 0 and from Ns on clamp, as the header says) and the proposal labels / masks
come from step_losses_ref.proposal_labels, which follows the kernel's float32 operation order; the float64 formulas take them as
inputs. Exact: out8[5..7] equal the integer sums of the float32 labels and masks; `total` equals out8[0] bitwise; a vote row whose
seed label is 0, columns 0..3 of a proposal row whose label is 0 and column 4 of a row whose mask is 0 are exactly 0; with no
positive seed label / no proposal inside 0.3 / an empty mask the loss concerned is exactly 0. Everything else: err <= R * Y,
err = max|got - ref64| / max|ref64|, Y = max(e32, 4 * 2^-24), e32 the distance of the float32 run of step_losses_ref from its
float64 run (never the kernel's own output). Forced values in every case that has room: vote and box residuals of exactly 0 and
exactly +-1 (smooth-L1's knee), logits of +-100, one proposal inside 0.3, one between 0.3 and 0.6, one beyond 0.6.

The ratio R. err / Y measured on an MI355X per result (table below); R = twice the worst ratio, rounded up to one significant
digit, and R <= 8 is asserted.

  case (B,N,Ns,M)                   total / seed cls / seed reg / proposal cls / proposal reg     d seed_cls / d votes / d box_data
  one of each (1,1,1,1)             0.34 / 0.31 / 0.19 / 0.07 / 0.36     0.14 / 0.19 / 0.44
  ragged (2,37,50,5)                0.21 / 0.19 / 0.35 / 0.13 / 0.16     0.64 / 0.26 / 0.15
  1023 seeds (3,341,400,7)          0.00 / 0.02 / 0.00 / 0.01 / 0.20     0.60 / 0.00 / 0.22
  1024 seeds (4,256,256,3)          0.09 / 0.14 / 0.19 / 0.12 / 0.00     0.41 / 0.31 / 0.10
  1025 seeds (5,205,300,64)         0.12 / 0.01 / 0.12 / 0.00 / 0.00     0.73 / 0.21 / 0.00
  more proposals (2,3,8,200)        0.24 / 0.01 / 0.02 / 0.00 / 0.17     0.16 / 0.02 / 0.34
  0.00 is an exact 0 where the case forces one (no positive seed label at 1023 seeds, no proposal inside 0.3 at 1024 seeds, an
  empty mask at 1025 seeds); otherwise an error below 0.005 Y (total, 1023 seeds: 2e-11; proposal cls, more proposals: 5e-10).
  Worst 0.73 (d seed_cls, 1025 seeds), so R = 2; nothing came near the ratio of 4 that asks for a look.

Refusals (B, N or M <= 0, ld_reg 3, a null pointer, Ns <= 0 with an index list, a null output): PTT_EINVAL, "bad size / null
pointer / inconsistent descriptor" in the header's list of statuses, and every output word untouched.

Adam pair. On the SHAPES of tests/test_optimization_gpu.py (1 element, one chunk + 4, over two chunks), parameters, both moments and
gradients between guard words: the device-hyper form is bit-identical to the by-value form, and both are bit-identical to
ptt_optim_clip_step_f32 with one group of kind Adam on copies of the same tensors (the header: "the update of
ptt_adam_clip_step_f32, bit for bit") — with max_norm active, inactive and absent (then the partial sums and the norm are not
touched), weight_decay 0 and 0.01, write_clipped 0 and 1.

The whole file takes about three seconds on an MI355X; no case more than 0.2."""
import ctypes
import math
import os
import re

import pytest
import torch

from ptt_amd import _lib, ops
from tests import guard
from tests import step_losses_ref as S
from tests.guard import check_guard, embed, guarded
from tests.test_optimization_gpu import SHAPES

pytestmark = pytest.mark.gpu
L, P = guard.launch, guard.ptr
F32, F64, I32, I64 = torch.float32, torch.float64, torch.int32, torch.int64
U = 2.0 ** -24
W = (0.2, 1.0, 1.5, 0.2)

R_RATIO = 2.0               # twice the worst measured err / Y (0.73, table above), rounded up to one significant digit
RATIOS = {}


def test_r_is_within_its_cap():
    assert R_RATIO <= 8


def bound(case, got, ref64, ref32):
    Y = max(S.rel_err(ref32, ref64), 4 * U)
    err = S.rel_err(got.detach().cpu(), ref64)
    r = err / Y
    RATIOS[case] = max(RATIOS.get(case, 0.0), r)
    print("RATIO %-52s err %.3e  Y %.3e  err/Y %.2f" % (case, err, Y, r))
    assert r <= R_RATIO, "%s: %.2f x the float32 formulation's own distance from float64 (R = %g)" % (case, r, R_RATIO)


def E(t, dev, **kw):
    return embed(t.to(dev).contiguous(), **kw)


def G(shape, dtype, dev, **kw):
    return guarded(shape, dtype, device=dev, **kw)


def done(outs, ins=()):
    torch.cuda.synchronize()
    for v in outs:
        check_guard(v)
    for v in ins:
        check_guard(v, all_written=False)


def same_bits(a, b, what):
    a, b = a.contiguous().view(I32).reshape(-1), b.to(a.device).contiguous().view(I32).reshape(-1)
    assert a.numel() == b.numel() and torch.equal(a, b), "%s: not the same bits" % what


def _header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "ptt_hip.h")) as fh:
        return " ".join(re.sub(r"^\s*\*", " ", fh.read(), flags=re.M).split())


# ================================================================================================================== losses
# name -> B, N, Ns, M, ld_reg, index list, total given, upstream, (pos_weight_seed, pos_weight_box), what is forced to zero
LOSS_CASES = {
    "one of each":        dict(B=1, N=1, Ns=1, M=1, ld=4, inds=True, total=True, up=None, pw=(1.0, 1.0), zero=None),
    "ragged":             dict(B=2, N=37, Ns=50, M=5, ld=7, inds=True, total=False, up=0.75, pw=(1.0, 2.0), zero=None),
    "1023 seeds":         dict(B=3, N=341, Ns=400, M=7, ld=4, inds=False, total=True, up=None, pw=(2.0, 1.0), zero="seed labels"),
    "1024 seeds":         dict(B=4, N=256, Ns=256, M=3, ld=7, inds=True, total=False, up=0.75, pw=(2.0, 2.0), zero="labels"),
    "1025 seeds":         dict(B=5, N=205, Ns=300, M=64, ld=4, inds=True, total=True, up=0.75, pw=(1.0, 2.0), zero="masks"),
    "more proposals":     dict(B=2, N=3, Ns=8, M=200, ld=7, inds=True, total=True, up=None, pw=(2.0, 1.0), zero=None),
}


def loss_inputs(c):
    """Host float32 inputs of one case. The ground-truth rows are multiples of 2^-10, so that a residual of exactly 0 or +-1 can
    be placed; the index list (when there is one) holds an index below 0 and one beyond Ns."""
    B, N, Ns, M = c['B'], c['N'], c['Ns'], c['M']
    g = torch.Generator().manual_seed(B * 1000 + N + M)
    r = lambda *s: torch.randn(*s, generator=g, dtype=F32)
    reg = torch.round(torch.cat((r(B, 3) * 0.5, r(B, 1)), dim=1) * 1024) / 1024
    votes = reg[:, None, :3] + r(B, N, 3) * 0.8
    zero = c['zero']
    if zero == "labels":                                    # every proposal beyond 0.6
        u = r(B, M, 3)
        centres = reg[:, None, :3] + (0.7 + torch.rand(B, M, 1, generator=g)) * u / u.norm(dim=2, keepdim=True)
    elif zero == "masks":                                   # every proposal between 0.3 and 0.6
        u = r(B, M, 3)
        centres = reg[:, None, :3] + (0.35 + 0.2 * torch.rand(B, M, 1, generator=g)) * u / u.norm(dim=2, keepdim=True)
    else:
        centres = reg[:, None, :3] + r(B, M, 3) * 0.25
        if M >= 3:                                          # one proposal of each kind per frame
            centres[:, 0] = reg[:, :3] + torch.tensor([0.05, 0.0, 0.0])
            centres[:, 1] = reg[:, :3] + torch.tensor([0.0, 0.45, 0.0])
            centres[:, 2] = reg[:, :3] + torch.tensor([0.0, 0.0, 2.0])
        elif M == 1:
            centres[:, 0] = reg[:, :3] + torch.tensor([0.05, 0.0, 0.0])
    box = torch.cat((centres + r(B, M, 3) * 0.7, reg[:, None, 3:4] + r(B, M, 1) * 1.5, r(B, M, 1) * 3), dim=2)
    seed_cls = r(B, N) * 3
    if N >= 3:                                              # the knee, the origin and saturated logits
        votes[:, 0] = reg[:, :3]
        votes[:, 1] = reg[:, :3] + 1.0
        votes[:, 2] = reg[:, :3] - 1.0
        seed_cls[:, 0], seed_cls[:, 1] = 100.0, -100.0
    if M >= 3:
        box[:, 0, :4] = reg + torch.tensor([0.0, 1.0, -1.0, 0.25])          # the labelled row: the origin and both knees
        box[:, 1, :4] = reg + 1.0
        box[:, 2, :4] = reg - 1.0
        box[:, 0, 4], box[:, 2, 4] = 100.0, -100.0
    if c['inds']:
        cls_label = (torch.rand(B, Ns, generator=g) > 0.6).to(F32)
        if zero != "seed labels" and Ns >= 2:
            cls_label[:, 0], cls_label[:, Ns - 1] = 1.0, 0.0
        inds = torch.stack([torch.randint(0, Ns, (N,), generator=g) for _ in range(B)])
        if N >= 3:
            inds[:, 1], inds[:, 2] = 0, 0                                 # the forced vote rows carry a label (unless all are 0)
            inds[0, 0], inds[B - 1, N - 1] = -3, Ns + 5                   # clamped to point 0 and to point Ns - 1
            if B > 1:
                inds[0, N - 1] = Ns                                       # the first index beyond the cloud
    else:
        cls_label, inds = (torch.rand(B, N, generator=g) > 0.6).to(F32), None
    if zero == "seed labels":
        cls_label.zero_()
    elif N >= 3 and not c['inds']:
        cls_label[:, :3] = 1.0
    full = torch.full((B, c['ld']), float("nan"), dtype=F32)                # NaN in the spare columns
    full[:, :4] = reg
    return seed_cls, cls_label, inds, votes, full, box, centres


def loss_desc(c, emb, dev):
    seed_cls, cls_label, inds, votes, reg, box, centres, pw_s, pw_b = emb
    d = _lib.TrackLossDesc()
    d.seed_cls, d.cls_label, d.votes, d.reg_label = seed_cls.data_ptr(), cls_label.data_ptr(), votes.data_ptr(), reg.data_ptr()
    d.search_inds = inds.data_ptr() if inds is not None else None
    d.box_data, d.centres, d.pos_weight_seed, d.pos_weight_box = box.data_ptr(), centres.data_ptr(), pw_s.data_ptr(), pw_b.data_ptr()
    d.B, d.N, d.Ns, d.M, d.ld_reg = c['B'], c['N'], c['Ns'], c['M'], c['ld']
    d.w_seed_cls, d.w_seed_reg, d.w_box_cls, d.w_box_reg = W
    return d


def loss_setup(c, dev):
    host = loss_inputs(c)
    pw = (torch.tensor([c['pw'][0]], dtype=F32), torch.tensor([c['pw'][1]], dtype=F32))
    emb = [E(t, dev) if t is not None else None for t in host + pw]
    return host, emb, loss_desc(c, emb, dev)


@pytest.mark.parametrize("name", list(LOSS_CASES))
def test_track_losses_forward_and_backward(dev, name):
    c = LOSS_CASES[name]
    B, N, M = c['B'], c['N'], c['M']
    (seed_cls, cls_label, inds, votes, reg, box, centres), emb, d = loss_setup(c, dev)
    ins = [v for v in emb if v is not None]
    y = S.seed_labels(cls_label, inds)
    label, mask, dist = S.proposal_labels(centres, reg)
    if c['zero'] is None and M >= 3:
        assert bool((label[:, 0] == 1).all()) and bool((mask[:, 1] == 0).all()) and bool(((mask[:, 2] == 1) & (label[:, 2] == 0)).all())
    args = (seed_cls, y, votes, reg, box, label, mask, c['pw'][0], c['pw'][1], W)
    ref64, ref32 = S.losses(*args), S.losses(*args, dtype=F32)
    tag = "losses %s" % name

    def forward():
        out8 = G((8,), F32, dev)
        total = G((1,), F32, dev) if c['total'] else None
        L("ptt_track_losses_f32", dev, ctypes.byref(d), P(out8), P(total))
        done([out8] + ([total] if total is not None else []), ins)
        return (out8, total) if total is not None else (out8,)
    first, second = forward(), forward()
    for a, b in zip(first, second):
        same_bits(a, b, tag + ": a second launch")
    out8 = first[0]
    if c['total']:
        same_bits(first[1], out8[:1], tag + ": total against out8[0]")
    got = out8.cpu()
    assert float(got[5]) == float(y.sum()) and float(got[6]) == float(mask.sum()) and float(got[7]) == float(label.sum()), tag + ": the label sums"
    if c['zero'] == "seed labels":
        assert float(got[5]) == 0 and float(got[2]) == 0, tag
    if c['zero'] in ("labels", "masks"):
        assert float(got[7]) == 0 and float(got[4]) == 0, tag
    if c['zero'] == "masks":
        assert float(got[6]) == 0 and float(got[3]) == 0, tag
    if c['zero'] == "labels":
        assert float(got[6]) == B * M, tag
    for k, what in enumerate(("total", "seed cls", "seed reg", "proposal cls", "proposal reg")):
        bound("%s %s" % (tag, what), got[k], ref64[k], ref32[k])
    plain = [t.to(dev).contiguous() if t is not None else None for t in (seed_cls, cls_label, inds, votes, reg, box, centres)]
    pw_dev = (emb[7].contiguous(), emb[8].contiguous())
    p_total, p_out = ops.track_losses(*plain, *pw_dev, W)
    same_bits(out8, p_out, tag + " against ops.track_losses")
    same_bits(out8[:1], p_total.reshape(1), tag + " against ops.track_losses (total)")

    up = None if c['up'] is None else E(torch.tensor([c['up']], dtype=F32), dev)

    def backward():
        outs = [G((B, N), F32, dev), G((B, N, 3), F32, dev), G((B, M, 5), F32, dev)]
        L("ptt_track_losses_bwd_f32", dev, ctypes.byref(d), P(out8), P(up), *[P(o) for o in outs])
        done(outs, ins + [out8] + ([up] if up is not None else []))
        return outs
    g1, g2 = backward(), backward()
    for a, b in zip(g1, g2):
        same_bits(a, b, tag + ": a second backward launch")
    upv = 1.0 if c['up'] is None else c['up']
    r64, r32 = S.gradients(*args, upstream=upv), S.gradients(*args, upstream=upv, dtype=F32)
    for what, got_g, a, b in zip(("d seed_cls", "d votes", "d box_data"), g1, r64, r32):
        bound("%s %s" % (tag, what), got_g, a, b)
    d_votes, d_box = g1[1].cpu(), g1[2].cpu()
    assert float(d_votes[y == 0].abs().max() if bool((y == 0).any()) else 0.0) == 0.0, tag + ": vote rows without a label"
    assert float(d_box[..., :4][label == 0].abs().max() if bool((label == 0).any()) else 0.0) == 0.0, tag + ": box rows without a label"
    assert float(d_box[..., 4][mask == 0].abs().max() if bool((mask == 0).any()) else 0.0) == 0.0, tag + ": scores outside the mask"
    p_g = ops.track_losses_bwd(p_out, None if up is None else up.contiguous(), *plain, *pw_dev, W)
    for what, a, b in zip(("d seed_cls", "d votes", "d box_data"), g1, p_g):
        same_bits(a, b, "%s %s against ops.track_losses_bwd" % (tag, what))


EINVAL_WORDS = "bad size / null pointer / inconsistent descriptor"


@pytest.mark.parametrize("what", ["B 0", "N 0", "M -1", "ld_reg 3", "null votes", "null pos_weight_box", "Ns 0 with indices", "null out8"])
def test_track_losses_refusals(dev, what):
    assert "PTT_EINVAL = -1" in _header() and EINVAL_WORDS in _header()
    c = LOSS_CASES["ragged"]
    _, emb, d = loss_setup(c, dev)
    if what == "B 0":
        d.B = 0
    elif what == "N 0":
        d.N = 0
    elif what == "M -1":
        d.M = -1
    elif what == "ld_reg 3":
        d.ld_reg = 3
    elif what == "null votes":
        d.votes = None
    elif what == "null pos_weight_box":
        d.pos_weight_box = None
    elif what == "Ns 0 with indices":
        d.Ns = 0
    B, N, M = c['B'], c['N'], c['M']
    out8, total = G((8,), F32, dev), G((1,), F32, dev)
    grads = [G((B, N), F32, dev), G((B, N, 3), F32, dev), G((B, M, 5), F32, dev)]
    sums = E(torch.ones(8, dtype=F32), dev)
    with pytest.raises(RuntimeError, match="PTT_EINVAL"):
        L("ptt_track_losses_f32", dev, ctypes.byref(d), None if what == "null out8" else P(out8), P(total))
    with pytest.raises(RuntimeError, match="PTT_EINVAL"):
        L("ptt_track_losses_bwd_f32", dev, ctypes.byref(d), None if what == "null out8" else P(sums), None, *[P(o) for o in grads])
    if what == "null out8":                                 # and each null gradient output of the backward
        for k in range(3):
            ptrs = [P(o) for o in grads]
            ptrs[k] = None
            with pytest.raises(RuntimeError, match="PTT_EINVAL"):
                L("ptt_track_losses_bwd_f32", dev, ctypes.byref(d), P(sums), None, *ptrs)
    torch.cuda.synchronize()
    guard.assert_untouched(out8, total, sums, *grads)
    guard.assert_untouched(*[v for v in emb if v is not None])


# =============================================================================================================== Adam pair
LR, BETAS, EPS, STEP = 1e-3, (0.5, 0.999), 1e-6, 3


def adam_tensors(dev, embedded):
    """Parameters, gradients (norm far above 10) and both moments of SHAPES as 1-D tensors, the same values on every call."""
    g = torch.Generator().manual_seed(31)
    sizes = [int(torch.Size(s).numel()) for s in SHAPES]
    mk = (lambda t: E(t, dev)) if embedded else (lambda t: t.to(dev))
    params = [mk(torch.randn(n, generator=g)) for n in sizes]
    grads = [mk(torch.randn(n, generator=g) * 0.3) for n in sizes]
    m = [mk(torch.randn(n, generator=g) * 0.1) for n in sizes]
    v = [mk(torch.rand(n, generator=g) * 0.1) for n in sizes]
    return params, grads, m, v


@pytest.mark.parametrize("max_norm", ["active", "inactive", "absent"])
@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
@pytest.mark.parametrize("write_clipped", [0, 1])
def test_adam_pair_and_the_adam_kind_of_optim_clip_step(dev, max_norm, weight_decay, write_clipped):
    chunk = int(ops._host("ptt_adam_chunk_elems"))
    sizes = [int(torch.Size(s).numel()) for s in SHAPES]
    assert 1 in sizes and chunk + 4 in sizes and any(n > 2 * chunk for n in sizes)
    mn = {"active": 10.0, "inactive": 1e6, "absent": 0.0}[max_norm]
    step_size, bias2_sqrt = LR / (1.0 - BETAS[0] ** STEP), math.sqrt(1.0 - BETAS[1] ** STEP)
    h = ops.AdamTable.hyper(BETAS[0], BETAS[1], EPS, step_size, bias2_sqrt, weight_decay, mn, bool(write_clipped))
    original = adam_tensors(dev, False)
    results = []
    for form in ("value", "device"):
        params, grads, m, v = adam_tensors(dev, True)
        table = ops.AdamTable(params, m, v)
        table._refresh_grads(grads, "AdamTable")
        partial, norm = G((table.n_chunks,), F64, dev), G((1,), F32, dev)
        common = (P(table.table), P(table.which), P(table.first), table.n_chunks)
        if form == "value":
            L("ptt_adam_clip_step_f32", dev, *common, ctypes.byref(h), P(partial), table.n_chunks, P(norm))
        else:
            ring = ops.AdamHyperRing(dev)
            ring.upload(h)
            L("ptt_adam_clip_step_dev_f32", dev, *common, P(ring.dev), 1 if mn > 0 else 0, P(partial), table.n_chunks, P(norm))
        torch.cuda.synchronize()
        for t in params + grads + m + v:
            check_guard(t, all_written=False)
        if mn > 0:
            check_guard(partial)
            check_guard(norm)
        else:
            guard.assert_untouched(partial, norm)
        results.append((params, grads, m, v, partial, norm))
    # the Adam kind of ptt_optim_clip_step_f32 on copies of the same tensors
    params, grads, m, v = adam_tensors(dev, False)
    ot = ops.OptimTable(params, m, v, [0] * len(params), 1)
    ot._refresh_grads(grads, "OptimTable")
    oh = ops.OptimTable.hyper("adam", LR, STEP, BETAS, EPS, weight_decay)
    assert (oh.step_size, oh.bias2_sqrt, oh.one_minus_beta1, oh.one_minus_beta2) == (h.step_size, h.bias2_sqrt, h.one_minus_beta1, h.one_minus_beta2)
    o_partial, o_norm = G((ot.n_chunks,), F64, dev), G((1,), F32, dev)
    L("ptt_optim_clip_step_f32", dev, P(ot.table), ot.host.data_ptr(), len(ot.rows), P(ot.which), P(ot.first), ot.n_chunks, ot.hyper_array([oh]), 1,
      float(mn), int(write_clipped), P(o_partial), ot.n_chunks, P(o_norm))
    torch.cuda.synchronize()
    results.append((params, grads, m, v, o_partial, o_norm))
    tag = "adam (max_norm %s, wd %g, write_clipped %d)" % (max_norm, weight_decay, write_clipped)
    for form, res in zip(("the device-hyper form", "ptt_optim_clip_step_f32 (kind Adam)"), results[1:]):
        for what, a_list, b_list in zip(("param", "grad", "exp_avg", "exp_avg_sq"), results[0][:4], res[:4]):
            for k, (a, b) in enumerate(zip(a_list, b_list)):
                same_bits(a, b, "%s: %s %d, by value against %s" % (tag, what, k, form))
        if mn > 0:
            same_bits(results[0][4], res[4], "%s: partial sums, by value against %s" % (tag, form))
            same_bits(results[0][5], res[5], "%s: norm, by value against %s" % (tag, form))
    # the step did something, and .grad is what clip_grad_norm_ leaves (or untouched)
    for k in range(len(sizes)):
        assert not torch.equal(results[0][0][k], original[0][k]) and not torch.equal(results[0][3][k], original[3][k]), tag
    if mn > 0:
        want = math.sqrt(sum(float((g.double() ** 2).sum()) for g in original[1]))
        assert abs(float(results[0][5][0]) - want) <= 1e-6 * want and want > 10.0, tag
    clipped = max_norm == "active" and write_clipped
    for k in range(len(sizes)):
        assert torch.equal(results[0][1][k], original[1][k]) != bool(clipped), tag + ": .grad"


def test_zz_ratio_report():
    """Not a check of its own: the err / Y table of the run (pytest -s), the source of R and of the table above."""
    worst = max(RATIOS.values()) if RATIOS else 0.0
    for k in sorted(RATIOS):
        print("REPORT %-60s %.2f" % (k, RATIOS[k]))
    print("REPORT worst err/Y %.2f over %d results; R = %g" % (worst, len(RATIOS), R_RATIO))
    assert worst <= R_RATIO
