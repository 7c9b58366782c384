"""ptt_step_ledger_f32 alone (ptt_amd/csrc/step_ops.hip) and ptt_amd.fit.StepLedger on top of it: a ring of capacity 4 that
wraps twice and ends mid-ring, a NaN and an infinity among the rows, the NULL-norm form, guard words around ring and state.
Every comparison is on bits or `==`: the kernel copies values and adds them in a fixed order."""
import numpy as np
import pytest
import torch

from tests import guard

pytestmark = pytest.mark.gpu
CAP, N, COLS = 4, 11, 6


def _rows():
    rs = np.random.RandomState(1234)
    rows = (rs.standard_normal((N, COLS)) * np.array([3.0, 1.0, 0.5, 1.0, 0.25, 10.0])).astype(np.float32)
    rows[:, 5] = np.abs(rows[:, 5])
    rows[3, 2] = np.nan
    rows[7, 5] = np.inf
    return rows


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _state(dev):
    ring = guard.guarded((CAP, COLS), torch.float32, device=dev)
    counts = guard.guarded((2,), torch.int64, device=dev)
    sums = guard.guarded((COLS,), torch.float64, device=dev)
    counts.zero_()
    sums.zero_()
    return ring, counts, sums


@pytest.mark.parametrize("with_norm", [True, False])
def test_append_ring_counters_and_sums(dev, with_norm):
    from ptt_amd import ops
    rows = _rows()
    # what the step hands over: the (8,) buffer of the one-launch losses (three more floats behind the five) and a (1,) norm
    out8 = torch.from_numpy(np.concatenate([rows[:, :5], np.full((N, 3), 77.0, np.float32)], axis=1)).to(dev)
    norms = torch.from_numpy(rows[:, 5:6].copy()).to(dev)
    expect = rows.copy()
    if not with_norm:
        expect[:, 5] = 0.0
    ring, counts, sums = _state(dev)
    sentinel = np.full((CAP, COLS), guard.SENTINEL, np.int32)
    want = sentinel.copy()
    for k in range(N):
        ops.step_ledger(out8[k], norms[k] if with_norm else None, ring, counts, sums)
        torch.cuda.synchronize()
        want[k % CAP] = _bits(expect[k])
        got = ring.cpu().numpy().view(np.int32)
        assert np.array_equal(got, want), (k, got, want)       # slot k % 4 holds row k bit for bit, the others are unchanged
        assert int(counts[0]) == k + 1
    bad = [k for k in range(N) if not np.isfinite(expect[k]).all()]
    assert bad == ([3, 7] if with_norm else [3])
    assert counts.cpu().tolist() == [N, len(bad)]
    s = np.zeros(COLS, np.float64)
    for k in range(N):
        if k not in bad:
            for c in range(COLS):
                s[c] += np.float64(expect[k, c])
    got = sums.cpu().numpy()
    assert all(got[c] == s[c] for c in range(COLS)), (got, s)
    for v in (ring, counts, sums):
        guard.check_guard(v)


def test_refused_launches_write_nothing(dev):
    from ptt_amd import ops
    ring, counts, sums = _state(dev)
    before = (counts.clone(), sums.clone())
    vals = torch.ones(8, device=dev)
    P = guard.ptr
    with pytest.raises(RuntimeError, match="PTT_EINVAL.*capacity=0"):
        ops._launch("ptt_step_ledger_f32", dev, P(vals), P(None), P(ring), 0, P(counts), P(sums))
    with pytest.raises(RuntimeError, match="PTT_EINVAL.*null losses"):
        ops._launch("ptt_step_ledger_f32", dev, P(None), P(None), P(ring), CAP, P(counts), P(sums))
    torch.cuda.synchronize()
    guard.assert_untouched(ring)
    assert torch.equal(counts, before[0]) and torch.equal(sums, before[1])
    guard.check_guard(counts)
    guard.check_guard(sums)
    with pytest.raises(ValueError):
        ops.step_ledger(vals[:4], None, ring, counts, sums)      # fewer than five loss values


def test_fetch_summary_reset(dev):
    from ptt_amd.fit import StepLedger
    rows = _rows()
    out8 = torch.from_numpy(np.concatenate([rows[:, :5], np.zeros((N, 3), np.float32)], axis=1)).to(dev)
    norms = torch.from_numpy(rows[:, 5:6].copy()).to(dev)
    led = StepLedger(dev, capacity=CAP)
    k = 0
    for n, dropped in ((3, 0), (2, 0), (6, 2)):
        for _ in range(n):
            led.append(out8[k], norms[k])
            k += 1
        got, d = led.fetch()
        kept = n - dropped
        assert d == dropped and got.shape == (kept, COLS) and got.dtype == np.float32
        assert np.array_equal(_bits(got), _bits(rows[k - kept:k])), (n, got)
    assert led.fetch()[0].shape == (0, COLS) and led.queued == N
    s = led.summary()
    finite = [r for r in rows if np.isfinite(r).all()]
    assert s['steps'] == N and s['non_finite'] == 2
    mean0 = np.float64(0.0)
    for r in finite:
        mean0 += np.float64(r[0])
    assert s['mean']['loss'] == float(mean0 / np.float64(len(finite)))
    led.reset()
    torch.cuda.synchronize()
    assert led.counts.cpu().tolist() == [N, 0] and not led.sums.cpu().numpy().any()
    s = led.summary()
    assert s['steps'] == 0 and s['non_finite'] == 0 and np.isnan(s['mean']['loss'])
    led.append(out8[0], None)
    s = led.summary()
    assert s['steps'] == 1 and s['mean']['loss'] == float(np.float64(rows[0, 0])) and s['mean']['grad_norm'] == 0.0
    got, d = led.fetch()
    assert d == 0 and np.array_equal(_bits(got), _bits(np.concatenate([rows[0, :5], [0.0]])[None]))
