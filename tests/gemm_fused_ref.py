"""Float64 reference of ptt_rows_gemm_bnbwd_fused_f32 (include/ptt_hip.h, "Round 5: the BatchNorm + ReLU backward of a layer
APPLIED BY ITS CONSUMER"), written from the header's formulas; plain torch on the host. Nothing here reads a kernel or
ptt_amd/ops.py.

    dz   = c0 + c1 * (z - mean) + (mask ? k1 * g_row : 0)       mask = z * act_a + act_b > 0, pooled: and arg[row // ns, ch] == row % ns
    out  = dz @ w.T
    dy   = out where zp * ap + bp > 0, else 0
    sums = [dy.sum(0), (dy * (zp - mp) * ip).sum(0)]

case() makes operands whose two ReLU masks are EXACT: z / zp and act_b / bp lie on a 2^-8 grid within +-8, act_a / ap are powers of
two between 0.25 and 2 of either sign, so z * a + b is the same number in float32 (with or without fma) and in float64 — the
module asserts that for what it returns. On top of that, at least 1 % of the elements of each mask are PLANTED exact zeros of
z * a + b where the gradient that the mask gates is not zero (rows 0, rows - 1 and the first row of the last row tile among them):
a `>=` in place of the strict `>` changes the result there by a whole k1 * g (or a whole `out`), not by a rounding.

tests/test_gemm_fused_ref_cpu.py anchors reference() to torch.autograd."""
import torch

F32, F64, I32 = torch.float32, torch.float64, torch.int32
GRID = 256                  # z, zp, act_b, bp = an integer / GRID
PLANT = 0.02                # the share of planted mask zeros aimed at (at least 0.01 is asserted)
C1_ZERO = slice(1, None, 13)        # channels whose c1 is 0: where the mask is off, dz == c0 bit for bit


def tile_rows(K, N):
    """Rows of a row tile of the geometry the launch takes for (K, N): 64 when K % 128 == 0 and N % 128 == 0, else 128."""
    return 64 if K % 128 == 0 and N % 128 == 0 else 128


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _grid(shape, lim, g):
    return torch.randint(-lim * GRID, lim * GRID + 1, shape, generator=g).to(F32) / GRID


def _mask_consts(C, g):
    """(a, b, t): a from {+-0.25, +-0.5, +-1, +-2}; the threshold t on the 2^-6 grid within +-4, so that b = -a * t lies on the 2^-8
    grid within +-8 and z = t is an exact zero of z * a + b."""
    a = torch.tensor([0.25, 0.5, 1.0, 2.0])[torch.randint(0, 4, (C,), generator=g)] * (torch.randint(0, 2, (C,), generator=g) * 2 - 1).to(F32)
    t = torch.randint(-4 * 64, 4 * 64 + 1, (C,), generator=g).to(F32) / 64
    return a, -a * t, t


def _forced_rows(rows, TR):
    """The rows that must carry plants, each with the channel phase (c % 3) it gets: no two of them meet in one (group, channel)."""
    return [(0, 0), (rows - 1, 1), ((rows - 1) // TR * TR, 2)]


def exact_argument(z, a, b):
    """z * a + b in float64, after asserting that float32 forms the same number: the product and the sum are both exact."""
    p32, p64 = z * a, z.to(F64) * a.to(F64)
    assert torch.equal(p32.to(F64), p64), "z * a is rounded in float32"
    s32, s64 = p32 + b, p64 + b.to(F64)
    assert torch.equal(s32.to(F64), s64), "z * a + b is rounded in float32"
    return s64


def case(rows, K, N, ns, seed):
    """The operands of one launch, float32 unless said otherwise: z (rows,K), g (rows,K) or (rows/ns,K), arg int32 (rows/ns,K) in [0,ns)
    or None, mean / act_a / act_b / k1 / c0 / c1 (K,), w (N,K), zp (rows,N), mp / ip / ap / bp (N,); `upper` / `lower`: where the
    planted zeros of the two masks are (bool, (rows,K) / (rows,N)); `ref`: reference() of all this, computed once."""
    assert rows > 0 and (ns == 0 or rows % ns == 0)
    g_ = _gen(seed)
    TR = tile_rows(K, N)
    groups = rows // ns if ns else rows
    z, zp = _grid((rows, K), 8, g_), _grid((rows, N), 8, g_)
    act_a, act_b, t = _mask_consts(K, g_)
    ap, bp, tp = _mask_consts(N, g_)
    g = torch.randn(groups, K, generator=g_)
    arg = torch.randint(0, ns, (groups, K), generator=g_, dtype=I32) if ns else None
    sign = lambda n: (torch.randint(0, 2, (n,), generator=g_) * 2 - 1).to(F32)
    mean, k1 = torch.randn(K, generator=g_) * 0.5, (torch.rand(K, generator=g_) + 0.5) * sign(K)
    c0, c1 = torch.randn(K, generator=g_) * 0.5, torch.randn(K, generator=g_) * 0.1
    c1[C1_ZERO] = 0.0
    w = torch.randn(N, K, generator=g_) / K ** 0.5
    mp, ip = torch.randn(N, generator=g_) * 0.5, torch.rand(N, generator=g_) + 0.5
    # ---- the planted zeros of the staged mask: z = t there, and (pooled) the row is its group's arg-max
    upper = torch.zeros(rows, K, dtype=torch.bool)
    if ns:
        pg = torch.rand(groups, K, generator=g_) < min(0.8, PLANT * ns)
        rin = torch.randint(0, ns, (groups, K), generator=g_)
        for r, ph in _forced_rows(rows, TR):
            pg[r // ns, ph::3] = True
            rin[r // ns, ph::3] = r % ns
        arg = torch.where(pg, rin.to(I32), arg)
        gi, ci = torch.nonzero(pg, as_tuple=True)
        upper[gi * ns + rin[gi, ci], ci] = True
    else:
        upper = torch.rand(rows, K, generator=g_) < PLANT
        for r, ph in _forced_rows(rows, TR):
            upper[r, ph::3] = True
    z = torch.where(upper, t.expand(rows, K), z)
    # ---- the planted zeros of the epilogue's mask
    lower = torch.rand(rows, N, generator=g_) < PLANT
    for r, ph in _forced_rows(rows, TR):
        lower[r, ph::3] = True
    zp = torch.where(lower, tp.expand(rows, N), zp)
    c = dict(rows=rows, K=K, N=N, ns=ns, z=z, g=g, arg=arg, mean=mean, act_a=act_a, act_b=act_b, k1=k1, c0=c0, c1=c1, w=w, zp=zp, mp=mp,
             ip=ip, ap=ap, bp=bp, upper=upper, lower=lower)
    # ---- what the docstring promises, asserted for the data returned
    for x, lim in ((z, 8), (zp, 8), (act_b, 8), (bp, 8)):
        assert torch.equal((x * GRID).round(), x * GRID) and float(x.abs().max()) <= lim
    assert all(float(v) in (0.25, 0.5, 1.0, 2.0) for v in torch.cat([act_a, ap]).abs().unique())
    assert bool((act_a < 0).any()) and bool((ap < 0).any())
    up_arg, lo_arg = exact_argument(z, act_a, act_b), exact_argument(zp, ap, bp)
    assert bool((up_arg[upper] == 0).all()) and bool((lo_arg[lower] == 0).all())
    ref = c["ref"] = reference(c)
    live_up = upper & (ref["g_rows"] != 0) & (k1 != 0) & ref["is_arg"]
    live_lo = lower & (ref["out"] != 0)
    assert int(live_up.sum()) >= 0.01 * rows * K and int(live_lo.sum()) >= 0.01 * rows * N, "fewer than 1 % planted zeros"
    for r, _ in _forced_rows(rows, TR):
        assert bool(live_up[r].any()) and bool(live_lo[r].any()), "row %d carries no planted zero" % r
    return c


def reference(c):
    """-> dict of float64 tensors: dz (rows,K), out (rows,N), dy (rows,N), sums (2,N); and the booleans mask (the staged mask,
    (rows,K)), is_arg (pooled: the row is its group's arg-max; dense: all True), g_rows (the gradient of every row, (rows,K))."""
    d = lambda k: c[k].to(F64)
    z, zp, ns = d("z"), d("zp"), int(c["ns"])
    rows = z.shape[0]
    if ns:
        r = torch.arange(rows)
        g_rows = d("g")[r // ns]
        is_arg = c["arg"].long()[r // ns] == (r % ns).unsqueeze(1)
    else:
        g_rows, is_arg = d("g"), torch.ones_like(z, dtype=torch.bool)
    mask = (z * d("act_a") + d("act_b") > 0) & is_arg
    t = d("c0") + d("c1") * (z - d("mean"))
    dz = torch.where(mask, t + d("k1") * g_rows, t)
    out = dz @ d("w").t()
    dy = torch.where(zp * d("ap") + d("bp") > 0, out, torch.zeros_like(out))
    sums = torch.stack([dy.sum(0), (dy * (zp - d("mp")) * d("ip")).sum(0)])
    return dict(dz=dz, out=out, dy=dy, sums=sums, mask=mask, is_arg=is_arg, g_rows=g_rows)
