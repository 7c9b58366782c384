"""tests/gemm_fused_ref.py against its definition: the constants k1, c0, c1 of include/ptt_hip.h ("Round 5", dbeta = sum dy,
dgamma = sum dy * xhat) put into reference() must give the gradients torch.autograd gives for

    zp -> relu(batch_norm(zp)) -> @ W^T -> z -> relu(batch_norm(z)) [-> max over groups of ns rows] -> sum(. * G)

in float64 on ordinary random data: dz = d loss / d z, out = d loss / d relu(batch_norm(zp)), and sums = the gradients of the lower
BatchNorm's beta and gamma. No kernel takes part."""
import pytest
import torch
import torch.nn.functional as F

from tests import gemm_fused_ref as R

F64 = torch.float64
EPS = 1e-5


def chain(rows, K, N, ns, seed):
    g_ = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g_, dtype=F64)
    zp = rnd(rows, N).requires_grad_(True)
    gam_l, bet_l = (rnd(N) * 0.3 + 1).requires_grad_(True), (rnd(N) * 0.2).requires_grad_(True)
    wf = (rnd(K, N) / N ** 0.5)                                        # the layer's forward weight; the input gradient multiplies by it
    gam, bet = rnd(K) * 0.3 + 1, rnd(K) * 0.2
    gam[::5] *= -1                                                      # negative act_a
    xp = torch.relu(F.batch_norm(zp, None, None, gam_l, bet_l, True, 0.0, EPS))
    xp.retain_grad()
    z = xp @ wf.t()
    z.retain_grad()
    y = torch.relu(F.batch_norm(z, None, None, gam, bet, True, 0.0, EPS))
    if ns:
        pooled, arg = y.view(rows // ns, ns, K).max(dim=1)
        G = rnd(rows // ns, K)
        (pooled * G).sum().backward()
    else:
        arg, G = None, rnd(rows, K)
        (y * G).sum().backward()
    return dict(zp=zp, gam_l=gam_l, bet_l=bet_l, wf=wf, gam=gam, bet=bet, xp=xp, z=z, G=G, arg=arg)


def stats(x):
    var, mean = torch.var_mean(x, 0, unbiased=False)
    return mean, 1.0 / torch.sqrt(var + EPS)


@pytest.mark.parametrize("rows,K,N,ns", [(37, 12, 20, 0), (48, 8, 12, 16), (96, 12, 8, 32), (128, 4, 8, 64)])
def test_reference_is_the_gradient_autograd_gives(rows, K, N, ns):
    t = chain(rows, K, N, ns, 7 * rows + ns)
    z, zp = t["z"].detach(), t["zp"].detach()
    mean, invstd = stats(z)
    act_a = t["gam"] * invstd
    act_b = t["bet"] - mean * act_a
    xhat = (z - mean) * invstd
    live = z * act_a + act_b > 0
    if ns:
        r = torch.arange(rows)
        dy = torch.where(live & (t["arg"][r // ns] == (r % ns).unsqueeze(1)), t["G"][r // ns], torch.zeros_like(z))
    else:
        dy = torch.where(live, t["G"], torch.zeros_like(z))
    dbeta, dgamma = dy.sum(0), (dy * xhat).sum(0)
    k1 = t["gam"] * invstd                                              # ptt_hip.h: k1 = gamma * invstd,
    c1 = -k1 * invstd * dgamma / rows                                   # c1 = -k1 * invstd * dgamma / R,
    c0 = -k1 * dbeta / rows                                             # c0 = -k1 * dbeta / R
    mp, ip = stats(zp)
    ap = t["gam_l"].detach() * ip
    bp = t["bet_l"].detach() - mp * ap
    c = dict(rows=rows, K=K, N=N, ns=ns, z=z, g=t["G"], arg=t["arg"].int() if ns else None, mean=mean, act_a=act_a, act_b=act_b, k1=k1, c0=c0,
             c1=c1, w=t["wf"].t().contiguous(), zp=zp, mp=mp, ip=ip, ap=ap, bp=bp)
    ref = R.reference(c)
    close = lambda got, want: float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert close(ref["dz"], t["z"].grad)
    assert close(ref["out"], t["xp"].grad)
    assert close(ref["sums"][0], t["bet_l"].grad)                       # dbeta of the layer below
    assert close(ref["sums"][1], t["gam_l"].grad)                       # dgamma of the layer below
    assert ref["dz"].dtype == F64 and ref["sums"].shape == (2, N)


@pytest.mark.parametrize("rows,K,N,ns", [(17, 128, 128, 0), (197, 256, 128, 0), (389, 128, 64, 0), (5 * 16, 128, 128, 16), (3 * 32, 256, 128, 32),
                                         (3 * 64, 64, 64, 64)])
def test_case_data_is_exact_and_planted(rows, K, N, ns):
    """case() asserts its own promises; here the ones a reader would otherwise take on trust are restated on what it returned, and
    the planted zeros are shown to matter: `>=` in place of `>` in either mask moves the reference by far more than any bound."""
    c = R.case(rows, K, N, ns, seed=rows + K + N + ns)
    ref = c["ref"]
    assert c["z"].dtype == torch.float32 and c["z"].shape == (rows, K) and c["zp"].shape == (rows, N) and c["w"].shape == (N, K)
    assert c["g"].shape == ((rows // ns if ns else rows), K) and ((c["arg"] is None) == (ns == 0))
    if ns:
        assert c["arg"].dtype == torch.int32 and int(c["arg"].min()) >= 0 and int(c["arg"].max()) < ns
    up = R.exact_argument(c["z"], c["act_a"], c["act_b"])
    lo = R.exact_argument(c["zp"], c["ap"], c["bp"])
    TR = R.tile_rows(K, N)
    for r in (0, rows - 1, (rows - 1) // TR * TR):
        assert bool((c["upper"][r] & (up[r] == 0) & ref["is_arg"][r]).any()) and bool((c["lower"][r] & (lo[r] == 0)).any())
    assert bool((c["c1"] == 0).any()) and bool((~ref["mask"][:, c["c1"] == 0]).any())
    # the mutants: a mask that lets exact zeros through
    d = lambda k: c[k].double()
    t = d("c0") + d("c1") * (d("z") - d("mean"))
    dz_ge = torch.where((up >= 0) & ref["is_arg"], t + d("k1") * ref["g_rows"], t)
    moved = (dz_ge - ref["dz"]).abs() > 1e-5 * (1 + ref["dz"].abs())
    assert int(moved.sum()) >= 0.01 * rows * K
    dy_ge = torch.where(lo >= 0, ref["out"], torch.zeros_like(ref["out"]))
    terms = ref["dy"].abs().sum(0).max()
    assert float((dy_ge.sum(0) - ref["sums"][0]).abs().max()) > 1e-3 * float(terms)
    again = R.case(rows, K, N, ns, seed=rows + K + N + ns)
    assert all(torch.equal(c[k], again[k]) for k in ("z", "g", "zp", "w", "k1", "c0", "c1"))
