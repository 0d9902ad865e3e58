"""PSIS-LOO without a GPU: an independent numpy/scipy restatement of Pareto-smoothed importance-sampling LOO (Vehtari, Simpson, Gelman,
Yao & Gabry 2024; the generalised Pareto fit of Zhang & Stephens 2009) checked against known answers and its edge cases, finalize()
against it, the comparison tool's --criterion loo rules, and the C ABI's argument validation."""
import ctypes as C
import math

import numpy as np
import pytest
from scipy import stats

from pyhillfit_amd import compare_models as cm
from pyhillfit_amd import loo

EPS = np.finfo(float).eps


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def tail_length(S):
    return math.ceil(min(S / 5.0, 3.0 * math.sqrt(S)))


def _seq_sum(a):
    """left-to-right sum (the device's order)"""
    return float(np.cumsum(a)[-1]) if len(a) else 0.0


def gpd_fit(x):
    """Zhang & Stephens (2009) for ascending exceedances x: 30 + floor(sqrt n) grid points, prior constant 3, first-quartile anchor,
    profile-likelihood weights (those below 10 eps dropped), then k <- (n k + 5)/(n + 10).  -> (k, sigma), sigma from the unadjusted k"""
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    m = 30 + int(math.sqrt(n))
    xs = x[int(n / 4.0 + 0.5) - 1]
    if xs == 0.0:
        xs = x[x > 0][0]                                             # over a quarter ties with the cutoff: the smallest positive one
    b = 1.0 / x[-1] + (1.0 - np.sqrt(m / (np.arange(m) + 0.5))) / (3.0 * xs)
    kk = np.array([_seq_sum(np.log1p(-bj * x)) for bj in b]) / n
    lik = n * (np.log(-b / kk) - kk - 1.0)
    with np.errstate(over="ignore"):                                    # an overflowing sum gives the weight 0, as on the device
        w = np.array([1.0 / _seq_sum(np.exp(lik - lj)) for lj in lik])
    keep = w >= 10 * EPS
    wsum = _seq_sum(np.where(keep, w, 0.0))
    bpost = _seq_sum(np.where(keep, b * (w / wsum), 0.0))
    kraw = float(np.mean(np.log1p(-bpost * x)))
    return (n * kraw + 5.0) / (n + 10.0), -kraw / bpost


def gpd_quantile(p, k, sigma):
    t = np.log1p(-p)
    return -sigma * t if k == 0.0 else sigma * np.expm1(-k * t) / k


def psis_loo(ll):
    """one point's S log-likelihoods -> dict(elpd, lppd, khat, sigma, tail (the M + 1 smallest, ascending))"""
    ll = np.asarray(ll, dtype=np.float64).ravel()
    S = ll.size
    M = tail_length(S)
    t = np.sort(ll)
    mx = t[-1]
    lppd = (mx + math.log(_seq_sum(np.exp(ll - mx)))) - math.log(S) if mx > -np.inf else -np.inf
    t0, tM = t[0], t[M]
    if t0 == -np.inf:                                                  # a draw with p(y | theta) = 0: infinite ratio
        return dict(elpd=-np.inf, lppd=lppd, khat=np.inf, sigma=np.nan, tail=t[:M + 1])
    wcut = math.exp(t0 - tM)
    W = np.exp(t0 - t[:M])                                             # descending: W[0] = 1, the largest ratio
    X = W - wcut
    if M >= 5 and X[0] > X[M - 1]:
        k, sigma = gpd_fit(X[::-1])
        j = np.arange(M)
        Wt = np.minimum(wcut + gpd_quantile((M - j - 0.5) / M, k, sigma), 1.0)
    else:
        k, sigma = (np.inf, np.nan) if M < 5 else (0.0, 0.0)
        Wt = W
    w_nt = float(np.sum(np.exp(t0 - t[M:])))
    cap = math.exp(0.75 * math.log(S)) * ((w_nt + np.sum(Wt)) / S)
    Wt = np.minimum(Wt, cap)
    num = (S - M) + np.sum(np.exp(np.log(Wt) + (t[:M] - t0)))
    elpd = (t0 + math.log(num)) - math.log(w_nt + np.sum(Wt))
    return dict(elpd=elpd, lppd=lppd, khat=k, sigma=sigma, tail=t[:M + 1])


def direct_loo_weights(ll):
    """plain (unsmoothed) importance-sampling LOO: elpd_i = -log mean exp(-l)"""
    return -(np.log(np.mean(np.exp(-(ll - ll.min())))) - ll.min())


# ---- known answers --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0.2, 0.5, 0.9])
def test_gpd_fit_recovers_k(k):
    """n = 20 000 draws of GPD(k, 1): the fit is within 0.05 of k (about 4 standard errors at k = 0.9) and sigma within 5 %"""
    x = np.sort(stats.genpareto.rvs(k, scale=1.0, size=20000, random_state=np.random.default_rng(int(k * 10))))
    kh, sh = gpd_fit(x)
    assert abs(kh - k) < 0.05, (kh, k)
    assert abs(sh - 1.0) < 0.05, sh


def test_psis_khat_of_pareto_ratios():
    """importance ratios exp(-l) with a GPD(0.5) tail: PSIS's k-hat sees it (the tail is the ratios' own upper 3 sqrt S)"""
    rng = np.random.default_rng(3)
    ratios = 1.0 + stats.genpareto.rvs(0.5, size=40000, random_state=rng)
    res = psis_loo(-np.log(ratios))
    assert abs(res["khat"] - 0.5) < 0.1, res["khat"]


def test_conjugate_normal_matches_analytic_loo():
    """y_i ~ N(theta, 1), theta ~ N(0, 10^2): elpd_loo_i against the exact leave-one-out predictive N(mu_-i, 1 + 1/tau_-i)"""
    rng = np.random.default_rng(7)
    n, S = 20, 40000
    y = rng.normal(1.5, 1.0, n)
    y[0] = 4.5                                                         # one influential point
    tau = 0.01 + n
    theta = rng.normal(np.sum(y) / tau, 1 / math.sqrt(tau), S)
    tau_i = 0.01 + n - 1
    mu_i = (np.sum(y) - y) / tau_i
    want = stats.norm.logpdf(y, mu_i, np.sqrt(1 + 1 / tau_i))
    got = np.array([psis_loo(stats.norm.logpdf(yi, theta, 1.0))["elpd"] for yi in y])
    khat = np.array([psis_loo(stats.norm.logpdf(yi, theta, 1.0))["khat"] for yi in y])
    assert np.all(khat < 0.7)
    np.testing.assert_allclose(got, want, atol=0.02)
    assert abs(np.sum(got) - np.sum(want)) < 0.1
    # plain importance sampling agrees with PSIS where k-hat is small
    np.testing.assert_allclose(got, [direct_loo_weights(stats.norm.logpdf(yi, theta, 1.0)) for yi in y], atol=0.02)


def test_equal_ratios_give_lppd_exactly():
    for S, v in ((10, -3.25), (1000, 0.7), (12345, -41.0)):
        res = psis_loo(np.full(S, v))
        assert res["elpd"] == res["lppd"]
        assert res["khat"] == (np.inf if tail_length(S) < 5 else 0.0)


# ---- edge cases -----------------------------------------------------------------------------------------------------------------
def test_tail_length_rule():
    assert [tail_length(S) for S in (2, 10, 20, 21, 100, 225, 226, 1000, 4800064)] == [1, 2, 4, 5, 20, 45, 46, 95, 6573]


def test_short_tail_is_not_fitted():
    """M < 5 (S <= 20): k-hat = +inf, sigma = NaN, the raw ratios (truncated) give elpd_loo"""
    ll = np.random.default_rng(1).normal(-2.0, 0.5, 20)
    res = psis_loo(ll)
    assert tail_length(20) == 4 and res["khat"] == np.inf and np.isnan(res["sigma"])
    S = ll.size
    w = np.exp(-(ll - ll.min()))
    cap = S ** 0.75 * w.mean()
    assert np.all(w <= cap)                                             # nothing truncated here
    want = math.log(S) - math.log(np.sum(w)) + ll.min()
    assert res["elpd"] == pytest.approx(want, rel=1e-13)
    res21 = psis_loo(np.random.default_rng(2).normal(-2.0, 0.5, 21))    # S/5 binds and M = 5: fitted
    assert np.isfinite(res21["khat"]) and res21["sigma"] > 0


def test_equal_tail_is_not_smoothed():
    """the M smallest l all equal (above or at the cutoff): the exceedances are all equal, nothing to fit: k-hat = 0, sigma = 0"""
    S = 400
    M = tail_length(S)
    ll = np.concatenate([np.full(M, -5.0), np.linspace(-1.0, 0.0, S - M)])
    res = psis_loo(ll)
    assert res["khat"] == 0.0 and res["sigma"] == 0.0
    w = np.exp(-(ll - ll.min()))
    assert res["elpd"] == pytest.approx(math.log(S) - math.log(np.sum(w)) + ll.min(), rel=1e-12)


def test_minus_inf_draw():
    """sigma <= 1e-3 gives l = -inf: an infinite ratio, elpd_loo_i = -inf, k-hat = +inf"""
    ll = np.random.default_rng(4).normal(-2.0, 0.5, 500)
    ll[17] = -np.inf
    res = psis_loo(ll)
    assert res["elpd"] == -np.inf and res["khat"] == np.inf and np.isnan(res["sigma"])
    assert np.isfinite(res["lppd"])


def test_quartile_ties_with_cutoff():
    """over a quarter of the tail tied with the cutoff (repeated MCMC values): the smallest positive exceedance anchors the grid"""
    rng = np.random.default_rng(9)
    S = 2000
    M = tail_length(S)
    ll = np.concatenate([np.full(M // 2 + 1, -3.0), rng.uniform(-3.0, 0.0, S - M // 2 - 1)])
    ll[:20] = rng.uniform(-9.0, -3.5, 20)
    res = psis_loo(ll)
    assert np.isfinite(res["khat"]) and np.isfinite(res["elpd"])


# ---- finalize -------------------------------------------------------------------------------------------------------------------
def test_finalize_against_restatement():
    rng = np.random.default_rng(12)
    S = 3000
    ll = rng.normal(-2.0, 0.6, (7, S))
    ll[3] = -np.log(1.0 + stats.genpareto.rvs(0.9, size=S, random_state=rng))    # a heavy-tailed point
    rs = [psis_loo(x) for x in ll]
    f = loo.finalize([r["elpd"] for r in rs], [r["lppd"] for r in rs], [r["khat"] for r in rs], [r["sigma"] for r in rs], [1.0] * 7, S)
    e = np.array([r["elpd"] for r in rs])
    assert f["elpd_loo"] == pytest.approx(e.sum(), rel=1e-14)
    assert f["se_elpd_loo"] == pytest.approx(math.sqrt(7 * np.var(e, ddof=1)), rel=1e-12)
    assert f["looic"] == pytest.approx(-2 * e.sum(), rel=1e-14)
    assert f["p_loo"] == pytest.approx(sum(r["lppd"] - r["elpd"] for r in rs), rel=1e-12)
    thr = min(1 - 1 / math.log10(S), 0.7)
    assert f["khat_threshold"] == thr
    assert f["n_khat_above_threshold"] == sum(r["khat"] > thr for r in rs) >= 1
    assert f["n_khat_above_1"] == sum(r["khat"] > 1 for r in rs)
    assert f["max_khat"] == max(r["khat"] for r in rs) and f["n_undetermined"] == 0
    g = loo.finalize(e, e, np.zeros(7), np.zeros(7), [1, 1, 0, 1, 1, 1, 1], S)
    assert g["n_undetermined"] == 1 and np.isnan(g["elpd_loo"]) and np.isnan(g["se_elpd_loo"])
    rec = loo.json_record(dict(g, elpd_loo_i=np.where(np.arange(7) == 2, np.nan, e)), _points(7), 0)
    assert rec["elpd_loo"] is None and rec["pointwise"]["elpd_loo"][2] is None and rec["pointwise"]["determined"][2] is False


def test_khat_threshold():
    assert loo.khat_threshold(100) == pytest.approx(0.5)
    assert loo.khat_threshold(10 ** 6) == 0.7
    assert loo.khat_threshold(1000) == pytest.approx(1 - 1 / 3)


# ---- comparison -----------------------------------------------------------------------------------------------------------------
class _P(object):
    def __init__(self, n, kinds=None):
        self.info = [[(1, float(i + 1), 50.0, (kinds or ["uncensored"] * n)[i]) for i in range(n)]]


def _points(n, kinds=None):
    return _P(n, kinds)


def _loo_obj(elpd, khat, kinds=None, S=4000):
    n = len(elpd)
    f = loo.finalize(np.array(elpd, dtype=float), np.array(elpd, dtype=float) + 0.1, np.array(khat, dtype=float), np.ones(n),
                     [0.0 if e is None or (isinstance(e, float) and np.isnan(e)) else 1.0 for e in elpd], S)
    return loo.json_record(f, _points(n, kinds), 0)


def test_compare_loo_rules():
    a = _loo_obj([-1.0, -2.0, -1.5, -0.5], [0.1, 0.2, 0.3, 0.1])
    b = _loo_obj([-1.5, -2.5, -2.0, -1.2], [0.1, 0.8, 0.3, 0.1])
    r = cm.compare(a, b, criterion="loo")
    d = np.array([0.5, 0.5, 0.5, 0.7])
    assert r["elpd_diff"] == pytest.approx(d.sum()) and r["se_diff"] == pytest.approx(math.sqrt(4 * np.var(d, ddof=1)))
    assert r["preferred"] == "A" and r["n_khat_a"] == 0 and r["n_khat_b"] == 1 and r["khat_flagged"] is True
    assert cm.compare(a, a, criterion="loo")["khat_flagged"] is False
    und = _loo_obj([-1.0, float("nan"), -1.5, -0.5], [0.1, 0.2, 0.3, 0.1])
    assert "error" in cm.compare(a, und, criterion="loo") and "not determined" in cm.compare(und, a, criterion="loo")["error"]
    short = _loo_obj([-1.0, -2.0, -1.5], [0.1, 0.2, 0.3])
    assert "point sets differ" in cm.compare(a, short, criterion="loo")["error"]
    assert cm.compare(a, short, intersection=True, criterion="loo")["n_points"] == 3
    cens = _loo_obj([-1.0, -2.0, -1.5, -0.5], [0.1, 0.2, 0.3, 0.1], kinds=["censored-0", "uncensored", "uncensored", "censored-100"])
    r = cm.compare(a, cens, criterion="loo")
    assert r["n_mixed"] == 2 and "warning" in r


def test_compare_waic_unchanged_by_criterion():
    """the default criterion reads "waic" and adds no loo keys"""
    w = {"pointwise": {"elpd": [-1.0, -2.0, -3.0]}, "points": {"experiment": [1, 1, 1], "dose": [1.0, 2.0, 3.0], "response": [5.0, 6.0, 7.0],
                                                             "kind": ["uncensored"] * 3}}
    v = {"pointwise": {"elpd": [-1.5, -2.0, -3.5]}, "points": w["points"]}
    r = cm.compare(w, v)
    assert set(r) == {"n_points", "n_only_a", "n_only_b", "elpd_a", "elpd_b", "elpd_diff", "se_diff", "preferred", "n_mixed"}


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from pyhillfit_amd import _lib
    return _lib.load()


def test_abi_validation(lib):
    assert lib.phf_psis_tail_length(65, 100) == tail_length(6500) == 242
    assert lib.phf_psis_tail_length(64, 75001) == 6573
    # the default: k = min(M + 1, total_rows), every point exact, while the workspace fits 32 GiB
    assert lib.phf_psis_tail_per_chain(3, 7, 65, 100, 0) == 100              # total_rows < M + 1 = 243
    assert lib.phf_psis_tail_per_chain(210, 20, 64, 75001, 0) == 6574        # the single-level CLI shape: 14.1 GB
    assert lib.phf_psis_tail_per_chain(3, 7, 65, 1000, 5000) == 766          # a request is capped at M + 1
    assert lib.phf_psis_tail_per_chain(1, 1, 1, 10, 0) == 3
    assert lib.phf_psis_tail_per_chain(210, 20, 4096, 75001, 0) == 2 * math.ceil(52583 / 4096) + 32   # C3's shape: over the budget
    assert lib.phf_psis_workspace_bytes(3, 7, 65, 100, 0) == (3 * 7 * (6 + 100) * 65 + 21) * 8
    assert lib.phf_psis_workspace_bytes(3, 7, 65, 100, 10) == (3 * 7 * (6 + 10) * 65 + 21) * 8
    big = lib.phf_psis_tail_length(4096, 75001)                              # C3's chains: the sort goes to HBM scratch
    p2 = 1 << (big + 1 - 1).bit_length()
    assert lib.phf_psis_tail_per_chain(2, 3, 4096, 75001, 0) == big + 1
    assert lib.phf_psis_workspace_bytes(2, 3, 4096, 75001, 0) == (2 * 3 * (6 + big + 1) * 4096 + 6 + 6 * 2 * p2) * 8
    assert lib.phf_psis_workspace_bytes(2, 3, 4096, 75001, 58) == (2 * 3 * (6 + 58) * 4096 + 6 + 6 * 2 * p2) * 8
    for bad in ((0, 7, 65, 100, 0), (3, 0, 65, 100, 0), (3, 7, 0, 100, 0), (3, 7, 65, 0, 0), (3, 7, 1, 1, 0), (3, 7, 65, 100, -1),
                (3, 7, 65, 100, 3)):                                      # 3 x 65 < M + 1
        assert lib.phf_psis_workspace_bytes(*bad) == 0
        assert lib.phf_last_error()
    assert lib.phf_psis_tail_length(1, 1) == 0 and b"at least 2" in lib.phf_last_error()
    assert lib.phf_psis_workspace_bytes(3, 7, 65, 100, 3) == 0 and b"M + 1" in lib.phf_last_error()
    with pytest.raises(ValueError):
        loo.workspace_bytes(1, 1, 1, 0)
    with pytest.raises(ValueError):
        loo.tail_length(1, 1)
    assert lib.phf_psis_init(3, 7, 65, 100, 0, None, C.c_size_t(1 << 20), None) == -1 and b"null" in lib.phf_last_error()
    assert lib.phf_psis_init(3, 7, 65, 100, 0, C.c_void_p(8), C.c_size_t(16), None) == -1 and b"smaller" in lib.phf_last_error()
    from pyhillfit_amd._lib import PointwisePoints
    p = PointwisePoints(2, 4, 8, 8, 8, 8)
    fake, huge = C.c_void_p(8), C.c_size_t(1 << 34)
    assert lib.phf_psis_reduce(C.byref(p), 2, 64, 10, 0, fake, C.c_size_t(16), fake, None, None) == -1 and b"smaller" in lib.phf_last_error()
    assert lib.phf_psis_reduce(C.byref(p), 2, 64, 10, 0, fake, huge, None, None, None) == -1 and b"null" in lib.phf_last_error()
    assert lib.phf_psis_reduce(C.byref(p), 3, 64, 10, 0, fake, huge, fake, None, None) == -1 and b"one row per problem" in lib.phf_last_error()
    args = lambda **kw: [kw.get(k, v) for k, v in (("pts", C.byref(p)), ("lik", 2), ("ne", 0), ("rows", fake), ("n", 10), ("Q", 2),
                                                   ("stride", 4), ("C", 64), ("first", 0), ("total", 10), ("k", 0), ("ws", fake),
                                                   ("wsb", huge), ("s", None))]
    assert lib.phf_psis_accumulate(*args(lik=4)) == -1 and b"likelihood" in lib.phf_last_error()
    assert lib.phf_psis_accumulate(*args(lik=3)) == -1 and b"num_expts" in lib.phf_last_error()
    assert lib.phf_psis_accumulate(*args(lik=3, ne=2)) == -1 and b"row_stride_cols" in lib.phf_last_error()
    assert lib.phf_psis_accumulate(*args(stride=2)) == -1 and b"row_stride_cols" in lib.phf_last_error()
    assert lib.phf_psis_accumulate(*args(first=5)) == -1 and b"total_rows" in lib.phf_last_error()
    assert lib.phf_psis_accumulate(*args(Q=3)) == -1 and b"one row per problem" in lib.phf_last_error()
    assert lib.phf_psis_accumulate(*args(wsb=C.c_size_t(8))) == -1 and b"smaller" in lib.phf_last_error()
    assert lib.phf_psis_accumulate(*args(rows=None)) == -1 and b"null" in lib.phf_last_error()
    assert lib.phf_psis_accumulate(*args(pts=None)) == -1 and b"null points" in lib.phf_last_error()
    assert lib.phf_psis_accumulate(*args(k=-2)) == -1 and b"tail_per_chain" in lib.phf_last_error()
    assert lib.phf_psis_accumulate(*args(n=0, first=10)) == 0                # nothing to do: no launch
