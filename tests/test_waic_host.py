"""WAIC without a GPU: an independent numpy/scipy restatement of the pointwise log-likelihoods (checked against hand values and
the sum identities), finalize() against a direct WAIC of a full draw matrix and known answers, the comparison tool's arithmetic,
refusal and flagging, and the C ABI's argument validation."""
import ctypes as C
import math

import numpy as np
import pytest
from scipy.special import expit, log_ndtr, logsumexp

from pyhillfit_amd import compare_models as cm
from pyhillfit_amd import waic as wc

HALF_LN_2PI = 0.5 * math.log(2 * math.pi)


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def _pred(conc, pic50, hill):
    """percent block 100 (1 - 1/(1 + (c/IC50)^h)) with IC50 = 10^(6 - pIC50) uM, in the logistic form"""
    a = hill * (np.log(conc) - math.log(10.0) * (6.0 - pic50))
    return 100.0 * expit(np.minimum(a, 40.0))


def sl_loglik(model, conc, y, theta):
    """single-level pointwise log-likelihood of the points (conc, y), all in [0, 100], at theta = (pIC50[, Hill], sigma)"""
    conc, y = np.asarray(conc, dtype=np.float64), np.asarray(y, dtype=np.float64)
    pic50, hill, sigma = theta[0], (1.0 if model == 1 else theta[1]), theta[-1]
    if sigma <= 1e-3:
        return np.full(y.shape, -np.inf)
    pred = _pred(conc, pic50, hill)
    unc = -HALF_LN_2PI - math.log(sigma) - (y - pred) ** 2 / (2 * sigma ** 2)
    return np.where(y == 0, log_ndtr(-pred / sigma), np.where(y == 100, log_ndtr((pred - 100) / sigma), unc))


def hier_loglik(conc, y, expt, theta):
    """hierarchical pointwise log-likelihood (truncated normal on [0, 100]); expt: each point's experiment index"""
    conc, y, expt = np.asarray(conc, dtype=np.float64), np.asarray(y, dtype=np.float64), np.asarray(expt)
    ne = (len(theta) - 5) // 2
    sigma = theta[4 + 2 * ne]
    if sigma <= 1e-3:
        return np.full(y.shape, -np.inf)
    pred = _pred(conc, np.asarray(theta)[4 + 2 * expt], np.asarray(theta)[5 + 2 * expt])
    erfc = np.vectorize(math.erfc)
    mass = 1.0 - 0.5 * (erfc((100 - pred) / sigma / math.sqrt(2)) + erfc(pred / sigma / math.sqrt(2)))     # Phi(b) - Phi(a)
    return -HALF_LN_2PI - math.log(sigma) - (y - pred) ** 2 / (2 * sigma ** 2) - np.log(mass)


def reference_sl_loglik(model, conc, y, theta):
    """the reference's t = 1 single-level likelihood (doseresponse.py:203-248): pi_bit = n_total ln(2 pi)/2 over ALL points,
    the points outside [0, 100] included"""
    conc, y = np.asarray(conc, dtype=np.float64), np.asarray(y, dtype=np.float64)
    pic50, hill, sigma = theta[0], (1.0 if model == 1 else theta[1]), theta[-1]
    pred = _pred(conc, pic50, hill)
    z0, z100, other = y == 0, y == 100, (0 < y) & (y < 100)
    pi_bit = HALF_LN_2PI * len(y)
    return (np.sum(log_ndtr(-pred[z0] / sigma)) + np.sum(log_ndtr((pred[z100] - 100) / sigma)) - pi_bit
            - other.sum() * math.log(sigma) - np.sum((y[other] - pred[other]) ** 2) / (2 * sigma ** 2))


def direct_waic(ll):
    """ll [S][n]: the textbook WAIC of a full draw matrix"""
    S = ll.shape[0]
    lppd = logsumexp(ll, axis=0) - math.log(S)
    p = np.var(ll, axis=0, ddof=1)
    elpd = lppd - p
    return lppd, p, elpd, math.sqrt(len(elpd) * np.var(elpd, ddof=1))


# ---- restatement against hand values and the identities ------------------------------------------------------------------------
def test_hand_values():
    ic50 = 10.0 ** (6 - 5.0)                         # pIC50 = 5: a concentration of 10 uM is the IC50, pred = 50
    assert sl_loglik(2, [ic50], [50.0], (5.0, 1.7, 1.0))[0] == pytest.approx(-HALF_LN_2PI, rel=1e-15)
    assert sl_loglik(1, [ic50], [60.0], (5.0, 4.0))[0] == pytest.approx(-HALF_LN_2PI - math.log(4.0) - 100 / 32, rel=1e-15)
    assert sl_loglik(2, [ic50], [0.0], (5.0, 3.0, 50.0))[0] == pytest.approx(-1.8410216450092636, rel=1e-14)       # ln Phi(-1)
    assert sl_loglik(2, [ic50], [100.0], (5.0, 3.0, 50.0))[0] == pytest.approx(-1.8410216450092636, rel=1e-14)
    assert sl_loglik(2, [ic50], [50.0], (5.0, 1.0, 1e-3))[0] == -np.inf
    th = (0.1, 0.2, 5.0, 0.3, 5.0, 1.3, 7.0, 0.5, 50.0)                 # Ne = 2; experiment 0 at its IC50: pred = 50, mass = Phi(1) - Phi(-1)
    want = -HALF_LN_2PI - math.log(50.0) - math.log(0.6826894921370859)
    assert hier_loglik([ic50], [50.0], [0], th)[0] == pytest.approx(want, rel=1e-14)
    assert hier_loglik([ic50], [0.0], [0], th)[0] == pytest.approx(want - 0.5, rel=1e-14)


def _pair(rng, n):
    conc = 10.0 ** rng.uniform(-3, 2, n)
    y = rng.uniform(-5, 110, n)
    y[rng.random(n) < 0.25] = 0.0
    y[rng.random(n) < 0.1] = 100.0
    return conc, y


@pytest.mark.parametrize("model", [1, 2])
def test_single_level_sum_identity(model):
    rng = np.random.default_rng(model)
    for _ in range(20):
        conc, y = _pair(rng, 17)
        theta = (rng.uniform(3, 8),) + ((rng.uniform(0.3, 3),) if model == 2 else ()) + (rng.uniform(0.5, 30),)
        keep = (y >= 0) & (y <= 100)                                    # the sampler drops the others
        pointwise = sl_loglik(model, conc[keep], y[keep], theta)
        n_unc = np.sum((y > 0) & (y < 100))
        assert np.sum(pointwise) == pytest.approx(reference_sl_loglik(model, conc, y, theta) + (len(y) - n_unc) * HALF_LN_2PI, rel=1e-12)


def test_hierarchical_sum_identity():
    """sum_ij l_ij = the reference's log_data_likelihood (PyHillFit.py:113-132) - N ln(2 pi)/2"""
    rng = np.random.default_rng(7)
    th = np.array([1.0, 3.0, 5.0, 0.2, 5.5, 1.1, 6.2, 0.7, 4.9, 1.9, 8.0])
    conc = 10.0 ** rng.uniform(-2, 2, 12)
    y = rng.uniform(0, 100, 12)
    expt = np.repeat([0, 1, 2], 4)
    sigma = th[-1]
    ref = 0.0
    for i in range(3):
        m = expt == i
        pred = _pred(conc[m], th[4 + 2 * i], th[5 + 2 * i])
        from scipy.stats import norm
        ref += np.sum(norm.logpdf(y[m], pred, sigma) - np.log(norm.cdf(100, pred, sigma) - norm.cdf(0, pred, sigma)))
    assert np.sum(hier_loglik(conc, y, expt, th)) == pytest.approx(ref, rel=1e-12)


# ---- finalize ------------------------------------------------------------------------------------------------------------------
def test_finalize_matches_direct_waic():
    rng = np.random.default_rng(3)
    ll = rng.normal(-3, 0.7, (400, 9)) - rng.uniform(0, 30, 9)
    lppd, p, elpd, se = direct_waic(ll)
    res = wc.finalize(logsumexp(ll, axis=0), np.var(ll, axis=0, ddof=1), ll.shape[0])
    np.testing.assert_allclose(res["lppd_i"], lppd, rtol=1e-14)
    np.testing.assert_allclose(res["p_waic_i"], p, rtol=1e-14)
    assert res["elpd_waic"] == pytest.approx(np.sum(elpd), rel=1e-13)
    assert res["se_elpd_waic"] == pytest.approx(se, rel=1e-12)
    assert res["waic"] == pytest.approx(-2 * np.sum(elpd), rel=1e-13)
    assert res["n_p_waic_above_0.4"] == int(np.sum(p > 0.4)) > 0


def test_known_answers():
    la, lb = np.array([-1.5, -7.25, -0.1]), np.array([-2.0, -3.0, -0.1])
    S = 10
    const = np.tile(la, (S, 1))
    res = wc.finalize(logsumexp(const, axis=0), np.var(const, axis=0, ddof=1), S)
    np.testing.assert_allclose(res["lppd_i"], la, rtol=1e-14)
    assert res["p_waic"] == pytest.approx(0.0, abs=1e-30)
    alt = np.array([la if s % 2 == 0 else lb for s in range(S)])
    res = wc.finalize(logsumexp(alt, axis=0), np.var(alt, axis=0, ddof=1), S)
    np.testing.assert_allclose(res["lppd_i"], np.log((np.exp(la) + np.exp(lb)) / 2), rtol=1e-14)
    np.testing.assert_allclose(res["p_waic_i"], (la - lb) ** 2 / 4 * S / (S - 1), rtol=1e-14, atol=1e-30)


def test_json_record_and_points():
    pts = wc.Points.single_level([[np.array([[1.0, 0.0], [2.0, 50.0], [3.0, 120.0]]), np.array([[1.0, 100.0]])]], [[2, 5]])
    assert list(pts.count) == [3] and pts.info[0] == [(2, 1.0, 0.0, "censored-0"), (2, 2.0, 50.0, "uncensored"), (5, 1.0, 100.0, "censored-100")]
    assert list(pts.tag[0]) == [1, 0, 2]
    res = wc.finalize(np.array([0.0, -1.0, np.nan]), np.array([0.0, 0.5, 0.1]), 4)
    rec = wc.json_record(res, pts, 0)
    assert rec["pointwise"]["elpd"][2] is None and rec["elpd_waic"] is None
    assert rec["points"]["kind"] == ["censored-0", "uncensored", "censored-100"] and rec["draws"] == 4
    h = wc.Points.hierarchical([[np.array([[1.0, 0.0], [2.0, 50.0]]), np.array([[1.0, 105.0]])]])
    assert h.num_expts == 2 and list(h.tag[0]) == [0, 0, 1] and h.info[0][2][3] == "truncated"


# ---- compare_models ------------------------------------------------------------------------------------------------------------
def _w(points, elpd, kinds=None):
    e, d, y = zip(*points)
    return {"points": {"experiment": list(e), "dose": list(d), "response": list(y), "kind": kinds or ["uncensored"] * len(points)},
            "pointwise": {"elpd": list(elpd)}}


def test_compare_arithmetic():
    pts = [(1, 0.1, 10.0), (1, 1.0, 40.0), (2, 1.0, 40.0), (2, 10.0, 90.0), (1, 1.0, 40.0)]     # a replicate, aligned by occurrence
    a = np.array([-1.0, -2.0, -2.5, -3.0, -1.0])
    b = np.array([-1.5, -2.0, -3.5, -3.1, -4.0])
    perm = [2, 1, 0, 4, 3]                                                 # B lists its points in another order (replicates in theirs)
    wb = _w([pts[i] for i in perm], b[perm])
    r = cm.compare(_w(pts, a), wb)
    d = a - b
    assert r["elpd_diff"] == pytest.approx(np.sum(d)) and r["se_diff"] == pytest.approx(math.sqrt(5 * np.var(d, ddof=1)))
    assert r["n_mixed"] == 0 and r["n_points"] == 5 and "warning" not in r
    assert r["preferred"] == ("A" if np.sum(d) > 2 * r["se_diff"] else "neither")
    big = cm.compare(_w(pts, a), _w(pts, a - 10.0))
    assert big["preferred"] == "A" and big["se_diff"] == 0.0


def test_compare_refuses_and_flags():
    pts = [(1, 0.1, 0.0), (1, 1.0, 40.0), (1, 10.0, 100.0)]
    wa = _w(pts, [-1.0, -2.0, -0.5], ["censored-0", "uncensored", "censored-100"])
    wb = _w(pts + [(1, 3.0, 104.0)], [-3.0, -2.5, -4.0, -3.0], ["truncated"] * 4)
    r = cm.compare(wa, wb)
    assert "error" in r and r["n_only_b"] == 1 and "elpd_diff" not in r
    r = cm.compare(wa, wb, intersection=True)
    assert r["n_points"] == 3 and r["n_mixed"] == 2 and "warning" in r
    assert r["elpd_diff"] == pytest.approx(-3.5 + 9.5)


# ---- the C ABI without a GPU ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from pyhillfit_amd import _lib
    return _lib.load()


def test_abi_validation(lib):
    assert lib.phf_waic_workspace_bytes(3, 7, 65, 100) == 3 * 7 * 5 * 65 * 8
    for bad in ((0, 7, 65, 100), (3, 0, 65, 100), (3, 7, 0, 100), (3, 7, 65, 0)):
        assert lib.phf_waic_workspace_bytes(*bad) == 0
        assert lib.phf_last_error()
    with pytest.raises(ValueError):
        wc.workspace_bytes(1, 1, 1, 0)
    assert lib.phf_waic_init(3, 7, 65, 100, None, C.c_size_t(1 << 20), None) == -1 and b"null" in lib.phf_last_error()
    assert lib.phf_waic_init(3, 7, 65, 100, C.c_void_p(8), C.c_size_t(16), None) == -1 and b"smaller" in lib.phf_last_error()
    assert lib.phf_waic_reduce(3, 7, 65, 100, C.c_void_p(8), C.c_size_t(16), C.c_void_p(8), None) == -1
    from pyhillfit_amd._lib import PointwisePoints
    p = PointwisePoints(2, 4, 8, 8, 8, 8)
    fake, big = C.c_void_p(8), C.c_size_t(1 << 30)
    args = lambda **kw: [kw.get(k, v) for k, v in (("pts", C.byref(p)), ("lik", 2), ("ne", 0), ("rows", fake), ("n", 10), ("Q", 2),
                                                   ("stride", 4), ("C", 64), ("first", 0), ("total", 10), ("ws", fake), ("wsb", big),
                                                   ("s", None))]
    assert lib.phf_waic_accumulate(*args(lik=4)) == -1 and b"likelihood" in lib.phf_last_error()
    assert lib.phf_waic_accumulate(*args(lik=3)) == -1 and b"num_expts" in lib.phf_last_error()
    assert lib.phf_waic_accumulate(*args(lik=3, ne=2)) == -1 and b"row_stride_cols" in lib.phf_last_error()
    assert lib.phf_waic_accumulate(*args(stride=2)) == -1 and b"row_stride_cols" in lib.phf_last_error()
    assert lib.phf_waic_accumulate(*args(first=5)) == -1 and b"total_rows" in lib.phf_last_error()
    assert lib.phf_waic_accumulate(*args(Q=3)) == -1 and b"one row per problem" in lib.phf_last_error()
    assert lib.phf_waic_accumulate(*args(wsb=C.c_size_t(8))) == -1 and b"smaller" in lib.phf_last_error()
    assert lib.phf_waic_accumulate(*args(rows=None)) == -1 and b"null" in lib.phf_last_error()
    assert lib.phf_waic_accumulate(*args(pts=None)) == -1 and b"null points" in lib.phf_last_error()
    assert lib.phf_waic_accumulate(*args(n=0, first=10)) == 0                # nothing to do: no launch
    assert lib.phf_pointwise_loglik_single_level(C.byref(p), 3, 1, fake, fake, fake, None) == -1 and b"model" in lib.phf_last_error()
    assert lib.phf_pointwise_loglik_single_level(C.byref(p), 2, -1, fake, fake, fake, None) == -1
    assert lib.phf_pointwise_loglik_single_level(C.byref(p), 2, 0, None, None, None, None) == 0
    assert lib.phf_pointwise_loglik_hierarchical(C.byref(p), 0, 1, fake, fake, fake, None) == -1 and b"num_expts" in lib.phf_last_error()
    assert lib.phf_pointwise_loglik_hierarchical(None, 3, 1, fake, fake, fake, None) == -1
