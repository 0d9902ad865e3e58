"""Posterior correlations and the multivariate R-hat without a GPU: the host build of phf_comoments.h (the twin of the kernels)
against numpy's two-pass covariance in long double, every cut of a run into calls, the dropped middle row, finalize() with known
answers, degenerate inputs, the C ABI's argument validation and the command line's flag."""
import ctypes as C
import json

import numpy as np
import pytest

import comoments_twin as tw


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return tw.build_shim(tmp_path_factory.mktemp("comoments"))


def halves(rows, d):
    """rows [N][Q][stride][C] -> [Q][2][C][h][d]: the two half-chains of every chain"""
    N = rows.shape[0]
    h = N // 2
    x = np.transpose(rows[:, :, :d, :], (1, 3, 0, 2))                       # [Q][C][N][d]
    return np.stack([x[:, :, :h], x[:, :, N - h:]], axis=1)


def cov_of_state(shim, ws, d, h):
    """[Q][2][C][d][d] sample covariances (divisor h - 1) and [Q][2][C][d] means from the twin's state, in long double"""
    w = ws.astype(np.longdouble)
    Q, _, _, Cn = ws.shape
    S, x0 = w[:, :, d:2 * d], w[:, :, :d]
    cov = np.zeros((Q, 2, Cn, d, d), dtype=np.longdouble)
    for i in range(d):
        for j in range(i, d):
            P = w[:, :, 2 * d + shim.v_pair(d, i, j)]
            cov[..., i, j] = cov[..., j, i] = (P - S[:, :, i] * S[:, :, j] / h) / (h - 1)
    return cov, np.moveaxis(x0 + S / h, 2, 3)


def result_of(shim, rows, d, columns=None):
    from pyhillfit_amd import correlations as cr
    N = rows.shape[0]
    red = tw.twin_reduce(shim, tw.twin_accumulate(shim, rows, d, N), d, N)
    return [cr.finalize_reduced(r, d, columns) for r in red], red


# ---- 1. the twin against numpy ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 3, 11, 17])
@pytest.mark.parametrize("N", [8, 9, 257])
def test_twin_against_numpy(shim, d, N):
    Q, Cn, h = 2, 5, N // 2
    rows = tw.normal_rows(Q, d, Cn, N, seed=100 * d + N, stride=d + 1, fill=np.nan)       # the log-target column is never read
    ws = tw.twin_accumulate(shim, rows, d, N)
    assert ws.shape == (Q, 2, 2 * d + d * (d + 1) // 2 + 2, Cn)
    assert np.all(ws[:, :, -2] == h) and np.all(ws[:, :, -1] == 0)
    cov, mean = cov_of_state(shim, ws, d, h)
    x = halves(rows, d).astype(np.longdouble)
    want_mean = x.mean(axis=3)
    dev = x - want_mean[:, :, :, None, :]
    want = np.einsum("qkcni,qkcnj->qkcij", dev, dev) / (h - 1)
    var = np.einsum("qkcii->qkci", want)
    scale = np.sqrt(var[..., :, None] * var[..., None, :])
    err = float(np.max(np.abs(cov - want) / scale))
    merr = float(np.max(np.abs(mean - want_mean) / np.sqrt(var)))
    print("d = %d, N = %d: worst covariance error %.3g of sqrt(var_i var_j), worst mean error %.3g sd" % (d, N, err, merr))
    assert err <= 1e-10 and merr <= 1e-10
    # the reduction: W is the mean of the half-chains' covariances, B/h the covariance of their means
    from pyhillfit_amd import correlations as cr
    red = tw.twin_reduce(shim, ws, d, N)
    for q in range(Q):
        W, Bh, gm, m, dropped, hh = cr.unpack(red[q], d)
        assert (m, dropped, hh) == (2 * Cn, 0, h)
        Wn = want[q].reshape(2 * Cn, d, d).mean(axis=0)
        mk = want_mean[q].reshape(2 * Cn, d)
        Bn = np.cov(mk.astype(np.float64), rowvar=False, ddof=1).reshape(d, d)
        s = np.sqrt(np.outer(np.diag(Wn), np.diag(Wn))).astype(np.float64)
        assert np.max(np.abs(W - Wn.astype(np.float64)) / s) <= 1e-10
        assert np.max(np.abs(Bh - Bn) / s) <= 1e-10
        assert np.max(np.abs(gm - mk.mean(axis=0).astype(np.float64)) / np.sqrt(np.diag(s))) <= 1e-10


# ---- 2. cuts ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [3, 11])
def test_every_cut_gives_the_same_bits(shim, d):
    rows = tw.normal_rows(2, d, 5, 9, seed=7 + d)
    whole = tw.twin_accumulate(shim, rows, d, 9)
    for cut in range(1, 9):                                                 # N = 9: all eight positions
        assert np.array_equal(whole, tw.twin_in_calls(shim, rows, d, [cut])), cut
    assert np.array_equal(whole, tw.twin_in_calls(shim, rows, d, range(1, 9)))              # 1-row calls
    for N in (8, 257):
        rows = tw.normal_rows(2, d, 5, N, seed=11 + d + N)
        whole, h = tw.twin_accumulate(shim, rows, d, N), N // 2
        for cut in (h, h + 1, N - h, N - h + 1):                            # at and one past the half boundary (and the middle row)
            assert np.array_equal(whole, tw.twin_in_calls(shim, rows, d, [cut])), (N, cut)
        assert np.array_equal(whole, tw.twin_in_calls(shim, rows, d, [h, N - h] if N % 2 else [h]))
    rows = tw.normal_rows(1, d, 3, 33, seed=5)
    assert np.array_equal(tw.twin_accumulate(shim, rows, d, 33), tw.twin_in_calls(shim, rows, d, range(1, 33)))


# ---- 3. odd N --------------------------------------------------------------------------------------------------------------------------
def test_the_middle_row_of_an_odd_run_influences_nothing(shim):
    d, N = 3, 9
    rows = tw.normal_rows(2, d, 5, N, seed=3)
    assert [shim.v_half_of(C.c_int64(N), C.c_int64(n)) for n in range(N)] == [0, 0, 0, 0, -1, 1, 1, 1, 1]
    ws = tw.twin_accumulate(shim, rows, d, N)
    red = tw.twin_reduce(shim, ws, d, N)
    for v in (1e300, np.nan):
        other = rows.copy()
        other[N // 2] = v
        ws2 = tw.twin_accumulate(shim, other, d, N)
        assert np.array_equal(ws, ws2) and np.array_equal(red, tw.twin_reduce(shim, ws2, d, N))
        assert np.array_equal(ws, tw.twin_in_calls(shim, other, d, [4, 5]))               # the middle row as a call of its own


# ---- 4. finalize with known answers -----------------------------------------------------------------------------------------------------
def all_draws(rows, d, q=0):
    """[N * C][d]: every draw of problem q"""
    return np.transpose(rows[:, q, :d, :], (0, 2, 1)).reshape(-1, d)


def check_invariants(res, rows, d):
    """what holds for every determined result: the pooled covariance is np.cov of all draws, R-hat^m >= max R-hat_j, the direction"""
    h, m = res["rows_per_half_chain"], res["half_chains"]
    pooled = (m * (h - 1.0) * res["W"] + h * (m - 1.0) * res["B_over_h"]) / (m * h - 1.0)
    want = np.cov(all_draws(rows, d), rowvar=False, ddof=1).reshape(d, d)
    s = np.sqrt(np.outer(np.diag(want), np.diag(want)))
    assert np.max(np.abs(pooled - want) / s) <= 1e-10
    assert np.max(np.abs(res["sd"] - np.sqrt(np.diag(want))) / np.sqrt(np.diag(want))) <= 1e-10
    assert np.max(np.abs(res["mean"] - all_draws(rows, d).mean(axis=0)) / np.sqrt(np.diag(want))) <= 1e-10
    assert res["rhat_multivariate"] >= np.max(res["rhat_from_moments"]) - 1e-12
    a = res["apart_direction"]
    assert abs(np.linalg.norm(a) - 1.0) <= 1e-12 and a[np.argmax(np.abs(a))] > 0
    for M in (res["correlation"], res["within_correlation"]):
        assert np.array_equal(M, M.T) and np.all(np.diag(M) == 1.0) and np.all(np.abs(M) <= 1.0)
    ev = res["principal_axes"]["eigenvalues"]
    assert np.all(np.diff(ev) <= 0) and abs(ev.sum() - d) <= 1e-10
    assert abs(res["principal_axes"]["condition_number"] - ev[0] / ev[-1]) <= 1e-12 * ev[0] / ev[-1]


@pytest.mark.parametrize("rho", [0.0, 0.6, -0.95])
def test_bivariate_normal(shim, rho):
    Cn, N = 32, 1024                                                        # m h = 64 x 512 draws
    rng = np.random.default_rng(41)
    z = rng.standard_normal((N, 1, 2, Cn))
    rows = np.empty_like(z)
    rows[:, :, 0] = 5.5 + 0.3 * z[:, :, 0]
    rows[:, :, 1] = 1.2 + 2.0 * (rho * z[:, :, 0] + np.sqrt(1.0 - rho * rho) * z[:, :, 1])
    res = result_of(shim, rows, 2, ["pIC50", "Hill"])[0][0]
    assert (res["half_chains"], res["rows_per_half_chain"], res["half_chains_dropped"], res["reason"]) == (64, 512, 0, None)
    bound = 5.0 * (1.0 - rho * rho) / np.sqrt(64 * 512)
    print("rho = %+.2f: correlation %.5f (bound %.5f), within %.5f, R-hat^m %.5f" % (
        rho, res["correlation"][0, 1], bound, res["within_correlation"][0, 1], res["rhat_multivariate"]))
    assert abs(res["correlation"][0, 1] - rho) <= bound
    assert abs(res["within_correlation"][0, 1] - rho) <= 2 * bound
    assert res["rhat_multivariate"] < 1.01
    check_invariants(res, rows, 2)
    assert res["strongest_pair"][:2] == (0, 1) and res["strongest_pair"][2] == res["within_correlation"][0, 1]
    if rho:
        # the long axis of a correlated pair is the (1, sign rho) diagonal of the standardised columns
        assert np.allclose(np.abs(res["principal_axes"]["longest_axis"]), np.sqrt(0.5), atol=1e-9)
        assert abs(res["principal_axes"]["eigenvalues"][0] - (1.0 + abs(res["within_correlation"][0, 1]))) <= 1e-12
    # d = 1: the multivariate R-hat IS the split-R-hat
    one = result_of(shim, rows[:, :, :1], 1)[0][0]
    assert abs(one["rhat_multivariate"] - one["rhat_from_moments"][0]) <= 1e-12
    assert one["apart_direction"][0] == 1.0 and one["strongest_pair"] is None
    assert abs(one["rhat_from_moments"][0] - res["rhat_from_moments"][0]) <= 1e-12


@pytest.mark.parametrize("d", [3, 6])
def test_chains_displaced_along_a_known_direction(shim, d):
    Cn, N = 32, 1024
    rng = np.random.default_rng(43 + d)
    v = rng.standard_normal(d)
    v /= np.linalg.norm(v)
    rows = rng.standard_normal((N, 1, d, Cn))                               # independent unit-variance columns
    rows += 10.0 * np.arange(Cn)[None, None, None, :] * v[None, None, :, None]             # chain k displaced by k * 10 within-sd along v
    res = result_of(shim, rows, d)[0][0]
    cos = abs(float(np.dot(res["apart_direction"], v)))
    print("d = %d: |cos(apart_direction, v)| = %.6f, R-hat^m = %.3f, max R-hat_j = %.3f" % (
        d, cos, res["rhat_multivariate"], np.max(res["rhat_from_moments"])))
    assert cos >= 0.99
    assert res["rhat_multivariate"] > 2
    check_invariants(res, rows, d)
    # inside a chain nothing is correlated: the within correlation sees no displacement, the pooled one is all of it
    off = ~np.eye(d, dtype=bool)
    assert np.max(np.abs(res["within_correlation"][off])) < 5.0 / np.sqrt(64 * 512)
    big = np.abs(np.outer(v, v))[off] > 0.05
    assert np.all(np.abs(res["correlation"][off][big]) > 0.9)


# ---- 5. degenerate inputs ---------------------------------------------------------------------------------------------------------------
def no_nan(obj):
    if isinstance(obj, dict):
        return all(no_nan(v) for v in obj.values())
    if isinstance(obj, (list, tuple)):
        return all(no_nan(v) for v in obj)
    return not (isinstance(obj, float) and obj != obj)


def test_constant_column(shim):
    from pyhillfit_amd import correlations as cr
    rows = tw.normal_rows(1, 3, 5, 40, seed=9)
    rows[:, :, 1] = 1.0
    res = result_of(shim, rows, 3, ["pIC50", "Hill", "sigma"])[0][0]
    rec = cr.json_record(res)
    text = json.dumps(rec, allow_nan=False)
    assert "NaN" not in text and no_nan(rec)
    assert "Hill" in rec["reason"] and "singular" in rec["reason"]
    assert rec["rhat_multivariate"] is None and rec["lambda_max"] is None and rec["apart_direction"] is None
    assert rec["principal_axes"] is None and rec["strongest_pair"] is None
    for M in (rec["correlation"], rec["within_correlation"]):
        assert all(M[1][j] is None and M[j][1] is None for j in range(3))
        assert M[0][0] == 1.0 and M[2][2] == 1.0 and M[0][2] is not None and M[0][2] == M[2][0]
    assert rec["rhat_from_moments"][1] is None and rec["rhat_from_moments"][0] is not None
    assert rec["sd"][1] == 0.0 and rec["mean"][1] == 1.0


@pytest.mark.parametrize("chain,half", [(0, 0), (2, 1)])
def test_a_nan_drops_its_half_chain(shim, chain, half):
    from pyhillfit_amd import correlations as cr
    d, Cn, N = 3, 5, 41
    h = N // 2
    rows = tw.normal_rows(1, d, Cn, N, seed=13)
    bad = rows.copy()
    bad[(0 if half == 0 else N - h) + 7, 0, 1, chain] = np.nan
    ws_bad, ws = tw.twin_accumulate(shim, bad, d, N), tw.twin_accumulate(shim, rows, d, N)
    assert ws_bad[0, half, -1, chain] == 1.0 and ws_bad[0, :, -1].sum() == 1.0
    other = np.ones((2, Cn), dtype=bool)
    other[half, chain] = False
    assert all(np.array_equal(ws_bad[0, k, :, c], ws[0, k, :, c]) for k in range(2) for c in range(Cn) if other[k, c])
    red = tw.twin_reduce(shim, ws_bad, d, N)
    # whatever the dropped half-chain holds is not read: the clean run with only the flag set reduces to the same bits
    ws[0, half, -1, chain] = 1.0
    assert np.array_equal(red, tw.twin_reduce(shim, ws, d, N))
    res = cr.finalize_reduced(red[0], d)
    assert res["half_chains_dropped"] == 1 and res["half_chains"] == 2 * Cn - 1 and res["reason"] is None
    # and the rest is the run without that half-chain
    x = halves(rows, d)[0].astype(np.longdouble)[other]                    # [2 C - 1][h][d]
    means = x.mean(axis=1)
    dev = x - means[:, None, :]
    Wn = (np.einsum("kni,knj->kij", dev, dev) / (h - 1)).mean(axis=0).astype(np.float64)
    Bn = np.cov(means.astype(np.float64), rowvar=False, ddof=1)
    s = np.sqrt(np.outer(np.diag(Wn), np.diag(Wn)))
    assert np.max(np.abs(res["W"] - Wn) / s) <= 1e-10 and np.max(np.abs(res["B_over_h"] - Bn) / s) <= 1e-10
    assert np.max(np.abs(res["mean"] - x.reshape(-1, d).mean(axis=0).astype(np.float64))) <= 1e-10
    assert no_nan(cr.json_record(res))


def test_fewer_than_two_half_chains(shim):
    from pyhillfit_amd import correlations as cr
    rows = tw.normal_rows(1, 2, 1, 12, seed=15)
    rows[2, 0, 0, 0] = np.inf
    res = result_of(shim, rows, 2)[0][0]
    rec = cr.json_record(res)
    json.dumps(rec, allow_nan=False)
    assert rec["half_chains"] == 1 and rec["half_chains_dropped"] == 1 and "fewer than two" in rec["reason"]
    for key in ("mean", "sd", "rhat_from_moments"):
        assert rec[key] == [None, None]
    for key in ("correlation", "within_correlation"):
        assert rec[key] == [[None, None], [None, None]]
    for key in ("rhat_multivariate", "lambda_max", "apart_direction", "principal_axes", "strongest_pair"):
        assert rec[key] is None
    line = cr.report_line(0, ["Drug + Chan"], [res])
    assert "0 of 1 with" in line and "1 not determined" in line


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from pyhillfit_amd import _lib
    return _lib.load()


def test_short_runs_are_refused_as_the_diagnostics_refuse_them(lib):
    from pyhillfit_amd import correlations as cr
    from pyhillfit_amd import diagnostics as dg
    for mod, args in ((cr, (1, 3, 4, 7)), (dg, (1, 3, 4, 7))):
        with pytest.raises(ValueError, match="h = floor"):
            mod.workspace_bytes(*args)
    assert cr.workspace_bytes(1, 3, 4, 8) == 8 * 2 * 4 * (6 + 6 + 2)
    assert cr.workspace_bytes(3, 17, 70, 40) == 8 * 3 * 2 * 70 * cr.fields(17) and cr.fields(17) == 34 + 153 + 2


# ---- 6. the C ABI without a GPU ---------------------------------------------------------------------------------------------------------
def test_abi_validation(lib, shim):
    from pyhillfit_amd import correlations as cr
    fake = C.c_void_p(8)
    big = C.c_size_t(1 << 40)

    def acc(x=fake, n=10, Q=3, stride=4, chains=64, d=3, first=0, total=100, ws=fake, wb=big):
        return lib.phf_comoments_accumulate(x, n, Q, stride, chains, d, first, total, ws, wb, None)

    def init(Q=3, d=3, chains=64, total=100, ws=fake, wb=big):
        return lib.phf_comoments_init(Q, d, chains, total, ws, wb, None)

    def red(Q=3, d=3, chains=64, total=100, ws=fake, wb=big, out=fake):
        return lib.phf_comoments_reduce(Q, d, chains, total, ws, wb, out, None)
    need = 8 * 3 * 2 * 64 * cr.fields(3)
    assert lib.phf_comoments_workspace_bytes(3, 3, 64, 100) == need
    for call in (acc, init, red):
        for bad in (dict(d=0), dict(d=-1), dict(Q=0), dict(chains=0)):
            assert call(**bad) == -1 and b"must be positive" in lib.phf_last_error()
        assert call(d=1025) == -1 and b"at most 1024 columns" in lib.phf_last_error()
        assert call(total=7) == -1 and b"h = floor" in lib.phf_last_error()
        assert call(ws=None) == -1 and b"null" in lib.phf_last_error()
        assert call(wb=C.c_size_t(need - 1)) == -1 and b"smaller" in lib.phf_last_error()
    assert acc(x=None) == -1 and b"null pointer" in lib.phf_last_error()
    assert red(out=None) == -1 and b"null pointer" in lib.phf_last_error()
    assert acc(stride=2) == -1 and b"row_stride_cols" in lib.phf_last_error()
    for bad in (dict(first=-1), dict(n=-1), dict(first=95, n=6), dict(first=100, n=1)):                 # a first_row out of order
        assert acc(**bad) == -1 and b"first_row" in lib.phf_last_error()
    assert acc(n=0) == 0 and acc(n=0, first=100) == 0                       # nothing to do: no launch
    assert lib.phf_comoments_workspace_bytes(3, 0, 64, 100) == 0 and b"must be positive" in lib.phf_last_error()
    assert lib.phf_comoments_workspace_bytes(3, 3, 64, 7) == 0 and b"h = floor" in lib.phf_last_error()
    # the layout constants of the header are the Python module's
    for d in (1, 2, 3, 4, 5, 11, 17, 133):
        assert shim.v_fields(d) == cr.fields(d) and shim.v_out_doubles(d) == cr.out_doubles(d)
        assert [shim.v_pair(d, i, j) for i in range(d) for j in range(i, d)] == list(range(cr.pairs(d)))


def test_every_new_symbol_is_declared_and_exported(lib):
    import os
    import re
    from conftest import REPO
    from pyhillfit_amd import _lib
    with open(os.path.join(REPO, "include", "pyhillfit_amd.h")) as f:
        declared = set(re.findall(r"\b(phf_comoments_\w+)\s*\(", f.read()))
    want = {"phf_comoments_workspace_bytes", "phf_comoments_init", "phf_comoments_accumulate", "phf_comoments_reduce"}
    assert declared == want
    for name in want:
        assert hasattr(lib, name) and name in _lib.EXPORTS


# ---- 7. the command line ----------------------------------------------------------------------------------------------------------------
def test_parser_flag(capsys):
    from pyhillfit_amd import PyHillFit, PyHillTemp
    from pyhillfit_amd import analyses as an
    p = PyHillFit.build_parser()
    for model in (["-m", "1"], ["-m", "2"], ["-m", "2", "--hierarchical"]):
        a = p.parse_args(["--data-file", "x.csv"] + model)
        PyHillFit.check_args(p, a)
        assert a.correlations is False and an.Correlations not in an.fit_analyses(a)
        a = p.parse_args(["--data-file", "x.csv", "--correlations"] + model)
        PyHillFit.check_args(p, a)
        assert a.correlations is True and an.fit_analyses(a) == [an.Correlations]
    temp = ["--data-file", "x.csv", "-m", "2", "-d", "0", "-c", "0"]
    with pytest.raises(SystemExit):
        PyHillTemp.build_parser().parse_args(temp + ["--correlations"])
    assert "unrecognized arguments: --correlations" in capsys.readouterr().err
    assert not hasattr(PyHillTemp.build_parser().parse_args(temp), "correlations")
    every = ["--diagnostics", "--diagnostic-batch-means", "--waic", "--loo", "--quantiles", "--ppc", "--sensitivity", "--next-dose", "4",
             "--correlations"]
    a = p.parse_args(["--data-file", "x.csv", "-m", "2"] + every)
    PyHillFit.check_args(p, a)
    kinds = an.fit_analyses(a)
    assert kinds[-1] is an.Correlations and len(kinds) == 9
    a = p.parse_args(["--data-file", "x.csv", "-m", "2", "--hierarchical", "--predictive-cdfs", "--diagnostics", "--diagnostic-batch-means",
                      "--de-every", "10", "--waic", "--loo", "--leave-experiment-out", "--quantiles", "--ppc", "--sensitivity", "--correlations"])
    PyHillFit.check_args(p, a)
    kinds = an.fit_analyses(a)
    assert kinds[-1] is an.Correlations and kinds.count(an.Correlations) == 1 and len(kinds) == 11
    assert an.tempered_analyses(PyHillTemp.build_parser().parse_args(temp + ["--diagnostics"])) == [an.Diagnostics]


def test_record_and_report_line(shim):
    from pyhillfit_amd import correlations as cr
    names = ["alpha", "beta", "mu", "s", "pic50_1", "hill_1", "pic50_2", "hill_2", "sigma"]
    rng = np.random.default_rng(61)
    rows = rng.standard_normal((64, 1, 9, 6))
    rows[:, :, 5] = -0.9 * rows[:, :, 4] + np.sqrt(1 - 0.81) * rows[:, :, 5]            # pic50_1 and hill_1 correlated inside every chain
    rows[:, :, 6] += 3.0 * np.arange(6)                                                  # the chains sit apart along pic50_2
    res = result_of(shim, rows, 9, names)[0][0]
    rec = cr.json_record(res)
    json.dumps(rec, allow_nan=False)
    assert set(rec) == {"columns", "rows_per_half_chain", "half_chains", "half_chains_dropped", "mean", "sd", "correlation",
                        "within_correlation", "rhat_from_moments", "rhat_multivariate", "lambda_max", "apart_direction", "principal_axes",
                        "strongest_pair", "method"}
    assert rec["columns"] == names and rec["rows_per_half_chain"] == 32 and rec["half_chains"] == 12 and rec["half_chains_dropped"] == 0
    assert list(rec["apart_direction"]) == names and max(rec["apart_direction"], key=lambda k: abs(rec["apart_direction"][k])) == "pic50_2"
    assert set(rec["principal_axes"]) == {"eigenvalues", "condition_number", "longest_axis"} and len(rec["principal_axes"]["eigenvalues"]) == 9
    assert rec["strongest_pair"]["columns"] == ["pic50_1", "hill_1"] and rec["strongest_pair"]["within_correlation"] < -0.8
    assert "Brooks & Gelman" in rec["method"] and "(m+1)/m" in rec["method"]
    assert rec["rhat_multivariate"] == np.sqrt(31.0 / 32.0 + rec["lambda_max"])
    calm = result_of(shim, rng.standard_normal((2048, 1, 3, 8)), 3, ["pIC50", "Hill", "sigma"])[0][0]
    assert calm["rhat_multivariate"] < 1.01
    line = cr.report_line(3, ["calm", "apart"], [calm, res])
    assert line.startswith("correlations [rank 3]: 1 of 2 with a multivariate R-hat > 1.01, 0 not determined; worst: apart (R-hat ")
    assert "pic50_2" in line.split("worst:")[1].split(";")[0]
    assert "strongest pIC50-Hill within correlation: apart (pic50_1, hill_1: -0." in line
    assert cr.report_line(2, [], []) == "correlations [rank 2]: no problems"


def test_chain_tool_column_names():
    from pyhillfit_amd import chain_correlations as cc
    assert cc.column_names(2, False) == ["pIC50", "sigma"] and cc.column_names(3, False) == ["pIC50", "Hill", "sigma"]
    assert cc.column_names(11, True) == ["alpha", "beta", "mu", "s", "pic50_1", "hill_1", "pic50_2", "hill_2", "pic50_3", "hill_3", "sigma"]
    assert cc.column_names(5, False) == ["column_%d" % i for i in range(5)]
