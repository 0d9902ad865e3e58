"""The shared accumulator headers on hard chains, without a GPU: the host builds of phf_comoments.h and phf_batch_means.h against the
exact reference of tests/hard_chains.py and its a-priori bounds (derivations: that module's docstring), the exact cases, the
confinement of a planted non-finite value, cut invariance on the hard data, and what the Python layer reports for a column that
never moved.  Also the generators and the reference themselves: on benign columns the exact reference and the existing numpy
restatements agree to 1e-12, and a naive one-pass sum misses the same bound by orders of magnitude where the shift matters."""
import ctypes as C

import numpy as np
import pytest

import comoments_twin as twin
import hard_chains as hc
import test_batch_means_host as bmh
from test_diagnostics_host import reduced as diag_numpy_reduced

SHAPES = [(c, n) for c, n, _ in hc.SHAPES]


@pytest.fixture(scope="module")
def cm_lib(tmp_path_factory):
    return twin.build_shim(tmp_path_factory.mktemp("hard_cm"))


@pytest.fixture(scope="module")
def bm_lib(tmp_path_factory):
    return bmh.build_shim(tmp_path_factory.mktemp("hard_bm"))


_cases = {}


def case_of(C_, N, which):
    key = (C_, N, which)
    if key not in _cases:
        _cases[key] = hc.Case(C_, N, 2, 20 + C_, which)
    return _cases[key]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def bm_state(lib, rows, cols, cuts=None):
    """the batch-means twin on rows [N][Q][stride][C] -> state [Q][cols][5 NL + 2][C]"""
    return np.stack([bmh.host_state(lib, rows[:, q], cols, cuts) for q in range(rows.shape[1])])


def bm_reduced(lib, st, h):
    """phf_batch_means_reduce in the header's operations on a host state (the lane order of the device is not restated: the bound
    covers any order of the chain sum): [Q][cols][NL + 1]"""
    nl = int(h).bit_length()
    x0, S1, S2 = hc.bm_fields(st, nl)
    Q, cols, Cn = x0.shape[:3]
    out = np.zeros((Q, cols, nl + 1))
    with np.errstate(invalid="ignore"):                     # inf - inf of a planted value is what is being looked at
        for l in range(nl - 1):
            n, b = float(h >> l), float(1 << l)
            v = np.vectorize(lambda s1, s2: lib.v_variance(s1, s2, n, b))(S1[..., l], S2[..., l])
            out[..., l] = v.reshape(Q, cols, -1).sum(axis=-1) / (2.0 * Cn)
        means = (x0 + S1[..., 0] / float(h)).reshape(Q, cols, -1)
        out[..., nl - 1] = means.mean(axis=-1)
        out[..., nl] = means.var(axis=-1, ddof=1)
    return out


# ---- the generators and the reference themselves -----------------------------------------------------------------------------------
def test_generators_layout_and_families():
    case = case_of(3, 37, "all")
    N, h = 37, 18
    assert case.rows.shape == (37, 2, case.cols + 1, 3) and np.all(np.isnan(case.rows[:, :, case.cols])) and np.all(np.isfinite(case.rows[:, :, :case.cols]))
    assert set(case.families) == {"offset", "outlying start", "drift", "constant"}
    assert len([f for f in case.families if f == "offset"]) == len(hc.MUS) * 3
    assert max(k for k in case.kappa if k is not None) == 1.0 + 1e12
    for j, (name, fam) in enumerate(zip(case.names, case.families)):
        x = case.rows[:, 0, j]
        if fam == "outlying start":
            assert np.all(x[0] == x[N - h]) and np.all(np.abs(x[0] - np.median(x, axis=0)) > 2 * np.std(x[1:h], axis=0)), name
        if name == "constant everywhere":
            assert np.all(x == 4.548)
        if name == "constant per chain":
            assert np.all(x == x[0]) and len(set(x[0])) == 3
        if name == "one stuck chain":
            assert np.all(x[:, 0] == -40.0) and np.std(x[:, 1]) > 0
    assert hc.plant_rows(37) == {"first of half 0": 0, "middle of half 0": 9, "dropped middle": 18, "first of half 1": 19, "last": 36}
    assert hc.segments(37, hc.cuts_of(37)) == [(0, 1), (1, 7), (7, 8), (8, 18), (18, 19), (19, 37)]
    assert not np.array_equal(case.rows[:, 0, :case.cols], case.rows[:, 1, :case.cols])


def test_exact_reference_agrees_with_numpy_on_benign_columns(bm_lib):
    """unit-scale columns at offsets 0, 4.548 and -40: double precision is a reference there, to 1e-12 of each output's scale"""
    case = case_of(3, 37, "all")
    benign = [j for j, n in enumerate(case.names) if n in ("offset mu=0 sd=1", "offset mu=4.548 sd=1", "offset mu=-40 sd=1")]
    assert len(benign) == 3
    rows = case.rows[:, :, benign + [case.cols]]
    dg, bm, cm = hc.diag_exact(rows, 3), hc.bm_exact(rows, 3), hc.cm_exact(rows, 3)
    for q in range(2):
        for j in range(3):
            acov, bh, h, M = diag_numpy_reduced(rows[:, q, j].T)
            L = len(acov) - 1
            assert np.all(np.abs(dg["red"][q, j, :L + 1] - acov) <= 1e-12 * acov[0])
            assert abs(dg["red"][q, j, L + 2] - bh) <= 1e-12 * bh
            assert abs(dg["red"][q, j, L + 1] - rows[:, q, j][np.r_[0:18, 19:37]].mean()) <= 1e-12 * 40
            want = bmh.numpy_reduced(rows[:, q, j])
            assert np.all(np.abs(bm["red"][q, j] - want) <= 1e-12 * np.maximum(np.abs(want), want[0]))
        hv = np.concatenate([rows[:18, q, :3], rows[19:, q, :3]], axis=2)                     # [h][d][2 C]
        covs = np.array([np.cov(hv[:, :, k].T) for k in range(6)])
        W = covs.mean(axis=0)
        Bh = np.cov(hv.mean(axis=0))
        iu = np.triu_indices(3)
        assert np.all(np.abs(cm["W"][q] - W[iu]) <= 1e-12 * np.max(np.abs(W)))
        assert np.all(np.abs(cm["Bh"][q] - Bh[iu]) <= 1e-12 * np.max(np.abs(Bh)))
        assert np.all(np.abs(cm["mean"][q] - hv.mean(axis=(0, 2))) <= 1e-12 * 40)


def test_waic_reference_agrees_with_numpy_on_benign_columns():
    case = case_of(3, 37, "all")
    benign = [j for j, n in enumerate(case.names) if n in ("offset mu=0 sd=1", "offset mu=-40 sd=1")]
    rows = case.rows[:, :, benign + [case.cols]]
    w = hc.waic_exact(rows, 2)
    for q in range(2):
        for p in range(2):
            x = rows[:, q, p].ravel()
            assert abs(w["lse"][q, p] - (x.max() + np.log(np.sum(np.exp(x - x.max()))))) <= 1e-12 * 40
            assert abs(w["var"][q, p] / np.var(x, ddof=1) - 1) <= 1e-12


def test_a_naive_one_pass_sum_misses_the_bound_where_the_shift_matters():
    """sd = 1e-9 |mu|: sum x^2 - (sum x)^2 / h in doubles has no correct digit, so the bound is one only the shifted sums meet"""
    case = case_of(3, 37, "all")
    j = case.names.index("offset mu=-4.7e+10 sd=47")
    ex = hc.diag_exact(case.rows[:, :1, [j, case.cols]], 1)
    x = case.rows[:18, 0, j, 0]
    naive = (np.sum(x * x) - np.sum(x) ** 2 / 18) / 18
    assert abs(naive - ex["acov"][0, 0, 0, 0, 0]) > 1e6 * hc.SLACK * ex["acov_bound"][0, 0, 0, 0, 0]
    assert ex["acov"][0, 0, 0, 0, 0] > 0 and ex["acov_bound"][0, 0, 0, 0, 0] < 1e-12 * ex["acov"][0, 0, 0, 0, 0]


# ---- a. accuracy against the a-priori bound; d. cut invariance ---------------------------------------------------------------------
@pytest.mark.parametrize("chains,N", SHAPES)
def test_batch_means_twin_within_bound(bm_lib, chains, N, capsys):
    """|twin - exact| <= 4 bound for S1, S2 of every level and half-chain and for every reduced output, every family (the bounds:
    hard_chains, 'batch means'); the whole run and the cut run bit-identical"""
    case = case_of(chains, N, "all")
    ex = hc.bm_exact(case.rows, case.cols)
    st = bm_state(bm_lib, case.rows, case.cols)
    assert np.array_equal(bits(st), bits(bm_state(bm_lib, case.rows, case.cols, hc.cuts_of(N))))
    nl = (N // 2).bit_length()
    x0, S1, S2 = hc.bm_fields(st, nl)
    red = bm_reduced(bm_lib, st, N // 2)
    t = hc.Table()
    for j, fam in enumerate(case.families):
        t.add("batch means", fam, "S1", S1[:, j], ex["S1"][:, j], ex["S1_bound"][:, j])
        t.add("batch means", fam, "S2", S2[:, j], ex["S2"][:, j], ex["S2_bound"][:, j])
        t.add("batch means", fam, "reduced", red[:, j], ex["red"][:, j], ex["red_bound"][:, j])
    with capsys.disabled():
        print("\n" + "\n".join(t.lines()))
    assert max(t.worst.values()) <= 1.0, t.lines()


@pytest.mark.parametrize("chains,N", SHAPES)
def test_comoments_twin_within_bound(cm_lib, chains, N, capsys):
    """|twin - exact| <= 4 bound for W, B/h, the grand mean and the pooled covariance (the bounds: hard_chains, 'co-moments');
    the whole run and the cut run bit-identical"""
    case = case_of(chains, N, "pairs")
    d = case.cols
    ex = hc.cm_exact(case.rows, d)
    ws = twin.twin_accumulate(cm_lib, case.rows, d, N)
    assert np.array_equal(bits(ws), bits(twin.twin_in_calls(cm_lib, case.rows, d, hc.cuts_of(N))))
    out = twin.twin_reduce(cm_lib, ws, d, N)
    t = hc.comoments_table(out, ex, d, N // 2)
    with capsys.disabled():
        print("\n" + "\n".join(t.lines()))
    assert max(t.worst.values()) <= 1.0, t.lines()


# ---- b. exact cases ------------------------------------------------------------------------------------------------------------------
def test_constant_columns_are_exact_in_the_twins(bm_lib, cm_lib):
    case = case_of(3, 37, "all")
    j0, j1 = case.names.index("constant everywhere"), case.names.index("constant per chain")
    rows = case.rows[:, :, [j0, j1, case.cols]]
    nl = 5
    x0, S1, S2 = hc.bm_fields(bm_state(bm_lib, rows, 2), nl)
    assert not np.any(bits(S1)) and not np.any(bits(S2))                           # +0.0 bit for bit
    assert np.array_equal(x0[..., 0], rows[0, :, :2]) and np.array_equal(x0[..., 1], rows[0, :, :2])
    ws = twin.twin_accumulate(cm_lib, rows, 2, 37)
    assert not np.any(bits(ws[:, :, 2:2 + 2 + 3])) and np.array_equal(ws[:, 0, :2], rows[0, :, :2])       # S and P: +0.0
    out = twin.twin_reduce(cm_lib, ws, 2, 37)
    ex = hc.cm_exact(rows, 2)
    assert not np.any(bits(out[:, :3]))                                              # W exactly 0
    assert np.all(out[:, 3] == 0) and out[0, 5] > 0                                  # B/h: 0 for the one value, > 0 between chains
    assert np.all(np.abs(out[:, 3:6] - ex["Bh"]) <= hc.SLACK * ex["Bh_bound"])
    assert np.array_equal(out[:, 6], [4.548, 4.548])                                 # the mean is the value itself


def test_python_layer_reports_a_column_that_never_moved_as_undetermined():
    """W = 0 with B > 0 (constant within each chain): R-hat, ESS, MCSE and the correlations are NaN in the results, null with
    the reason in the JSON records, and counted in the ranks' report lines; never a finite number"""
    from pyhillfit_amd import batch_means as bm
    from pyhillfit_amd import correlations as co
    from pyhillfit_amd import diagnostics as dg
    h, M, L = 18, 6, 17
    acov = np.zeros((2, L + 1))
    acov[1] = 0.5 ** np.arange(L + 1)
    rhat, ess, mcse, limit = dg.finalize(acov, np.array([0.3, 0.01]), h, M)
    assert np.isnan(rhat[0]) and np.isnan(ess[0]) and np.isnan(mcse[0]) and not limit[0] and np.isfinite(rhat[1])
    res = {"rhat": rhat[None], "ess": ess[None], "mcse_mean": mcse[None], "lag_limit_reached": limit[None]}
    rec = dg.json_record(res, 0, 256, 37, 3)
    assert rec["rhat"][0] is None and rec["ess"][0] is None and rec["mcse_mean"][0] is None and rec["rhat"][1] is not None
    assert rec["reason"][0] is not None and "never moved" in rec["reason"][0] and rec["reason"][1] is None
    assert "reason" not in dg.json_record({k: v[:, 1:] for k, v in res.items()}, 0, 256, 37, 3)
    line = dg.report_line(0, ["a"], [rhat], [ess])
    assert "1 of 1 with R-hat > 1.01" in line and "1 with an ESS not determined" in line and "inf" in line
    red = np.zeros((2, 6))
    red[1, :4], red[:, 5] = [1.0, 0.9, 0.8, 0.7], [0.3, 0.01]
    b = bm.finalize(red, h, M)
    assert np.isnan(b["ess"][0]) and np.isnan(b["mcse_mean"][0]) and np.isnan(b["tau"][0]) and not b["plateau_reached"][0]
    W, Bh = np.array([[0.0, 0.0], [0.0, 1.0]]), np.array([[0.3, 0.0], [0.0, 0.01]])
    r = co.finalize(W, Bh, np.array([4.548, 1.0]), M, h)
    assert np.isnan(r["rhat_from_moments"][0]) and np.isnan(r["rhat_multivariate"]) and np.isnan(r["within_correlation"][0, 1])
    assert np.isnan(r["within_correlation"][0, 0]) and "never moved" in r["reason"]
    rec = co.json_record(r)
    assert rec["rhat_multivariate"] is None and rec["rhat_from_moments"][0] is None and rec["within_correlation"][0][1] is None
    assert "never moved" in rec["reason"] and "1 not determined" in co.report_line(0, ["a"], [r])


# ---- c. confinement of a non-finite value, d. cut invariance with it ---------------------------------------------------------------
WHERE = ["first of half 0", "middle of half 0", "dropped middle", "first of half 1", "last"]


def planted_case(shape):
    """(case, N, (problem, column, chain) of the planted value): 3 chains x 37 rows, or the long shape (h = 65: the aligned groups of
    32 rows with levels 0..4 in locals and levels 5, 6 in memory) with the value in chain 63"""
    if shape == "long":
        c_, n_, lags = hc.LONG_SHAPE
        key = ("long",)
        if key not in _cases:
            _cases[key] = hc.Case(c_, n_, 1, 7, "long", lags)
        return _cases[key], n_, (0, 1, 63)
    return case_of(3, 37, "pairs"), 37, (1, 1, 1)


@pytest.mark.parametrize("value", hc.NONFINITE, ids=["-inf", "+inf", "nan"])
@pytest.mark.parametrize("shape,where", [("3x37", w) for w in WHERE] + [("long", w) for w in WHERE if w != "dropped middle"])
def test_batch_means_twin_confines_a_non_finite_value(bm_lib, shape, where, value):
    """the planted (problem, column, chain): every variance the reduce forms from a level whose batches reach the row is NaN
    (S1 is +-inf or NaN, S2 - S1 S1 / n is inf - inf), the mean of the means is not finite; every other (problem, column, chain)
    keeps its bits; the dropped middle row changes nothing.  The planted rows fed whole and fed in cut calls: the same bits in the
    state and the reduced outputs, the NaN patterns included (x0 itself is the planted value at a half's first row: read from the
    rows in one call, stored and re-read across a cut)"""
    case, N, (q, j, c) = planted_case(shape)
    row = hc.plant_rows(N)[where]
    rows = hc.plant(case.rows, value, row, q, j, c)
    clean = bm_state(bm_lib, case.rows, case.cols)
    dirty = bm_state(bm_lib, rows, case.cols, hc.cuts_of(N))
    whole = bm_state(bm_lib, rows, case.cols)
    red_c, red_d = bm_reduced(bm_lib, clean, N // 2), bm_reduced(bm_lib, dirty, N // 2)
    assert np.array_equal(bits(whole), bits(dirty)) and np.array_equal(bits(bm_reduced(bm_lib, whole, N // 2)), bits(red_d))
    if where == "dropped middle":
        assert np.array_equal(bits(clean), bits(dirty))
        return
    mask = np.ones(clean.shape, dtype=bool)
    mask[q, j, :, c] = False
    assert np.array_equal(bits(clean)[mask], bits(dirty)[mask])
    hit = hc.bm_levels_hit(N, row)
    rmask = np.ones(red_c.shape, dtype=bool)
    rmask[q, j, hit] = False
    assert np.array_equal(bits(red_c)[rmask], bits(red_d)[rmask])
    assert np.all(np.isnan(red_d[q, j, hit[:-2] + hit[-1:]])) and not np.isfinite(red_d[q, j, hit[-2]]), red_d[q, j]


@pytest.mark.parametrize("value", hc.NONFINITE, ids=["-inf", "+inf", "nan"])
@pytest.mark.parametrize("where", WHERE)
def test_comoments_twin_drops_and_counts_the_half_chain(cm_lib, where, value):
    """phf_comoments.h: the half-chain with the planted value is flagged and left out whole, the others' accumulators keep their
    bits (also the planted half-chain's accumulators of pairs without the planted column), the other problem's output keeps its
    bits, and the planted problem's output is the exact reference's WITHOUT that half-chain, within the bound.  The planted rows
    fed whole and fed in cut calls: the same bits in the state and the output"""
    case = case_of(3, 37, "pairs")
    d, q, j, c = case.cols, 1, 1, 1
    row = hc.plant_rows(37)[where]
    rows = hc.plant(case.rows, value, row, q, j, c)
    clean = twin.twin_accumulate(cm_lib, case.rows, d, 37)
    dirty = twin.twin_in_calls(cm_lib, rows, d, hc.cuts_of(37))
    whole = twin.twin_accumulate(cm_lib, rows, d, 37)
    out_c, out_d = twin.twin_reduce(cm_lib, clean, d, 37), twin.twin_reduce(cm_lib, dirty, d, 37)
    assert np.array_equal(bits(whole), bits(dirty)) and np.array_equal(bits(twin.twin_reduce(cm_lib, whole, d, 37)), bits(out_d))
    if where == "dropped middle":
        assert np.array_equal(bits(clean), bits(dirty))
        return
    half = 0 if row < 18 else 1
    assert hc.cm_touched(d, j)[0] == cm_lib.v_fields(d) - 1
    mask = np.ones(clean.shape, dtype=bool)
    mask[q, half, hc.cm_touched(d, j), c] = False
    assert np.array_equal(bits(clean)[mask], bits(dirty)[mask])
    assert dirty[q, half, -1, c] == 1.0 and dirty[:, :, -1].sum() == 1.0
    assert np.array_equal(bits(out_c[0]), bits(out_d[0]))
    npair = d * (d + 1) // 2
    assert out_d[q, 2 * npair + 2 * d] == 5 and out_d[q, 2 * npair + 2 * d + 1] == 1 and np.all(np.isfinite(out_d))
    ex = hc.cm_exact(case.rows, d, dropped={(q, c, half)})
    t = hc.comoments_table(out_d, ex, d, 18)
    assert max(t.worst.values()) <= 1.0, t.lines()
