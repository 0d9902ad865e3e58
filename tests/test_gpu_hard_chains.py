"""The streaming accumulators on hard chains, on the GPU: the diagnostics, batch-means, co-moment, WAIC and stepping-stone kernels,
driven through their Python classes, against the exact reference of tests/hard_chains.py.

a. accuracy: |device - exact| <= 4 x the a-priori bound of every raw output (the derivations: hard_chains' docstring; the magnitudes
   come from the exact reference), every family with finite data; the worst error / bound per kernel and family is printed.
b. exact cases: a constant column leaves every accumulator +0.0 bit for bit; W = 0 is reported as undetermined, never as a number.
c. a planted -inf, +inf or NaN stays in its (problem, column): everything else keeps its bits.
d. the whole run and the run cut at rows [1, 7, 8, N//2, N//2 + 1] are bit-identical on the hard data, NaN patterns included."""
import numpy as np
import pytest

import hard_chains as hc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SHAPES = list(hc.SHAPES) + [hc.LONG_SHAPE]
WHERE = ["first of half 0", "middle of half 0", "dropped middle", "first of half 1", "last"]
_cache = {}


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return "cuda:0"


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def case_of(chains, N, lags, which):
    """the long shape: 1 problem x 3 columns; the others: 2 problems"""
    if (chains, N, lags) == hc.LONG_SHAPE:
        return cached(("case", chains, N, "long"), lambda: hc.Case(chains, N, 1, 7, "long", lags))
    return cached(("case", chains, N, which), lambda: hc.Case(chains, N, 2, 20 + chains, which))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def feed(acc, rows, cuts, device):
    t = torch.from_numpy(np.ascontiguousarray(rows)).to(device)
    for lo, hi in hc.segments(rows.shape[0], cuts):
        acc.accumulate(t[lo:hi])
    return acc


def run_diag(rows, cols, lags, cuts, device):
    """(workspace [Q][cols][4 L + 6][C], reduced [Q][cols][L + 3], result())"""
    from pyhillfit_amd.diagnostics import DEFAULT_LAGS, ChainDiagnostics
    N, Q, _, C = rows.shape
    d = feed(ChainDiagnostics(Q, C, cols, N, DEFAULT_LAGS if lags is None else lags, device), rows, cuts, device)
    red, res = d.reduced(), d.result()
    ws = d.ws[:Q * cols * (4 * d.L + 6) * C].reshape(Q, cols, 4 * d.L + 6, C).cpu().numpy()
    return ws, red, res, d.L


def diag_fields(ws, L):
    """workspace -> (acov [Q][cols][C][2][L+1], mean [Q][cols][C][2]) of the half-chains (phf_diagnostics.hip's Layout)"""
    acov = np.stack([ws[:, :, 3 * L + 3:4 * L + 4], ws[:, :, 0:L + 1]], axis=-1)              # [Q][cols][L+1][C][2]
    return np.moveaxis(acov, 2, -1), np.stack([ws[:, :, 4 * L + 4], ws[:, :, 4 * L + 5]], axis=-1)


def run_bm(rows, cols, cuts, device):
    from pyhillfit_amd.batch_means import BatchMeans
    N, Q, _, C = rows.shape
    b = feed(BatchMeans(Q, C, cols, N, device), rows, cuts, device)
    return b.workspace(), b.reduced(), b.result()


def run_cm(rows, d, cuts, device):
    from pyhillfit_amd.correlations import PosteriorCorrelations
    N, Q, _, C = rows.shape
    p = feed(PosteriorCorrelations(Q, C, d, N, device), rows, cuts, device)
    return p.workspace(), p.reduced(), p.result()


def run_waic(rows, points, cuts, device):
    """(workspace [Q][points][5][C]: m, s, x0, A, B;  lse [Q][points];  var [Q][points])"""
    from pyhillfit_amd import waic
    N, Q, _, C = rows.shape
    w = feed(waic.PointwiseWAIC(waic.Points.given([list(range(points))] * Q), "given", Q, C, N, device), rows, cuts, device)
    lse, var = w.reduced()
    return w.ws[:Q * points * 5 * C].reshape(Q, points, 5, C).cpu().numpy(), lse, var


def show(capsys, lines):
    with capsys.disabled():
        print("\n" + "\n".join(lines))


# ---- a. accuracy, d. cut invariance ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chains,N,lags", SHAPES)
def test_diagnostics_within_bound(gpu, capsys, chains, N, lags):
    """Every half-chain's acov(0..L) and mean, and phf_diagnostics_reduce's chain averages and B/h, within 4 x the bound
    (hard_chains, 'diagnostics': the operation order of phf_diagnostics.hip's header; a shorter form is printed beside it
    for the record and is not a bound).  Whole and cut runs: the same bits in the whole workspace and every result.
    Also printed: the relative error of the reported split-R-hat against the exact one per cancellation ratio kappa = 1 + d^2."""
    case = case_of(chains, N, lags, "all")
    ex = cached(("diag", chains, N), lambda: hc.diag_exact(case.rows, case.cols, lags))
    ws, red, res, L = run_diag(case.rows, case.cols, lags, None, gpu)
    ws2, red2, res2, _ = run_diag(case.rows, case.cols, lags, hc.cuts_of(N), gpu)
    assert np.array_equal(bits(ws), bits(ws2)) and np.array_equal(bits(red), bits(red2))
    for k in res:
        assert np.array_equal(res[k], res2[k], equal_nan=k != "lag_limit_reached"), k
    acov, mean = diag_fields(ws, L)
    t, short = hc.Table(), hc.Table()
    for j, fam in enumerate(case.families):
        t.add("diagnostics", fam, "acov per half-chain", acov[:, j], ex["acov"][:, j], ex["acov_bound"][:, j])
        t.add("diagnostics", fam, "mean per half-chain", mean[:, j], ex["mean"][:, j], ex["mean_bound"][:, j])
        t.add("diagnostics", fam, "reduced", red[:, j], ex["red"][:, j], ex["red_bound"][:, j])
        short.add("diag (short form)  ", fam, "acov per half-chain", acov[:, j], ex["acov"][:, j], ex["acov_bound_short"][:, j])
    lines = t.lines() + short.lines()[1:]
    for j, kappa in enumerate(case.kappa):
        if kappa is not None:
            rel = np.max(np.abs(res["rhat"][:, j] / ex["rhat"][:, j] - 1))
            lines.append("R-hat, kappa = %.3g (%s): relative error %.2g" % (kappa, case.names[j], rel))
    show(capsys, ["diagnostics, %d chains x %d rows, L = %d" % (chains, N, L)] + lines)
    assert max(t.worst.values()) <= 1.0, lines


@pytest.mark.parametrize("chains,N,lags", SHAPES)
def test_batch_means_within_bound(gpu, capsys, chains, N, lags):
    """S1 and S2 of every level and half-chain and phf_batch_means_reduce's outputs within 4 x the bound (hard_chains, 'batch
    means'); h = 18 has levels 0..4 (row by row against memory), h = 65 levels 0..6 (the aligned groups of 32 rows in registers and
    the levels >= 5 in memory).  Whole and cut runs: the same bits."""
    case = case_of(chains, N, lags, "all")
    ex = cached(("bm", chains, N), lambda: hc.bm_exact(case.rows, case.cols))
    ws, red, res = run_bm(case.rows, case.cols, None, gpu)
    ws2, red2, res2 = run_bm(case.rows, case.cols, hc.cuts_of(N), gpu)
    assert np.array_equal(bits(ws), bits(ws2)) and np.array_equal(bits(red), bits(red2))
    nl = (N // 2).bit_length()
    x0, S1, S2 = hc.bm_fields(ws, nl)
    t = hc.Table()
    for j, fam in enumerate(case.families):
        t.add("batch means", fam, "S1", S1[:, j], ex["S1"][:, j], ex["S1_bound"][:, j])
        t.add("batch means", fam, "S2", S2[:, j], ex["S2"][:, j], ex["S2_bound"][:, j])
        t.add("batch means", fam, "reduced", red[:, j], ex["red"][:, j], ex["red_bound"][:, j])
    show(capsys, ["batch means, %d chains x %d rows" % (chains, N)] + t.lines())
    assert max(t.worst.values()) <= 1.0, t.lines()


@pytest.mark.parametrize("chains,N,lags", SHAPES)
def test_comoments_within_bound(gpu, capsys, chains, N, lags):
    """W, B/h, the grand mean and the pooled covariance over eight (three at the long shape) columns of all families at once, so
    that the cross terms pair a 1e-5-wide column with a 1e6-sd outlying start: within 4 x the bound (hard_chains, 'co-moments').
    Whole and cut runs: the same bits."""
    case = case_of(chains, N, lags, "pairs")
    d = case.cols
    ex = cached(("cm", chains, N), lambda: hc.cm_exact(case.rows, d))
    ws, out, _ = run_cm(case.rows, d, None, gpu)
    ws2, out2, _ = run_cm(case.rows, d, hc.cuts_of(N), gpu)
    assert np.array_equal(bits(ws), bits(ws2)) and np.array_equal(bits(out), bits(out2))
    t = hc.comoments_table(out, ex, d, N // 2)
    show(capsys, ["co-moments, %d chains x %d rows, %d columns" % (chains, N, d)] + t.lines())
    assert max(t.worst.values()) <= 1.0, t.lines()


@pytest.mark.parametrize("chains,N,lags", SHAPES)
def test_waic_within_bound(gpu, capsys, chains, N, lags):
    """The per-point log-sum-exp (against mpmath at 120 digits) and variance of l (against exact fractions), l handed in directly
    (phf_waic_accumulate_given): within 4 x the bound (hard_chains, 'WAIC').  Whole and cut runs: the same bits."""
    case = case_of(chains, N, lags, "pairs")
    ex = cached(("waic", chains, N), lambda: hc.waic_exact(case.rows, case.cols))
    ws, lse, var = run_waic(case.rows, case.cols, None, gpu)
    ws2, lse2, var2 = run_waic(case.rows, case.cols, hc.cuts_of(N), gpu)
    assert np.array_equal(bits(ws), bits(ws2)) and np.array_equal(bits(lse), bits(lse2)) and np.array_equal(bits(var), bits(var2))
    t = hc.Table()
    for j, fam in enumerate(case.families):
        t.add("WAIC", fam, "lse", lse[:, j], ex["lse"][:, j], ex["lse_bound"][:, j])
        t.add("WAIC", fam, "var", var[:, j], ex["var"][:, j], ex["var_bound"][:, j])
    show(capsys, ["WAIC, %d chains x %d rows" % (chains, N)] + t.lines())
    assert max(t.worst.values()) <= 1.0, t.lines()


# ---- b. exact cases ------------------------------------------------------------------------------------------------------------------
def test_constant_columns_are_exact_and_undetermined(gpu):
    """A column that never moves: every shifted value is exactly 0, so every Q, S, S1, S2, P, A and B is +0.0 bit for bit and the
    half-chain's mean is the value itself.  Constant within each chain and different between them: W exactly 0, B/h > 0 (its
    accuracy: the bound tests above).  The Python layer then reports R-hat, ESS and the correlations as NaN / null with the reason,
    and counts the column in the rank's report line."""
    from pyhillfit_amd import correlations as co
    from pyhillfit_amd import diagnostics as dg
    case = case_of(65, 37, None, "all")
    j0, j1, j2 = (case.names.index(n) for n in ("constant everywhere", "constant per chain", "offset mu=-40 sd=1"))
    rows = np.ascontiguousarray(case.rows[:, :, [j0, j1, j2, case.cols]])
    value = rows[0, :, :2]                                                           # [Q][2 columns][C]
    ws, red, res, L = run_diag(rows, 3, None, hc.cuts_of(37), gpu)
    assert L == 17 and not np.any(bits(ws[:, :2, :3 * L + 1])) and not np.any(bits(ws[:, :2, 3 * L + 2:4 * L + 4]))   # Q, head, ring, S, acov
    assert np.array_equal(ws[:, :2, 3 * L + 1], value) and np.array_equal(ws[:, :2, 4 * L + 4], value) and np.array_equal(ws[:, :2, 4 * L + 5], value)
    assert not np.any(bits(red[:, :2, :L + 1])) and np.all(red[:, 0, L + 2] < 1e-28) and np.all(red[:, 1, L + 2] > 1.0)
    for k in ("rhat", "ess", "mcse_mean"):
        assert np.all(np.isnan(res[k][:, :2])) and np.all(np.isfinite(res[k][:, 2])), k
    rec = dg.json_record(res, 0, 256, 37, 65)
    assert rec["rhat"][:2] == [None, None] and rec["ess"][:2] == [None, None] and rec["rhat"][2] is not None
    assert "never moved" in rec["reason"][0] and "never moved" in rec["reason"][1] and rec["reason"][2] is None
    line = dg.report_line(0, ["p0", "p1"], list(res["rhat"]), list(res["ess"]))
    assert "2 of 2 with R-hat > 1.01" in line and "2 with an ESS not determined" in line
    bws, bred, bres = run_bm(rows, 3, hc.cuts_of(37), gpu)
    x0, S1, S2 = hc.bm_fields(bws, 5)
    assert not np.any(bits(S1[:, :2])) and not np.any(bits(S2[:, :2])) and not np.any(bits(bws[:, :2, 2:7]))
    assert np.array_equal(x0[:, :2, :, 0], value) and np.array_equal(x0[:, :2, :, 1], value)
    assert not np.any(bits(bred[:, :2, :4])) and np.all(np.isnan(bres["ess"][:, :2])) and np.all(np.isnan(bres["mcse_mean"][:, :2]))
    cws, cout, cres = run_cm(rows, 3, hc.cuts_of(37), gpu)                          # [Q][2][x0 3 | S 3 | P 6 | rows | flag][C]
    moving = [3 + 2, 6 + hc.cm_pair(3, 2, 2)]                                        # S_2 and P_22 alone involve no constant column
    still = [f for f in range(3, 12) if f not in moving]
    assert not np.any(bits(cws[:, :, still])) and np.all(cws[:, :, 13] == 0)
    assert np.array_equal(cws[:, 0, :2], value) and np.array_equal(cws[:, 1, :2], value)
    assert not np.any(bits(cout[:, [0, 1, 2, 3, 4]])) and np.all(cout[:, 5] > 0)      # W: only W_22 is not +0.0
    assert cout[0, 12] == 4.548 and cout[1, 12] == 4.548
    for r in cres:
        assert np.all(np.isnan(r["rhat_from_moments"][:2])) and np.isfinite(r["rhat_from_moments"][2]) and np.isnan(r["rhat_multivariate"])
        assert np.all(np.isnan(r["within_correlation"][:2])) and np.all(np.isnan(r["within_correlation"][:, :2]))
        rec = co.json_record(r)
        assert rec["rhat_multivariate"] is None and "never moved" in rec["reason"] and rec["within_correlation"][0][2] is None
    assert "2 not determined" in co.report_line(0, ["p0", "p1"], cres)
    wws, lse, var = run_waic(rows, 3, hc.cuts_of(37), gpu)
    assert not np.any(bits(wws[:, :2, 3:5])) and np.array_equal(wws[:, :2, 2], value)     # A and B: +0.0; x0 the value


# ---- c. confinement of a non-finite value, d. cut invariance with it ---------------------------------------------------------------
# (shape, problem, column, chain): chain 1 sits inside the full first wavefront, chain 64 is the first lane of the ragged second one;
# the long shape has two lag blocks in diag_lag_kernel and, at h = 65, batch means' aligned groups of 32 rows and levels 5, 6 in memory
PLANTS = ([("65x37", 1, 1, c, w) for c in (1, 64) for w in WHERE]
          + [("long", 0, 1, 63, w) for w in WHERE if w != "dropped middle"])


def same_bits(a, b):
    """every array of two runs' outputs (tuples of arrays, dicts of arrays, lists of dicts): NaN at the same places and the same
    bits everywhere else (signed zeros and infinities included).  The sign and payload of a NaN are not compared: IEEE 754 leaves
    them open for arithmetic results, and hipcc forms x - x0 and pend + carry differently in the row-by-row and the 32-row paths of
    phf_bm_rows, so a NaN that enters through the rows comes out as 0x7ff8.. from one and 0xfff8.. from the other"""
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same_bits(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray) and a.dtype == np.float64:
        nan = np.isnan(a)
        return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(bits(a)[~nan], bits(b)[~nan])
    if isinstance(a, float):
        return same_bits(np.array([a]), np.array([b]))
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    return a == b


@pytest.mark.parametrize("value", hc.NONFINITE, ids=["-inf", "+inf", "nan"])
@pytest.mark.parametrize("shape,q,j,c,where", PLANTS)
def test_a_non_finite_value_stays_in_its_column(gpu, shape, q, j, c, where, value):
    """One value of (problem q, column j, chain c) replaced.  The planted rows are fed whole and in cut calls: the workspace, the
    reduced outputs and result() of the two have the same bits, NaN patterns included (at a half's first row x0 itself is the
    planted value: read from the rows in one call, stored and re-read across the cut at N//2 + 1).  Against the clean run:
    diagnostics, batch means: the planted (problem, column) is NaN in every variance-like output that reads the row, over both lag
    blocks and every batch level that reaches it (a mean may be +-inf), R-hat and ESS are NaN; every other (problem, column) and, in
    the workspace, every other chain keeps its bits.
    co-moments: phf_comoments.h drops the half-chain whole and counts it, so the planted problem's W and B/h change by design; they
    are held to the exact reference WITHOUT that half-chain, the accumulators that do not involve the planted column keep their
    bits, as does the other problem.  WAIC: every other point keeps its bits; the planted point's variance is not finite.
    The dropped middle row of the odd N is read by the three half-chain kernels not at all: nothing changes."""
    chains, N, lags = hc.LONG_SHAPE if shape == "long" else (65, 37, None)
    case = case_of(chains, N, lags, "pairs")
    d = case.cols
    row = hc.plant_rows(N)[where]
    half = 0 if row < N // 2 else 1
    cuts = hc.cuts_of(N)

    def run_all(x, cut):
        return (run_diag(x, d, lags, cut, gpu), run_bm(x, d, cut, gpu), run_cm(x, d, cut, gpu), run_waic(x, d, cut, gpu))
    clean = cached(("clean", shape), lambda: run_all(case.rows, cuts))
    rows = hc.plant(case.rows, value, row, q, j, c)
    dirty, whole = run_all(rows, cuts), run_all(rows, None)
    for name, a, b in zip(("diagnostics", "batch means", "co-moments", "WAIC"), whole, dirty):
        assert same_bits(a, b), name
    if where == "dropped middle":
        for a, b in zip(clean[:3], dirty[:3]):
            assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))
    else:
        # diagnostics
        (ws0, red0, res0, L), (ws1, red1, res1, _) = clean[0], dirty[0]
        assert L == (40 if shape == "long" else 17)
        keep = np.ones(ws0.shape, dtype=bool)
        keep[q, j, :, c] = False
        assert np.array_equal(bits(ws0)[keep], bits(ws1)[keep])
        keep = np.ones(red0.shape, dtype=bool)
        keep[q, j] = False
        assert np.array_equal(bits(red0)[keep], bits(red1)[keep])
        assert np.all(np.isnan(red1[q, j, :L + 1])) and np.isnan(red1[q, j, L + 2]) and not np.isfinite(red1[q, j, L + 1])
        for k in ("rhat", "ess", "mcse_mean"):
            assert np.isnan(res1[k][q, j]) and np.array_equal(bits(res0[k])[keep[..., 0]], bits(res1[k])[keep[..., 0]]), k
        # batch means
        (ws0, red0, res0), (ws1, red1, res1) = clean[1], dirty[1]
        keep = np.ones(ws0.shape, dtype=bool)
        keep[q, j, :, c] = False
        assert np.array_equal(bits(ws0)[keep], bits(ws1)[keep])
        nl = (N // 2).bit_length()
        hit = hc.bm_levels_hit(N, row)
        keep = np.ones(red0.shape, dtype=bool)
        keep[q, j, hit] = False
        assert np.array_equal(bits(red0)[keep], bits(red1)[keep])
        assert np.all(np.isnan(red1[q, j, hit[:-2] + hit[-1:]])) and not np.isfinite(red1[q, j, nl - 1])
        assert np.isnan(res1["ess"][q, j]) and np.isnan(res1["mcse_mean"][q, j])
        # co-moments
        (ws0, out0, _), (ws1, out1, cres) = clean[2], dirty[2]
        fields = ws0.shape[2]
        touched = hc.cm_touched(d, j)
        assert touched[0] == fields - 1
        keep = np.ones(ws0.shape, dtype=bool)
        keep[q, half, touched, c] = False
        assert np.array_equal(bits(ws0)[keep], bits(ws1)[keep])
        assert ws1[q, half, fields - 1, c] == 1.0 and ws1[:, :, fields - 1].sum() == 1.0
        others = [p for p in range(case.Q) if p != q]
        assert np.array_equal(bits(out0[others]), bits(out1[others]))
        npair = d * (d + 1) // 2
        assert out1[q, 2 * npair + 2 * d] == 2 * chains - 1 and out1[q, 2 * npair + 2 * d + 1] == 1 and np.all(np.isfinite(out1))
        assert [r["half_chains_dropped"] for r in cres] == [int(p == q) for p in range(case.Q)]
        ex = cached(("cm dropped", shape, c, half), lambda: hc.cm_exact(case.rows[:, q:q + 1], d, dropped={(0, c, half)}))
        t = hc.comoments_table(out1[q:q + 1], ex, d, N // 2)
        assert max(t.worst.values()) <= 1.0, t.lines()
    # WAIC reads every row
    (ws0, lse0, var0), (ws1, lse1, var1) = clean[3], dirty[3]
    keep = np.ones(ws0.shape, dtype=bool)
    keep[q, j, :, c] = False
    assert np.array_equal(bits(ws0)[keep], bits(ws1)[keep])
    keep = np.ones(lse0.shape, dtype=bool)
    keep[q, j] = False
    assert np.array_equal(bits(lse0)[keep], bits(lse1)[keep]) and np.array_equal(bits(var0)[keep], bits(var1)[keep])
    assert not np.isfinite(var1[q, j])


# ---- stepping stone: the kernel evaluates l itself ------------------------------------------------------------------------------
DELTAS = (1.0 / 3.0, 2.0 ** -10, 0.0)
SS_ROWS = {"first of half 0": 0, "middle of half 0": 9, "first of half 1": 19, "last": 36}


@pytest.fixture(scope="module")
def ss_case(gpu):
    """Amiodarone + hERG, model 2, three rungs of steps DELTAS; 37 rows x 65 chains of parameters spread so widely that l spans
    four orders of magnitude (at Delta = 1/3 a handful of draws carry the whole sum); a test with fewer chains takes the first of
    them.  l of every draw comes from phf_single_level_log_target, which runs the same phf_sl_log_target on the same doubles"""
    import os
    from conftest import REPO
    from pyhillfit_amd import doseresponse as dr
    dr.setup(os.path.join(REPO, "data", "crumb_dataset.json"))
    dr.define_model(2)
    ne, _, ex = dr.load_crumb_data("Amiodarone", "hERG")
    packed = dr.PackedPoints([dr.concatenate_experiments(ne, ex)])
    rng = np.random.default_rng(5)
    N, Q, C = 37, len(DELTAS), 65
    rows = np.full((N, Q, 4, C), np.nan)
    rows[:, :, 0] = 6.0 + rng.uniform(-2.5, 2.5, (N, Q, C))
    rows[:, :, 1] = rng.uniform(0.3, 3.0, (N, Q, C))
    rows[:, :, 2] = np.exp(rng.uniform(np.log(1.0), np.log(20.0), (N, Q, C)))
    l = ss_loglik(packed, rows, gpu)
    assert np.all(np.isfinite(l)) and l.min() < -1e4 and l.max() > -100
    return packed, rows, l


def ss_loglik(packed, rows, device):
    from pyhillfit_amd.sampler import log_target_batch
    N, Q, _, C = rows.shape
    theta = np.moveaxis(rows[:, :, :3], 2, -1).reshape(-1, 3)
    lik, _ = log_target_batch(packed, 2, np.zeros(len(theta), dtype=np.int32), np.ones(len(theta)), theta, device)
    return lik.reshape(N, Q, C)


def run_ss(packed, rows, cuts, device):
    """(accumulators [Q][5][C]: m, s1, s2, sum of l, n;  reduced [Q][7])"""
    from pyhillfit_amd import stepping_stone as ss
    N, Q, _, C = rows.shape
    st = feed(ss.SteppingStone(packed, 2, np.zeros(Q, dtype=np.int32), np.array(DELTAS), C, N, device), rows, cuts, device)
    return st.ws[:Q * 5 * C].view(Q, 5, C).cpu().numpy(), st.reduced()


def ss_table(acc, red, ex, problems, family=""):
    N, C = acc[0, 4, 0], acc.shape[2]
    t = hc.Table()
    for q in problems:
        name = "Delta=%.3g%s" % (DELTAS[q], family)
        ok = ~np.isnan(ex["log_r_chain"][q])
        with np.errstate(divide="ignore", invalid="ignore"):
            lr = acc[q, 0] + np.log(acc[q, 1]) - np.log(N)
        t.add("stepping stone", name, "log r per chain", lr[ok], ex["log_r_chain"][q][ok], ex["log_r_chain_bound"][q][ok])
        fin = ok & np.isfinite(ex["sum_ll"][q])
        t.add("stepping stone", name, "sum of l", acc[q, 3][fin], ex["sum_ll"][q][fin], ex["sum_ll_bound"][q][fin])
        if not np.isnan(ex["log_r"][q]):
            t.add("stepping stone", name, "log r", red[q, 0], ex["log_r"][q], ex["log_r_bound"][q])
            if C > 1:
                t.add("stepping stone", name, "between-chain var", red[q, 1] ** 2 * C, ex["var"][q], ex["var_bound"][q] + 4 * hc.U * ex["var"][q])
    return t


@pytest.mark.parametrize("chains", [1, 3, 65])
def test_stepping_stone_within_bound(gpu, ss_case, capsys, chains):
    """The per-chain log-ratios (from the accumulators m and s1), the sums of l, the pooled log r and the between-chain variance of
    r_c / r (the reduce's se squared times C; one chain has none: se NaN) within 4 x the bound (hard_chains, 'stepping stone'),
    against mpmath at 120 digits on the draws' own l.  Delta = 0: log r and se exactly 0, ESS the number of draws.  Whole and cut
    runs: the same bits."""
    packed, rows, l = ss_case
    rows, l = np.ascontiguousarray(rows[..., :chains]), l[..., :chains]
    N, Q, _, C = rows.shape
    ex = hc.ss_exact(l, DELTAS)
    acc, red = run_ss(packed, rows, None, gpu)
    assert same_bits((acc, red), run_ss(packed, rows, hc.cuts_of(N), gpu))
    t = ss_table(acc, red, ex, range(Q))
    assert np.all(red[:, 4] == N) and np.all(red[:, 6] == 0)
    assert red[2, 0] == 0.0 and red[2, 2] == 0.0 and red[2, 3] == N * C and (red[2, 1] == 0.0 if C > 1 else np.all(np.isnan(red[:, 1])))
    mean_bound = ex["sum_ll_bound"].sum(axis=1) / (N * C) + hc.gamma(hc.nred(C)) * np.abs(ex["sum_ll"]).sum(axis=1) / (N * C)
    t.add("stepping stone", "all", "mean of l", red[:, 5], [float(sum(hc.F(float(v)) for v in l[:, q].ravel()) / (N * C)) for q in range(Q)],
          mean_bound)
    show(capsys, ["stepping stone, %d chains x %d rows" % (C, N)] + t.lines())
    assert max(t.worst.values()) <= 1.0, t.lines()


@pytest.mark.parametrize("sigma", [0.0, np.inf, np.nan], ids=["sigma=0", "sigma=+inf", "sigma=nan"])
@pytest.mark.parametrize("where", list(SS_ROWS))
@pytest.mark.parametrize("chains,c", [(1, 0), (3, 1), (65, 1), (65, 64)])
def test_stepping_stone_confines_a_non_finite_draw(gpu, ss_case, chains, c, where, sigma):
    """The kernel reads parameters, not l, so the value is planted as the sigma of one draw of rung 0 (Delta = 1/3), chain c:
    sigma = 0 gives l = -inf (below the floor), sigma = NaN gives l = NaN, sigma = +inf whichever of the two the likelihood makes of
    it; the reference takes the l that phf_single_level_log_target returns for the planted rows.  The row decides the branch the
    draw takes: the first row meets the empty sums, later ones the rescale (a new maximum) or the plain add.
    l = -inf: weight 0, the draw still counts in n, the mean of l is -inf, log r stays within the bound.  l = NaN: the chain's sums
    are NaN, it is counted in nan_chains, the rung's log r is NaN.  Every other chain's accumulators and the other rungs' outputs
    keep their bits, and the planted rows fed whole and in cut calls give the same bits, NaN patterns included."""
    packed, rows, l = ss_case
    rows, l = np.ascontiguousarray(rows[..., :chains]), l[..., :chains]
    N = rows.shape[0]
    row = SS_ROWS[where]
    clean = cached(("ss clean", chains), lambda: run_ss(packed, rows, hc.cuts_of(N), gpu))
    dirty = hc.plant(rows, sigma, row, 0, 2, c)
    lp = ss_loglik(packed, dirty, gpu)
    got = lp[row, 0, c]
    assert (np.isneginf(got) if sigma == 0.0 else np.isnan(got) if np.isnan(sigma) else not np.isfinite(got)), got
    lp[row, 0, c] = np.nan
    lc = l.copy()
    lc[row, 0, c] = np.nan
    assert same_bits(lp, lc)                                          # no other draw's l changed
    lp[row, 0, c] = got
    (a0, r0), (a1, r1) = clean, run_ss(packed, dirty, hc.cuts_of(N), gpu)
    assert same_bits((a1, r1), run_ss(packed, dirty, None, gpu))
    keep = np.ones(a0.shape, dtype=bool)
    keep[0, :, c] = False
    assert np.array_equal(bits(a0)[keep], bits(a1)[keep]) and np.array_equal(bits(r0[1:]), bits(r1[1:]))
    t = ss_table(a1, r1, hc.ss_exact(lp[:, :1], DELTAS[:1]), [0])
    assert max(t.worst.values()) <= 1.0, t.lines()
    assert r1[0, 4] == N and a1[0, 4, c] == N
    if np.isneginf(got):
        assert r1[0, 6] == 0 and r1[0, 5] == -np.inf and np.isfinite(r1[0, 0]) and np.isfinite(a1[0, 1, c])
    else:
        assert r1[0, 6] == 1 and np.isnan(r1[0, 0]) and np.isnan(a1[0, 1, c]) and np.isnan(a1[0, 3, c])
