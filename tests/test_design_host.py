"""Expected information gain of a next dose without a GPU: the host build of phf_design.h (the twin of the kernel) against
scipy's normal distribution, known answers through twin accumulate -> finalize, the orderings the estimator must obey (coarse <= fine,
monotone in K, <= ln n, <= the continuous mutual information by adaptive quadrature), skipped draws, the C ABI's argument validation,
the command line's flags and the "next_dose" record."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
from scipy import integrate, special, stats

from conftest import REPO

CSRC = os.path.join(REPO, "pyhillfit_amd", "csrc")
LN10 = np.log(10.0)

SHIM = r"""
#include "phf_design.h"
/* one draw given by its prediction and sigma, added to the zeroed accumulator acc [PHF_DS_ACC_DOUBLES(K)] */
void v_draw(int K, double pred, double sigma, double* acc) {
  PHF_KFETCH_V(k_log, phf_k_log, PHF_K_LOG_N);
  const double scale = phf_rcp(sigma) * PHF_INV_SQRT2;
  double none = 0.0;
  for (int lane = 0; lane < PHF_DS_LANES; ++lane) {
    double* pt = (lane == 0) ? &acc[0] : ((lane == PHF_DS_LANES - 1) ? &acc[K + 1] : &none);
    phf_ds_lane_add(lane, K / PHF_DS_LANES, pred, scale, k_log, &acc[1 + lane * (K / PHF_DS_LANES)], pt, &acc[PHF_DS_OFF_HF(K) + lane],
                    &acc[PHF_DS_OFF_HC(K) + lane]);
  }
}
double v_pred(int model, double ln_dose, double pic50, double hill) {
  PHF_KFETCH_V(k_exp, phf_k_exp, PHF_K_EXP_N);
  double pred, scale;
  phf_ds_draw_terms(model, ln_dose, pic50, hill, 1.0, k_exp, &pred, &scale);
  return pred;
}
void v_accumulate(int model, int K, const double* rows, int64_t num_rows, int Q, int cols, int C, int64_t first_row, int every,
                  const double* ln_doses, int G, int NS, double* acc) {
  phf_ds_accumulate_host(model, K, rows, num_rows, Q, cols, C, first_row, every, ln_doses, G, NS, acc);
}
int v_acc_doubles(int K) { return PHF_DS_ACC_DOUBLES(K); }
int v_bins_ok(int K) { return phf_ds_bins_ok(K); }
int v_slots_ok(int NS) { return phf_ds_slots_ok(NS); }
int v_default_bins(void) { return PHF_DS_DEFAULT_BINS; }
double v_sigma_floor(void) { return PHF_SIGMA_FLOOR; }
"""


def build_shim(directory):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler for the host build of phf_design.h")
    src, so = directory / "shim.c", directory / "libshim.so"
    src.write_text(SHIM)
    # the flags of oracle/Makefile: the host evaluates the operation sequence the kernels do
    subprocess.check_call([cc, "-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-shared",
                           "-I", CSRC, "-o", str(so), str(src), "-lm"])
    lib = C.CDLL(str(so))
    lib.v_pred.restype = C.c_double
    lib.v_sigma_floor.restype = C.c_double
    return lib


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shim(tmp_path_factory.mktemp("design"))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def twin_draw(lib, K, pred, sigma):
    """one draw's accumulator: masses [K + 2], per-lane h_fine [64], per-lane h_coarse [64], counts"""
    acc = np.zeros(lib.v_acc_doubles(K))
    lib.v_draw(C.c_int(K), C.c_double(pred), C.c_double(sigma), _p(acc))
    return acc


def twin_pred(lib, model, dose, pic50, hill=1.0):
    return lib.v_pred(C.c_int(model), C.c_double(np.log(dose)), C.c_double(pic50), C.c_double(hill))


def make_rows(model, draws):
    """draws [n][C][model + 1] (pIC50, [Hill,] sigma) of ONE problem -> the samplers' rows [n][1][model + 2][C] (log-target column 0)"""
    d = np.asarray(draws, dtype=np.float64)
    rows = np.zeros((d.shape[0], 1, model + 2, d.shape[1]))
    rows[:, 0, :model + 1, :] = d.transpose(0, 2, 1)
    return rows


def twin_accumulate(lib, model, K, rows, doses, slots, first_row=0, every=1, acc=None):
    """rows [n][Q][cols][C], doses [Q][G] (uM) -> acc [Q][G][slots][A], the twin of phf_design_accumulate (acc: continued)"""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    ln = np.ascontiguousarray(np.log(np.asarray(doses, dtype=np.float64)))
    n, Q, cols, Cn = rows.shape
    if acc is None:
        acc = np.zeros((Q, ln.shape[1], slots, lib.v_acc_doubles(K)))
    lib.v_accumulate(C.c_int(model), C.c_int(K), _p(rows), C.c_int64(n), C.c_int(Q), C.c_int(cols), C.c_int(Cn), C.c_int64(first_row),
                     C.c_int(every), _p(ln), C.c_int(ln.shape[1]), C.c_int(slots), _p(acc))
    return acc


def twin_result(lib, model, K, rows, doses, slots=2, every=1):
    """twin accumulate -> finalize, per problem"""
    from pyhillfit_amd import design as ds
    acc = twin_accumulate(lib, model, K, rows, doses, slots, 0, every)
    return [ds.finalize(acc[q], np.asarray(doses)[q], [], K, every, rows.shape[3]) for q in range(rows.shape[1])]


def pic50_for_pred(pred, dose=1.0):
    """the pIC50 whose Hill = 1 curve predicts `pred` percent at `dose` uM"""
    return 6.0 - (np.log(dose) - np.log(pred / (100.0 - pred))) / LN10


def scipy_masses(K, pred, sigma):
    """the K + 2 masses from scipy's cdf / sf, each from the small tails on its side of pred"""
    e = np.arange(K + 1) * (100.0 / K)
    z = (e - pred) / sigma
    cdf, sf = stats.norm.cdf(z), stats.norm.sf(z)
    lo, hi = e[:-1], e[1:]
    m = np.where(hi <= pred, cdf[1:] - cdf[:-1], np.where(lo >= pred, sf[:-1] - sf[1:], 1.0 - cdf[:-1] - sf[1:]))
    return np.concatenate([[cdf[0]], m, [sf[-1]]])


# ---- 1. the masses -------------------------------------------------------------------------------------------------------------------
def test_constants(shim):
    from pyhillfit_amd import design as ds
    assert [k for k in range(1, 2100) if shim.v_bins_ok(k)] == list(ds.BIN_CHOICES) == [128, 256, 512, 1024]
    assert shim.v_default_bins() == ds.DEFAULT_BINS == 256
    assert [s for s in range(0, 70) if shim.v_slots_ok(s)] == list(range(2, 65, 2))
    assert all(shim.v_acc_doubles(k) == ds.acc_doubles(k) for k in ds.BIN_CHOICES)
    assert shim.v_sigma_floor() == 1e-3


@pytest.mark.parametrize("K", [128, 1024])
def test_masses_sum_to_one(shim, K):
    worst = [0.0, 0.0, 0.0]
    for sigma in (1.0000001e-3, 0.02, 0.39, 1.0, 5.0, 50.0):
        for pred in (0.0, 1e-9, 37.3, 50.0, 100.0 - 1e-9, 100.0):
            acc = twin_draw(shim, K, pred, sigma)
            m = acc[:K + 2]
            assert np.all(m >= 0.0), (sigma, pred)
            assert abs(np.sum(m) - 1.0) <= 1e-14, (sigma, pred, np.sum(m))
            want = scipy_masses(K, pred, sigma)
            assert np.max(np.abs(m - want)) <= 1e-15, (sigma, pred, np.max(np.abs(m - want)))
            hf, hc = acc[K + 2:K + 66].sum(), acc[K + 66:K + 130].sum()
            coarse = np.concatenate([want[:1], want[1:K + 1].reshape(-1, 2).sum(axis=1), want[K + 1:]])
            assert abs(hf - special.entr(want).sum()) <= 1e-12, (sigma, pred)
            assert abs(hc - special.entr(coarse).sum()) <= 1e-12, (sigma, pred)
            worst = [max(worst[0], abs(np.sum(m) - 1.0)), max(worst[1], np.max(np.abs(m - want))),
                     max(worst[2], abs(hf - special.entr(want).sum()))]
    print("K = %d: worst |sum - 1| %.3g, worst mass error %.3g, worst h_fine error %.3g" % (K, *worst))


# ---- 2. known answers through twin accumulate -> finalize ---------------------------------------------------------------------------
def test_identical_draws_give_zero(shim):
    draws = np.tile([5.7, 1.3, 4.0], (5, 4, 1))
    doses = [[0.01, 1.0, 3.0, 300.0]]
    for K in (128, 256):
        res = twin_result(shim, 2, K, make_rows(2, draws), doses)[0]
        assert res["draws_used"] == 20 and res["draws_skipped"] == 0
        assert np.all(np.abs(res["eig"]) <= 1e-12) and np.all(np.abs(res["eig_coarse"]) <= 1e-12), (res["eig"], res["eig_coarse"])


def test_two_point_posterior_gives_ln2(shim):
    lo, hi = pic50_for_pred(30.0), pic50_for_pred(70.0)
    assert abs(twin_pred(shim, 2, 1.0, lo) - 30.0) < 1e-12 and abs(twin_pred(shim, 2, 1.0, hi) - 70.0) < 1e-12
    draws = np.array([[[lo, 1.0, 0.5], [hi, 1.0, 0.5]]] * 3)           # 3 rows x 2 chains: the two points, equally often
    for K in (128, 1024):
        res = twin_result(shim, 2, K, make_rows(2, draws), [[1.0]])[0]
        assert abs(res["eig"][0] - np.log(2.0)) <= 1e-12 and abs(res["eig_coarse"][0] - np.log(2.0)) <= 1e-12, res["eig"]
    # model 1 reads (pIC50, sigma): the same posterior, the same answer
    res = twin_result(shim, 1, 256, make_rows(1, draws[:, :, [0, 2]]), [[1.0]])[0]
    assert abs(res["eig"][0] - np.log(2.0)) <= 1e-12


def test_hill_zero_is_flat_and_uninformative(shim):
    """Hill = 0: the prediction is 50 at every dose whatever pIC50 is, so with one sigma nothing can be learnt anywhere"""
    rng = np.random.default_rng(3)
    draws = np.stack([rng.uniform(3, 8, (6, 3)), np.zeros((6, 3)), np.full((6, 3), 2.5)], axis=2)
    res = twin_result(shim, 2, 256, make_rows(2, draws), [[1e-3, 0.1, 1.0, 50.0, 1e4]])[0]
    assert np.all(res["eig"] == res["eig"][0]) and np.all(np.abs(res["eig"]) <= 1e-12), res["eig"]
    assert np.all(res["mass_at_0"] == res["mass_at_0"][0])


# ---- 3. provable orderings -------------------------------------------------------------------------------------------------------------
def continuous_mi(pred, sigma):
    """the mutual information of the censored normal's continuous response, (value, quad's error estimate): the two point masses'
    terms exactly, the density on (0, 100) by adaptive quadrature between the sorted predictions"""
    pred, sigma = np.asarray(pred, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
    p0, p1 = stats.norm.cdf((0.0 - pred) / sigma), stats.norm.sf((100.0 - pred) / sigma)
    value = sum(special.entr(p.mean()) - special.entr(p).mean() for p in (p0, p1))

    def f(y):
        d = stats.norm.pdf(y, pred, sigma)
        return special.entr(d.mean()) - special.entr(d).mean()
    cuts = np.unique(np.clip(np.concatenate([[0.0, 100.0], pred, pred - 4 * sigma, pred + 4 * sigma]), 0.0, 100.0))
    err = 0.0
    for a, b in zip(cuts[:-1], cuts[1:]):
        v, e = integrate.quad(f, a, b, epsabs=1e-11, epsrel=1e-11, limit=200)
        value, err = value + v, err + e
    return float(value), float(err)


@pytest.mark.parametrize("name,seed,pred_range,sigma_range", [
    ("around 50", 11, (25.0, 75.0), (2.0, 8.0)), ("near the 0 bound", 12, (0.05, 12.0), (2.0, 8.0)), ("small sigma", 13, (20.0, 80.0), (0.02, 0.2))])
def test_orderings(shim, name, seed, pred_range, sigma_range):
    rng = np.random.default_rng(seed)
    n = 64
    want_pred, sigma = rng.uniform(*pred_range, n), rng.uniform(*sigma_range, n)
    pic50 = pic50_for_pred(want_pred)
    pred = np.array([twin_pred(shim, 2, 1.0, p) for p in pic50])          # what the twin itself predicts
    assert np.max(np.abs(pred - want_pred)) < 1e-10
    draws = np.stack([pic50, np.ones(n), sigma], axis=1).reshape(16, 4, 3)
    eig = {}
    for K in (128, 256, 512, 1024):
        res = twin_result(shim, 2, K, make_rows(2, draws), [[1.0]])[0]
        assert res["draws_used"] == n
        eig[K] = res["eig"][0]
        assert -1e-12 <= res["eig_coarse"][0] <= res["eig"][0] + 1e-12, (K, res["eig_coarse"][0], res["eig"][0])
        assert res["eig"][0] <= np.log(n)
        assert abs(res["gap"][0] - (res["eig"][0] - res["eig_coarse"][0])) == 0.0
        if K > 128:
            assert abs(res["eig_coarse"][0] - eig[K // 2]) <= 1e-12      # the coarse value IS the K/2 value
            assert eig[K] >= eig[K // 2] - 1e-12
    exact, err = continuous_mi(pred, sigma)
    for K in sorted(eig):
        print("%s: K = %4d eig = %.9f deficit to the continuous value %.3g (continuous %.9f +- %.2g)" % (name, K, eig[K], exact - eig[K], exact, err))
    assert eig[1024] <= exact + err, (eig[1024], exact, err)


# ---- 4. skipped draws ------------------------------------------------------------------------------------------------------------------
def test_skipped_draws(shim):
    rng = np.random.default_rng(21)
    good = np.stack([rng.uniform(4.5, 7, 9), rng.uniform(0.4, 3, 9), rng.uniform(0.5, 20, 9)], axis=1)
    bad = np.array([[5.5, 1.0, 1e-3], [np.nan, 1.0, 4.0], [5.5, np.inf, 4.0], [5.5, 1.0, np.nan], [-np.inf, 1.0, 4.0], [5.5, 1.0, -2.0]])
    mixed = np.vstack([good[:2], bad[:1], good[2:5], bad[1:3], good[5:], bad[3:]])
    doses = [[0.03, 1.0, 30.0]]
    a = twin_accumulate(shim, 2, 256, make_rows(2, mixed[:, None, :]), doses, 2)          # C = 1: a draw is a row
    b = twin_accumulate(shim, 2, 256, make_rows(2, good[:, None, :]), doses, 2)
    A = shim.v_acc_doubles(256)
    assert np.array_equal(a[..., :A - 1], b[..., :A - 1])                                 # everything but the count of the skipped
    assert np.all(a[0, :, 0, A - 1] == 6) and np.all(b[..., A - 1] == 0) and np.all(a[0, :, 0, A - 2] == 9)
    from pyhillfit_amd import design as ds
    ra, rb = ds.finalize(a[0], doses[0], [], 256, 1, 1), ds.finalize(b[0], doses[0], [], 256, 1, 1)
    assert ra["draws_used"] == 9 and ra["draws_skipped"] == 6 and rb["draws_skipped"] == 0
    assert np.array_equal(ra["eig"], rb["eig"]) and np.array_equal(ra["eig_coarse"], rb["eig_coarse"])
    # model 1 never reads a Hill column: its second column is sigma
    m1 = twin_accumulate(shim, 1, 128, make_rows(1, np.array([[[5.5, 4.0]], [[5.5, 1e-3]], [[np.nan, 4.0]]])), [[1.0]], 2)
    assert m1[0, 0, 0, -2] == 1 and m1[0, 0, 0, -1] == 2
    # nothing usable: NaN, not a number made of nothing
    none = ds.finalize(twin_accumulate(shim, 2, 128, make_rows(2, bad[:, None, :]), doses, 2)[0], doses[0], [], 128, 1, 1)
    assert none["draws_used"] == 0 and none["best"] is None and np.all(np.isnan(none["eig"]))
    assert ds.json_record(none)["best"] is None and ds.json_record(none)["candidates"][0]["eig"] is None


def test_row_cuts_and_thinning_of_the_twin(shim):
    """the same rows and the same `every` give the same bits however the calls cut them (the kernel is held to this twin)"""
    rng = np.random.default_rng(22)
    draws = np.stack([rng.uniform(4.5, 7, (7, 5)), rng.uniform(0.4, 3, (7, 5)), rng.uniform(0.5, 20, (7, 5))], axis=2)
    rows, doses = make_rows(2, draws), [[0.1, 10.0]]
    whole = twin_accumulate(shim, 2, 128, rows, doses, 4, 1, 2)
    cut = twin_accumulate(shim, 2, 128, rows[:3], doses, 4, 1, 2)
    cut = twin_accumulate(shim, 2, 128, rows[3:], doses, 4, 4, 2, acc=cut)
    assert np.array_equal(whole, cut)
    assert np.all(whole[0, :, :, -2].sum(axis=1) == 3 * 5)                 # global rows 2, 4, 6 of the rows 1..7
    only = twin_accumulate(shim, 2, 128, rows[[1, 3, 5]], doses, 4, 0, 1)
    assert np.array_equal(whole, only)


# ---- 5. the C ABI without a GPU ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from pyhillfit_amd import _lib
    return _lib.load()


def test_abi_validation(lib):
    fake = C.c_void_p(8)
    big = C.c_size_t(1 << 40)

    def acc(model=2, bins=256, x=fake, n=10, Q=3, stride=4, chains=64, first=0, every=1, doses=fake, G=4, slots=2, a=fake, ab=big):
        return lib.phf_design_accumulate(model, bins, x, n, Q, stride, chains, first, every, doses, G, slots, a, ab, None)
    for model in (0, 3, -1):
        assert acc(model=model) == -1 and b"model must be 1 or 2" in lib.phf_last_error()
    for bins in (0, 64, 100, 255, 2048):
        assert acc(bins=bins) == -1 and b"bins must be 128, 256, 512 or 1024" in lib.phf_last_error()
    assert acc(G=0) == -1 and b"num_doses" in lib.phf_last_error()
    assert acc(every=0) == -1 and b"every" in lib.phf_last_error()
    assert acc(chains=0) == -1 and b"num_chains" in lib.phf_last_error()
    assert acc(Q=0) == -1 and b"num_problems" in lib.phf_last_error()
    for slots in (0, 1, 3, 66):
        assert acc(slots=slots) == -1 and b"num_slots" in lib.phf_last_error()
    assert acc(stride=2) == -1 and b"row_stride_cols" in lib.phf_last_error()
    assert acc(model=1, stride=1) == -1 and b"row_stride_cols" in lib.phf_last_error()
    assert acc(n=-1) == -1 and b"num_rows" in lib.phf_last_error()
    assert acc(first=-1) == -1 and b"first_row" in lib.phf_last_error()
    assert acc(ab=C.c_size_t(3 * 4 * 2 * (256 + 132) * 8 - 1)) == -1 and b"smaller" in lib.phf_last_error()
    for k in ("x", "doses", "a"):
        assert acc(**{k: None}) == -1 and b"null pointer" in lib.phf_last_error()
    assert acc(n=0) == 0                                                   # nothing to do: no launch
    assert acc(first=1, n=6, every=7, x=None, doses=None, a=None) == 0     # no row of the call is used: no launch
    assert [lib.phf_design_accumulator_doubles(k) for k in (128, 256, 512, 1024, 100)] == [260, 388, 644, 1156, -1]
    used = lib.phf_design_rows_used
    from pyhillfit_amd import design as ds
    for first, n, every in ((0, 61, 1), (0, 61, 7), (1, 6, 7), (1, 7, 7), (7, 1, 7), (8, 100, 7), (0, 0, 3), (5, 1, 1)):
        want = len([r for r in range(first, first + n) if r % every == 0])
        assert used(first, n, every) == want == ds.rows_used(first, n, every)
    assert used(-1, 1, 1) == -1 and used(0, -1, 1) == -1 and used(0, 1, 0) == -1


def test_python_arguments():
    from pyhillfit_amd import design as ds
    with pytest.raises(ValueError):
        ds.check_bins(200)
    with pytest.raises(ValueError):
        ds.parse_concs("1,-2")
    assert ds.parse_concs("0.1, 10") == (0.1, 10.0)
    for bad in (lambda: ds.NextDose(3, 1, 4, [[1.0]], device="cuda"), lambda: ds.NextDose(2, 1, 4, [[1.0]], device="cpu")):
        with pytest.raises(ValueError):
            bad()
    assert ds.default_slots(30, 16, 64) == 16 and ds.default_slots(210, 16, 4096) == 2 and ds.default_slots(2, 3, 3) == 2
    assert ds.default_slots(2, 1, 65) == 64 and ds.default_slots(1, 1, 1) == 2
    assert ds.workspace_bytes(2, 3, 256, 3) == 8 * 2 * 3 * (2 * 388 + 1)
    d = ds.candidate_doses([0.1, 1.0, 10.0, 0.0], 5, (2.5,))
    assert d.shape == (6,) and d[0] == pytest.approx(0.01) and d[4] == pytest.approx(100.0) and d[5] == 2.5


# ---- 6. the flags and the record ---------------------------------------------------------------------------------------------------------
def test_parser_flags():
    from pyhillfit_amd import PyHillFit
    from pyhillfit_amd import analyses as an
    from pyhillfit_amd import design as ds
    p = PyHillFit.build_parser()
    a = p.parse_args(["--data-file", "x.csv", "-m", "2"])
    PyHillFit.check_args(p, a)
    assert a.next_dose == 0 and a.next_dose_concs is None and a.next_dose_bins is None and a.next_dose_every is None
    assert an.fit_analyses(a) == []
    a = p.parse_args(["--data-file", "x.csv", "-m", "2", "--diagnostics", "--sensitivity", "--next-dose", "8"])
    PyHillFit.check_args(p, a)
    assert (a.next_dose, a.next_dose_bins, a.next_dose_every, a.next_dose_concs) == (8, ds.DEFAULT_BINS, ds.DEFAULT_EVERY, None)
    kinds = an.fit_analyses(a)
    assert [k.__name__ for k in kinds] == ["Diagnostics", "Sensitivity", "Design"] and kinds[-1] is an.Design
    b = p.parse_args(["--data-file", "x.csv", "-m", "2", "--diagnostics", "--sensitivity"])
    PyHillFit.check_args(p, b)
    assert an.fit_analyses(b) == kinds[:-1]
    a = p.parse_args(["--data-file", "x.csv", "-m", "1", "--next-dose", "4", "--next-dose-concs", "1.0,30", "--next-dose-bins", "1024",
                      "--next-dose-every", "5"])
    PyHillFit.check_args(p, a)
    assert (a.next_dose_concs, a.next_dose_bins, a.next_dose_every) == ((1.0, 30.0), 1024, 5)


@pytest.mark.parametrize("extra,flag", [
    (["--hierarchical", "--next-dose", "4"], "--next-dose is single-level only"),
    (["--next-dose-bins", "256"], "--next-dose-bins needs --next-dose"),
    (["--next-dose-concs", "1.0"], "--next-dose-concs needs --next-dose"),
    (["--next-dose-every", "2"], "--next-dose-every needs --next-dose"),
    (["--next-dose", "4", "--next-dose-bins", "300"], "--next-dose-bins"),
    (["--next-dose", "4", "--next-dose-every", "0"], "--next-dose-every"),
    (["--next-dose", "4", "--next-dose-concs", "0"], "--next-dose-concs"),
    (["--next-dose", "-1"], "--next-dose"),
])
def test_flag_refusals(extra, flag, capsys):
    from pyhillfit_amd import PyHillFit
    with pytest.raises(SystemExit) as e:
        PyHillFit.main(["--data-file", "does-not-exist.csv", "-m", "2"] + extra)
    assert e.value.code == 2
    assert flag in capsys.readouterr().err


def test_chain_tool_refusals(capsys):
    from pyhillfit_amd import chain_design
    for argv, flag in ((["x.txt", "--data-file", "d.csv", "--bins", "100"], "--bins"), (["x.txt", "--data-file", "d.csv", "--every", "0"], "--every"),
                       (["x.txt", "--data-file", "d.csv", "--doses", "0"], "--doses"), (["x.txt", "--data-file", "d.csv", "-m", "3"], "-m"),
                       (["x.txt", "--data-file", "d.csv", "--concs", "-1"], "--concs")):
        with pytest.raises(SystemExit) as e:
            chain_design.main(argv)
        assert e.value.code == 2 and flag in capsys.readouterr().err


def test_record_and_report_line(shim):
    from pyhillfit_amd import design as ds
    rng = np.random.default_rng(31)
    draws = np.stack([rng.uniform(5.0, 6.5, (8, 3)), rng.uniform(0.6, 2, (8, 3)), rng.uniform(2, 8, (8, 3))], axis=2)
    concs = [0.1, 1.0, 10.0]
    doses = ds.candidate_doses(concs, 4, (1.0,))
    acc = twin_accumulate(shim, 2, 256, make_rows(2, draws), [doses], 2, 0, 2)
    res = ds.finalize(acc[0], doses, concs, 256, 2, 3)
    rec = ds.json_record(res)
    assert set(rec) == {"bins", "every", "draws_used", "draws_skipped", "candidates", "best", "criterion"}
    assert rec["bins"] == 256 and rec["every"] == 2 and rec["draws_used"] == 4 * 3 and rec["draws_skipped"] == 0
    assert len(rec["candidates"]) == 5
    for c, d in zip(rec["candidates"], doses):
        assert set(c) == {"dose", "eig", "eig_coarse", "gap", "eig_by_chain_parity", "predictive_mass_at_0", "predictive_mass_at_100",
                          "already_tested"}
        assert c["dose"] == d and c["gap"] == c["eig"] - c["eig_coarse"] and -1e-12 <= c["eig_coarse"] <= c["eig"] + 1e-12
        assert len(c["eig_by_chain_parity"]) == 2 and all(np.isfinite(v) for v in c["eig_by_chain_parity"])
        assert 0.0 <= c["predictive_mass_at_0"] <= 1.0 and 0.0 <= c["predictive_mass_at_100"] <= 1.0
    assert [c["already_tested"] for c in rec["candidates"]] == [False, False, False, False, True]
    assert rec["best"] == max(rec["candidates"], key=lambda c: c["eig"])
    assert "100/K %" in rec["criterion"] and "lower bound" in rec["criterion"] and "rises with K" in rec["criterion"]
    json.dumps(rec, allow_nan=False)
    # one chain: no halves to compare
    one = ds.json_record(ds.finalize(twin_accumulate(shim, 2, 128, make_rows(2, draws[:, :1]), [doses], 2)[0], doses, concs, 128, 1, 1))
    assert all(c["eig_by_chain_parity"] is None for c in one["candidates"])
    line = ds.report_line(0, ["Drug + Chan"], [res], 4)
    assert line.startswith("next-dose [rank 0]: 1 problems") and "Drug + Chan at" in line and "end of the grid" in line
    # a pair whose best dose is the first or the last grid dose is counted; a named dose beyond the grid is not an end
    ends = dict(res, best=0), dict(res, best=3), dict(res, best=4), dict(res, best=1)
    assert "; 2 problems have their best dose at an end of the grid" in ds.report_line(1, list("abcd"), list(ends), 4)
    assert ds.report_line(2, [], []) == "next-dose [rank 2]: no problems"
