"""Power-scaling sensitivity without a GPU: the host build of phf_sensitivity.h (the components as exact parts of the targets, the
weight and mass rule, the cumulative Jensen-Shannon sums), a numpy restatement of the accumulation against the conjugate-normal known
answer, the C ABI's argument validation, the command lines' flags and the "sensitivity" record."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, REPO
from test_quantiles_host import base_width, bin_of, holds, t_of

CSRC = os.path.join(REPO, "pyhillfit_amd", "csrc")

SHIM = r"""
#include "phf_sensitivity.h"
/* single-level: theta [d][m]; out [4][m] = prior, likelihood, and phf_sl_log_target's own likelihood and prior at t = 1 */
void v_sl(int model, const double* lc, const double* y, const double* w, int n_other, int n_cens, double n_other_points, double ss_within,
          double pi_bit, int64_t m, const double* theta, double* out) {
  for (int64_t i = 0; i < m; ++i) {
    double th[3] = {theta[i], theta[m + i], model == 2 ? theta[2 * m + i] : 0.0};
    double lik, prior, ll1;
    phf_sens_sl_components(model, lc, y, w, n_other, n_cens, n_other_points, ss_within, pi_bit, th, phf_k_exp, phf_k_log, &out[i], &out[m + i]);
    phf_sl_log_target(model, lc, y, w, n_other, n_cens, n_other_points, ss_within, pi_bit, 1.0, th, phf_k_exp, phf_k_log, &lik, &prior, &ll1);
    out[2 * m + i] = lik;
    out[3 * m + i] = prior;
  }
}
/* hierarchical: theta [dim][m]; out [4][m] = prior, likelihood, population, phf_hier_log_target_by_experiment */
void v_hier(int ne, const int32_t* es, int max_pts, const double* lc, const double* y, const phf_hier_prior* pr, int64_t m,
            const double* theta, double* out) {
  int start[PHF_HIER_CAP + 1];
  for (int i = 0; i <= ne; ++i) start[i] = es[i];
  for (int64_t i = 0; i < m; ++i) {
    phf_sens_hier_components(ne, es, max_pts, lc, y, theta + i, (int)m, pr, phf_k_exp, phf_k_log, &out[i], &out[m + i], &out[2 * m + i]);
    out[3 * m + i] = phf_hier_log_target_by_experiment(ne, start, lc, y, theta + i, (int)m, pr, phf_k_exp, phf_k_log);
  }
}
double v_alpha_m1(double delta, int direction) { return phf_sens_alpha_m1(delta, direction); }
void v_weights(double alpha_m1, double c_ref, int64_t n, const double* c, double* w, int32_t* clamped, uint64_t* mass) {
  for (int64_t i = 0; i < n; ++i) {
    int cl;
    w[i] = phf_sens_weight(alpha_m1, c[i], c_ref, &cl);
    clamped[i] = cl;
    mass[i] = phf_sens_mass(w[i]);
  }
}
/* a chain's steps in row order: acc [4] = n, sum w, sum w^2, clamped; col [3] = sum w, sum w d, sum w d^2 */
void v_weight_steps(int64_t n, const double* w, const int32_t* clamped, double* acc) {
  for (int64_t i = 0; i < n; ++i) phf_sens_weight_step(w[i], clamped[i], &acc[0], &acc[1], &acc[2], &acc[3]);
}
void v_column_steps(int64_t n, const double* w, const double* x, double anchor, double inv_w0, double* col) {
  for (int64_t i = 0; i < n; ++i)
    phf_sens_column_step(w[i], x[i] - anchor, phf_sens_binned(x[i], anchor, inv_w0), &col[0], &col[1], &col[2]);
}
void v_cjs(int bins, const uint64_t* base, const uint64_t* mass, double* out) { phf_sens_cjs_sums(bins, base, mass, phf_k_log, out); }
"""


def build_shim(directory):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler for the host build of phf_sensitivity.h")
    src, so = directory / "shim.c", directory / "libshim.so"
    src.write_text(SHIM)
    # the flags of oracle/Makefile: the host evaluates the operation sequence the kernels do
    subprocess.check_call([cc, "-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-shared",
                           "-I", CSRC, "-o", str(so), str(src), "-lm"])
    lib = C.CDLL(str(so))
    lib.v_alpha_m1.restype = C.c_double
    lib.v_alpha_m1.argtypes = [C.c_double, C.c_int]
    return lib


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shim(tmp_path_factory.mktemp("sensitivity"))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- the host build, as numpy functions (shared with tests/test_gpu_sensitivity.py) ---------------------------------------------------
def host_sl_components(lib, packed, pair, model, theta):
    """theta [m][d] -> [4][m]: prior, likelihood, then phf_sl_log_target's likelihood and prior at t = 1"""
    th = np.ascontiguousarray(np.asarray(theta, dtype=np.float64).T)
    m = th.shape[1]
    out = np.empty((4, m))
    k = packed.counts[pair]
    lc, y, w = (np.ascontiguousarray(a[pair]) for a in (packed.ln_conc, packed.response, packed.weight))
    lib.v_sl(C.c_int(model), _p(lc), _p(y), _p(w), C.c_int(int(k[0])), C.c_int(int(k[1] + k[2])), C.c_double(packed.extra[pair, 0]),
             C.c_double(packed.extra[pair, 1]), C.c_double(packed.pi_bit[pair]), C.c_int64(m), _p(th), _p(out))
    return out


def host_hier_components(lib, packed, pair, prior, theta):
    """theta [m][dim] -> [4][m]: prior, likelihood, population, phf_hier_log_target_by_experiment"""
    th = np.ascontiguousarray(np.asarray(theta, dtype=np.float64).T)
    m = th.shape[1]
    out = np.empty((4, m))
    es = np.ascontiguousarray(packed.expt_start[pair], dtype=np.int32)
    lc, y = np.ascontiguousarray(packed.ln_conc[pair]), np.ascontiguousarray(packed.response[pair])
    lib.v_hier(C.c_int(packed.n_expts), _p(es), C.c_int(packed.stride), _p(lc), _p(y), C.byref(prior), C.c_int64(m), _p(th), _p(out))
    return out


def host_weights(lib, alpha_m1, c_ref, c):
    c = np.ascontiguousarray(c, dtype=np.float64).ravel()
    w, cl, mass = np.empty(c.size), np.empty(c.size, dtype=np.int32), np.empty(c.size, dtype=np.uint64)
    lib.v_weights(C.c_double(alpha_m1), C.c_double(c_ref), C.c_int64(c.size), _p(c), _p(w), _p(cl), _p(mass))
    return w, cl, mass


def numpy_weights(alpha_m1, c_ref, c):
    e = alpha_m1 * (np.asarray(c, dtype=np.float64).ravel() - c_ref)
    w = np.exp(np.clip(e, -8.0, 8.0))
    return w, ((e < -8.0) | (e > 8.0)).astype(np.int32), np.floor(w * 2.0 ** 20 + 0.5).astype(np.uint64)


def host_cjs_sums(lib, base, mass):
    base, mass = np.ascontiguousarray(base, dtype=np.uint64), np.ascontiguousarray(mass, dtype=np.uint64)
    out = np.empty(5)
    lib.v_cjs(C.c_int(base.size), _p(base), _p(mass), _p(out))
    return out


class Restatement(object):
    """numpy restatement of one problem's accumulation: x [n][columns][chains] and its two components comps [2][n][chains], all rows
    at once (the device's result does not depend on how they are cut).  weights(alpha_m1, c_ref, c) -> (w, clamped, mass): the host
    build's (bit for bit the device's) or numpy's."""

    def __init__(self, x, comps, delta, bins, weights, alpha_m1=None):
        x, comps = np.asarray(x, dtype=np.float64), np.asarray(comps, dtype=np.float64)
        n, cols, Cn = x.shape
        self.B, self.n, self.C = bins, n, Cn
        am1 = alpha_m1 or (1.0 / (1.0 + delta) - 1.0, (1.0 + delta) - 1.0)
        self.w = np.zeros((4, n, Cn))                          # 0: the draw enters nothing of that weight
        self.clamped_draw = np.zeros((4, n, Cn), dtype=np.int32)
        self.mass = np.zeros((4, n, Cn), dtype=np.uint64)
        self.c_ref = [np.nan, np.nan]
        self.non_finite = [0, 0]
        for comp in range(2):
            c = comps[comp]
            fin = np.isfinite(c)
            self.non_finite[comp] = int((~fin).sum())
            if not fin.any():
                continue
            self.c_ref[comp] = float(c.ravel()[np.flatnonzero(fin.ravel())[0]])      # the first finite draw in (row, chain) order
            for d in range(2):
                w, cl, ms = weights(am1[d], self.c_ref[comp], c[fin])
                self.w[2 * comp + d][fin], self.clamped_draw[2 * comp + d][fin], self.mass[2 * comp + d][fin] = w, cl, ms
        self.clamped = self.clamped_draw.reshape(4, -1).sum(axis=1)
        self.counts = np.zeros((cols, 5, bins), dtype=np.uint64)
        self.anchor, self.w0, self.level = np.full(cols, np.nan), np.full(cols, np.nan), np.zeros(cols, dtype=int)
        self.nonfinite_values = np.zeros(cols, dtype=int)
        for j in range(cols):
            v = x[:, j, :].ravel()
            fin = np.flatnonzero(np.isfinite(v))
            if not fin.size:
                self.nonfinite_values[j] = v.size
                continue
            a = float(v[fin[0]])
            w0 = base_width(a)
            t = t_of(v, a, w0)
            ok = np.isfinite(t)
            tmin, tmax = t_of(v[ok].min(), a, w0), t_of(v[ok].max(), a, w0)
            k = 0
            while not holds(tmin, tmax, k, bins) and k < 1100:
                k += 1
            b = bin_of(t[ok], k, bins)
            np.add.at(self.counts[j, 0], b, np.uint64(1))
            for s in range(4):
                np.add.at(self.counts[j, 1 + s], b, self.mass[s].ravel()[ok])
            self.anchor[j], self.w0[j], self.level[j] = a, w0, k
            self.nonfinite_values[j] = int((~ok).sum())

    def D(self, j, comp, cjs):
        return (cjs(self.counts[j, 0], self.counts[j, 1 + 2 * comp])[0] + cjs(self.counts[j, 0], self.counts[j, 2 + 2 * comp])[0])


def host_chain_sums(lib, r, x):
    """the host header's per-chain accumulation of a Restatement r over x [n][columns][chains]: weights [4][4][chains] and
    columns [columns][5][3][chains]"""
    n, cols, Cn = x.shape
    wsum, csum = np.zeros((4, 4, Cn)), np.zeros((cols, 5, 3, Cn))
    ones = np.ones(n)
    for c in range(Cn):
        for s in range(4):
            acc = np.zeros(4)
            lib.v_weight_steps(C.c_int64(n), _p(np.ascontiguousarray(r.w[s, :, c])), _p(np.ascontiguousarray(r.clamped_draw[s, :, c])), _p(acc))
            wsum[s, :, c] = acc
        for j in range(cols):
            if not np.isfinite(r.anchor[j]):
                continue
            xs = np.ascontiguousarray(x[:, j, c])
            for s in range(5):
                col = np.zeros(3)
                w = ones if s == 0 else np.ascontiguousarray(r.w[s - 1, :, c])
                lib.v_column_steps(C.c_int64(n), _p(w), _p(xs), C.c_double(r.anchor[j]), C.c_double(1.0 / r.w0[j]), _p(col))
                csum[j, s, :, c] = col
    return wsum, csum


def crumb_packed(oracle_pair, names):
    from pyhillfit_amd import doseresponse as dr
    return dr.PackedPoints([(oracle_pair(d, c).concs, oracle_pair(d, c).responses) for d, c in names])


SL_GRID = [(p, h, s) for p in (-4.0, -3.0, 0.0, 5.3, 9.0) for h in (-0.1, 0.0, 0.8, 10.0, 10.1) for s in (0.0005, 0.001, 0.0011, 2.0, 60.0)]


# ---- components ---------------------------------------------------------------------------------------------------------------------
def test_single_level_components_are_exact_parts_of_the_target(shim, golden_meta, oracle_pair):
    g = np.load(os.path.join(GOLDEN, "g1_log_target.npz"))
    names = [(m["drug"], m["channel"]) for m in golden_meta["g1_pairs"]]
    packed = crumb_packed(oracle_pair, names)
    seen_inf = 0
    for ip in range(len(names)):
        for model in (1, 2):
            sel = (g["pair"] == ip) & (g["model"] == model)
            th3 = np.concatenate([g["theta"][sel], np.array(SL_GRID)])
            th = th3 if model == 2 else th3[:, [0, 2]]
            out = host_sl_components(shim, packed, ip, model, th)
            prior, lik, t_lik, t_prior = out
            with np.errstate(invalid="ignore"):
                total, target = prior + lik, t_lik + t_prior
            assert np.array_equal(total, target, equal_nan=True)                     # bit for bit, -inf where the target is -inf
            assert np.array_equal(prior, t_prior) and np.array_equal(lik, t_lik)
            assert not np.isnan(target).any()
            seen_inf += int(np.isneginf(target).sum())
            # and the golden's own target on its t = 1 rows, to the project's tolerance
            one = sel & (g["t"] == 1.0)
            k = int(one.sum())
            if k:
                idx = np.flatnonzero(one[sel])
                want, got = g["target"][one], total[idx]
                fin = np.isfinite(want)
                assert np.array_equal(np.isfinite(got), fin)
                np.testing.assert_allclose(got[fin], want[fin], rtol=1e-12, atol=0)
    assert seen_inf > 50


def test_hierarchical_components_sum_to_the_target(shim, golden_meta, oracle_pair):
    from pyhillfit_amd import hierarchical as H
    g = np.load(os.path.join(GOLDEN, "g2_hier_target.npz"))
    prior = H.make_prior(g["shapes"], g["scales"], g["locs"])
    infs = 0
    for ip, m in enumerate(golden_meta["g2_pairs"]):
        p = oracle_pair(m["drug"], m["channel"], m["file"])
        packed = H.PackedHierPoints([p.experiments])
        pr, lik, pop, target = host_hier_components(shim, packed, 0, prior, g["theta_%d" % ip])
        with np.errstate(invalid="ignore"):
            total = (lik + pop) + pr
        inf = np.isneginf(target)
        infs += int(inf.sum())
        assert np.array_equal(np.isneginf(total), inf) and not np.isnan(total).any()   # -inf exactly where the target is -inf
        assert not np.any(np.isneginf(pr) & ~inf) and not np.any(np.isneginf(lik) & ~inf)
        assert np.array_equal(np.isneginf(pr), np.isneginf(lik))                        # outside the support: both components
        fin = np.isfinite(target)
        assert fin.sum() > 10
        assert np.all(np.abs(total[fin] - target[fin]) <= 1e-12 * np.maximum(1.0, np.abs(target[fin])))
        # the likelihood component is the reference's own data term (the golden's lik), where that is finite
        ok = fin & np.isfinite(g["lik_%d" % ip])
        np.testing.assert_allclose(lik[ok], g["lik_%d" % ip][ok], rtol=1e-10)
    assert infs >= 64


# ---- the mass rule ------------------------------------------------------------------------------------------------------------------
def test_mass_rule(shim):
    am1 = shim.v_alpha_m1(0.25, 1)
    assert am1 == 0.25 and shim.v_alpha_m1(0.25, 0) == 1.0 / 1.25 - 1.0 and shim.v_alpha_m1(0.01, 1) == (1.0 + 0.01) - 1.0
    c = np.array([3.0, 3.0 + 8.0 / 0.25, 3.0 + 8.0 / 0.25 + 1e-9 * 40, 3.0 + 40.0, 3.0 - 8.0 / 0.25, 3.0 - 33.0, 3.0 + 1.0, 3.0 - 1e300, 3.0 + 1e300])
    w, cl, mass = host_weights(shim, am1, 3.0, c)
    assert w[0] == 1.0 and mass[0] == 2 ** 20 and cl[0] == 0                       # an exponent of 0
    assert list(cl) == [0, 0, 1, 1, 0, 1, 0, 1, 1]                                  # clamped beyond +-8 only
    assert w[2] == w[1] == w[3] == w[8] and w[5] == w[4] == w[7]
    assert np.isclose(w[1], np.exp(8.0), rtol=1e-14) and np.isclose(w[4], np.exp(-8.0), rtol=1e-14)
    assert mass.max() == mass[1] and float(mass.max()) < 2.0 ** 31.6 and mass.min() == mass[4] and mass.min() >= 351
    assert int(mass.max()) * 2 ** 32 < 2 ** 64                                       # 2^32 draws of the largest mass fit a uint64
    assert mass[6] == int(np.floor(w[6] * 2.0 ** 20 + 0.5))
    nw, ncl, nm = numpy_weights(am1, 3.0, c)
    assert np.array_equal(ncl, cl) and np.allclose(nw, w, rtol=1e-14) and np.max(np.abs(nm.astype(np.int64) - mass.astype(np.int64))) <= 1


def test_c_ref_is_the_first_finite_draw_in_row_chain_order():
    comps = np.full((2, 3, 4), np.nan)
    comps[0, 0, 2], comps[0, 0, 3], comps[0, 1, 0] = 7.0, 8.0, 9.0                  # row 0 chain 2 comes before row 1 chain 0
    comps[1, 1, 3], comps[1, 2, 0] = -np.inf, 5.0                                    # -inf is not finite
    x = np.zeros((3, 1, 4))
    r = Restatement(x, comps, 0.01, 64, numpy_weights)
    assert r.c_ref == [7.0, 5.0] and r.non_finite == [9, 11]
    assert r.mass[0, 0, 2] == 2 ** 20 and r.mass[2, 2, 0] == 2 ** 20 and r.mass[2, 1, 3] == 0
    assert r.counts[0, 0].sum() == 12 and r.counts[0, 1].sum() == r.mass[0].sum() and r.counts[0, 3].sum() == 2 ** 20


# ---- CJS ----------------------------------------------------------------------------------------------------------------------------
def _cjs_of_sums(s):
    from pyhillfit_amd.sensitivity import cjs_from_sums
    return float(cjs_from_sums(s[0], s[1], s[2], s[3]))


def test_cjs_properties(shim):
    from pyhillfit_amd.sensitivity import cjs_numpy
    rng = np.random.default_rng(3)
    B = 256
    base = np.zeros(B, dtype=np.uint64)
    base[40:200] = rng.integers(0, 50, 160).astype(np.uint64)
    base[40], base[199] = 3, 2
    # identical weights: exactly 0, in the host build and in numpy
    same = host_cjs_sums(shim, base, base * np.uint64(2 ** 20))
    assert same[0] == 0.0 and same[2] == 0.0 and _cjs_of_sums(same) == 0.0 and same[4] == float(base.sum()) * 2 ** 20
    assert cjs_numpy(base, base * np.uint64(7))[0] == 0.0
    # symmetric under swapping P and Q
    other = (base * rng.integers(1, 2 ** 20, B).astype(np.uint64))
    other1 = np.where(base > 0, np.maximum(other, 1), 0).astype(np.uint64)           # the same support, so the same bin range
    a, b = host_cjs_sums(shim, base, other1), host_cjs_sums(shim, other1, base)
    assert np.array_equal(a[:4], b[:4])
    assert cjs_numpy(base, other1)[0] == pytest.approx(cjs_numpy(other1, base)[0], rel=1e-13)
    # the host build against numpy
    assert _cjs_of_sums(a) == pytest.approx(cjs_numpy(base, other1)[0], rel=1e-12)
    # a right-tail shift: the survival branch wins
    x = np.arange(B, dtype=np.float64)
    tail = np.floor(base.astype(np.float64) * np.where(x >= 190, 3.0, 1.0) * 2 ** 10).astype(np.uint64)   # the last ten bins weigh three times
    cjs, hc, hs = cjs_numpy(base, tail)
    assert hs > hc > 0 and cjs == np.sqrt(hs)
    left = np.floor(base.astype(np.float64) * np.where(x < 50, 3.0, 1.0) * 2 ** 10).astype(np.uint64)      # ... and the mirror image: the CDF branch
    assert cjs_numpy(base, left)[1] > cjs_numpy(base, left)[2] > 0
    st = host_cjs_sums(shim, base, tail)
    assert st[2] / st[3] > st[0] / st[1] and _cjs_of_sums(st) == pytest.approx(cjs, rel=1e-12)
    # nothing binned, or no mass: all 0
    assert not host_cjs_sums(shim, np.zeros(B, dtype=np.uint64), np.zeros(B, dtype=np.uint64)).any()


# ---- known answer: conjugate normal -------------------------------------------------------------------------------------------------
def conjugate_normal():
    """prior N(0, 2^2), n = 5 observations of variance 1 with mean 1.5: 4 000 rows x 64 chains of exact posterior draws, and the two
    components as columns 1 and 2 of rows [4000][3][64]"""
    rng = np.random.default_rng(1)
    prec = 0.25 + 5.0
    mean = 7.5 / prec
    theta = mean + rng.standard_normal((4000, 64)) / np.sqrt(prec)
    return np.stack([theta, -theta ** 2 / 8.0, -2.5 * (theta - 1.5) ** 2], axis=1)


def analytic(comp, alpha):
    prec = alpha / 4.0 + 5.0 if comp == 0 else 0.25 + 5.0 * alpha
    mean = 7.5 / prec if comp == 0 else 7.5 * alpha / prec
    return mean, 1.0 / np.sqrt(prec)


def analytic_D(comp, delta, lo, hi, points=200001):
    """D from the exact normal CDFs of the power-scaled posteriors, by the same h on a fine uniform grid over [lo, hi]"""
    from scipy.stats import norm
    from pyhillfit_amd.sensitivity import _h
    x = np.linspace(lo, hi, points)
    P = norm.cdf(x, *analytic(comp, 1.0))
    tot = 0.0
    for alpha in (1.0 / (1.0 + delta), 1.0 + delta):
        Q = norm.cdf(x, *analytic(comp, alpha))
        tot += np.sqrt(max(_h(P, Q), _h(1.0 - P, 1.0 - Q), 0.0))
    return tot / (2.0 * np.log2(1.0 + delta))


@pytest.fixture(scope="module")
def conjugate():
    return conjugate_normal()


@pytest.mark.parametrize("bins", [1024, 4096, 16384])
def test_known_answer_conjugate_normal(conjugate, bins):
    from pyhillfit_amd import sensitivity as sn
    rows, delta = conjugate, 0.01
    r = Restatement(rows[:, :1], rows[:, 1:].transpose(1, 0, 2), delta, bins, numpy_weights)
    theta = rows[:, 0]
    D = [r.D(0, comp, sn.cjs_numpy) / (2.0 * np.log2(1.0 + delta)) for comp in range(2)]
    want = [analytic_D(comp, delta, theta.min(), theta.max()) for comp in range(2)]
    print("bins %d: D = %r, analytic %r, deviations %r" % (bins, D, want, [abs(a / b - 1.0) for a, b in zip(D, want)]))
    for comp in range(2):
        assert abs(D[comp] / want[comp] - 1.0) < 0.05, (comp, D[comp], want[comp])
    assert D[0] == pytest.approx(0.0235, abs=0.002) and D[1] == pytest.approx(0.085, abs=0.006)
    assert sn.diagnose(D[0], D[1]) == "likelihood-dominated" and D[0] < sn.DEFAULT_THRESHOLD < D[1]
    assert r.clamped.sum() == 0 and r.non_finite == [0, 0]
    # each weighted mean within 5 between-chain standard errors of the analytic mean
    worst = 0.0
    for comp in range(2):
        for d, alpha in enumerate((1.0 / (1.0 + delta), 1.0 + delta)):
            w = r.w[2 * comp + d]
            per_chain = (w * theta).sum(axis=0) / w.sum(axis=0)
            se = per_chain.std(ddof=1) / np.sqrt(per_chain.size)
            z = abs((w * theta).sum() / w.sum() - analytic(comp, alpha)[0]) / se
            worst = max(worst, z)
            assert z < 5.0, (comp, d, z)
    print("largest |weighted mean - analytic| / between-chain se: %.2f" % worst)


# ---- the C ABI's refusals, without a GPU --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from pyhillfit_amd import _lib
    return _lib.load()


def test_abi_refusals_without_gpu(lib):
    from pyhillfit_amd import _lib
    from pyhillfit_amd import hierarchical as H
    err = lambda: lib.phf_last_error()                                              # noqa: E731
    sz = lib.phf_sensitivity_workspace_bytes
    assert sz(2, 3, 64, 1000, 4096) > 2 * 3 * 5 * 4096 * 8
    assert sz(2, 3, 64, 1000, 4096) == sz(2, 3, 64, 1000, 4096)
    assert sz(0, 3, 64, 1000, 4096) == 0 and sz(2, 0, 64, 1000, 4096) == 0 and sz(2, 3, 0, 1000, 4096) == 0 and sz(2, 3, 64, 0, 4096) == 0
    for bad in (100, 32, 8192, 0, -64):                                              # not a power of two, or outside [64, 4096]
        assert sz(2, 3, 64, 1000, bad) == 0 and b"bins" in err(), bad
    assert sz(1, 1, 64, 2 ** 26 + 1, 64) == 0 and b"2^32" in err()                 # more draws than the uint64 masses allow
    # the scratch region is bounded: a longer run does not grow the workspace once the region is full
    assert sz(210, 3, 64, 4000, 4096) == sz(210, 3, 64, 400000, 4096)
    n = sz(2, 3, 64, 1000, 4096)
    assert lib.phf_sensitivity_init(2, 3, 64, 1000, 4096, None, n, None) == -1 and b"null" in err()
    assert lib.phf_sensitivity_init(2, 3, 64, 1000, 4096, 1, n - 1, None) == -1 and b"smaller" in err()
    pts = _lib.Points(2, 16, 1, 1, 1, 1, 1, 1)
    hp = H.HierPoints(2, 16, 3, 0, 1, 1, 1)
    pr = H.make_prior()
    acc = lib.phf_sensitivity_accumulate

    def call(kind=2, sl=C.addressof(pts), hier=None, prior=None, pc=0, lc=0, rows=1, nr=10, Q=2, stride=4, chains=64, cols=3, delta=0.01,
             bins=4096, first=0, total=1000, ws=1, nbytes=n):
        return acc(kind, sl, hier, prior, pc, lc, rows, nr, Q, stride, chains, cols, delta, bins, first, total, ws, nbytes, None)

    assert call(kind=0) == -1 and b"kind" in err() and call(kind=5) == -1
    for bad in (0.0, -0.01, 0.2500001, float("nan")):
        assert call(delta=bad) == -1 and b"delta" in err(), bad
    assert call(bins=1000) == -1 and b"bins" in err()
    assert call(sl=None) == -1 and b"null" in err()
    assert call(kind=3, hier=None, prior=None) == -1 and b"null" in err()
    assert call(kind=3, hier=C.addressof(hp), prior=None) == -1 and b"null" in err()
    assert call(kind=3, hier=C.addressof(hp), prior=C.addressof(pr), stride=10, cols=10) == -1 and b"row_stride_cols" in err()   # 5 + 2 Ne = 11
    assert call(stride=2, cols=2) == -1 and b"row_stride_cols" in err()              # model 2 reads three columns
    assert call(cols=5) == -1 and b"row_stride_cols" in err()
    assert call(kind=4, sl=None, pc=4, lc=0) == -1 and b"given" in err() and call(kind=4, sl=None, pc=0, lc=-1) == -1
    assert call(nr=10, first=995) == -1 and b"total_rows" in err()                  # rows beyond total_rows
    assert call(first=-1) == -1 and call(nr=-1) == -1
    assert call(rows=None) == -1 and b"null rows" in err()
    assert call(ws=None) == -1 and b"null workspace" in err()
    assert call(nbytes=n - 8) == -1 and b"smaller" in err()                          # a short workspace
    assert call(Q=3) == -1                                                           # the points have two pairs
    assert call(nr=0) == 0                                                           # nothing to do: no launch
    red = lib.phf_sensitivity_reduce
    assert red(2, 3, 64, 1000, 4096, None, n, 1, 1, 1, None, None) == -1 and b"null" in err()
    assert red(2, 3, 64, 1000, 4096, 1, n - 1, 1, 1, 1, None, None) == -1 and b"smaller" in err()
    assert red(2, 3, 64, 1000, 4096, 1, n, None, 1, 1, None, None) == -1 and b"null out" in err()
    comp = lib.phf_sensitivity_components
    assert comp(4, None, None, None, 1, 1, 1, 1, None) == -1 and b"kind" in err()
    assert comp(2, None, None, None, 1, 1, 1, 1, None) == -1 and b"null" in err()
    assert comp(2, C.addressof(pts), None, None, 1, None, 1, 1, None) == -1 and comp(2, C.addressof(pts), None, None, -1, 1, 1, 1, None) == -1
    assert comp(3, None, C.addressof(hp), C.addressof(pr), 2 ** 30, 1, 1, 1, None) == -1 and b"2^31" in err()
    assert comp(2, C.addressof(pts), None, None, 0, None, None, None, None) == 0


# ---- flags and the record -----------------------------------------------------------------------------------------------------------
def test_flags():
    from pyhillfit_amd import PyHillFit, chain_sensitivity
    from pyhillfit_amd import sensitivity as sn
    p = PyHillFit.build_parser()
    base = ["--data-file", "x.csv", "-m", "2"]
    a = p.parse_args(base)
    PyHillFit.check_args(p, a)
    assert a.sensitivity is False and a.sensitivity_delta is None
    a = p.parse_args(base + ["--sensitivity"])
    PyHillFit.check_args(p, a)
    assert (a.sensitivity_delta, a.sensitivity_bins, a.sensitivity_threshold) == (0.01, 4096, 0.05) == (sn.DEFAULT_DELTA, sn.DEFAULT_BINS, sn.DEFAULT_THRESHOLD)
    a = p.parse_args(base + ["--hierarchical", "--sensitivity", "--sensitivity-delta", "0.25", "--sensitivity-bins", "1024", "--sensitivity-threshold", "0.1"])
    PyHillFit.check_args(p, a)
    assert (a.sensitivity_delta, a.sensitivity_bins, a.sensitivity_threshold) == (0.25, 1024, 0.1)
    for bad in (["--sensitivity", "--sensitivity-delta", "0.3"], ["--sensitivity", "--sensitivity-delta", "0"], ["--sensitivity", "--sensitivity-bins", "1000"],
                ["--sensitivity", "--sensitivity-bins", "8192"], ["--sensitivity", "--sensitivity-threshold", "0"], ["--sensitivity-delta", "0.1"],
                ["--sensitivity-bins", "1024"], ["--sensitivity-threshold", "0.1"]):
        with pytest.raises(SystemExit):
            PyHillFit.check_args(p, p.parse_args(base + bad))
    cp = chain_sensitivity.build_parser()
    a = cp.parse_args(["f.txt", "--given", "3,4"])
    chain_sensitivity.check_args(cp, a)
    assert a.given == (3, 4) and a.delta == 0.01
    for bad in (["f.txt"], ["f.txt", "--given", "3"], ["f.txt", "--given", "2,2"], ["f.txt", "--data-file", "d", "--delta", "0.5"]):
        with pytest.raises(SystemExit):
            chain_sensitivity.check_args(cp, cp.parse_args(bad))


def test_record_shape_and_report():
    import json
    from pyhillfit_amd import sensitivity as sn
    Qn, nc = 2, 3
    slots = np.zeros((Qn, nc, 28))
    slots[..., 2] = 1000.0
    slots[..., 6] = 5.0                                                              # anchor
    per = np.zeros((Qn, nc, 2, 2, 5))
    per[..., 1], per[..., 3], per[..., 4] = 10.0, 10.0, 1000.0 * 2 ** 20
    per[0, 1, 0, :, 0] = 10.0 * (0.002 * np.log2(1.01)) ** 2                         # D = 0.002
    per[0, 2, 0, :, 2] = 10.0 * (0.06 * np.log2(1.01)) ** 2                          # prior only, through the survival branch
    per[1, 0, :, :, 0] = 10.0 * (0.08 * np.log2(1.01)) ** 2                          # both
    per[1, 1, 1, :, 0] = 10.0 * (0.09 * np.log2(1.01)) ** 2                          # likelihood only
    slots[..., 8:] = per.reshape(Qn, nc, 20)
    weights = np.tile(np.array([1000.0, 1001.0, 1003.0, 0.0]), (Qn, 4, 1))
    weights[1, 2, 3] = 4.0
    cols = np.zeros((Qn, nc, 5, 4))
    cols[..., 0], cols[..., 1], cols[..., 2] = 1000.0, 100.0, 1010.0               # mean 0.1, sd 1 in d
    cols[:, :, 1:, 1] = 110.0                                                       # weighted mean 0.11
    cols[:, :, 1:, 3] = 0.004
    res = sn.finalize(slots, weights, cols, 0.01, 0.05, 1000, 4096)
    assert res["D"][0, 1, 0] == pytest.approx(0.002) and res["D"][0, 2, 0] == pytest.approx(0.06) and res["D"][1, 1, 1] == pytest.approx(0.09)
    assert [list(r) for r in res["diagnosis"]] == [["none", "none", "prior-dominated (weak likelihood)"],
                                                    ["prior-data conflict", "likelihood-dominated", "none"]]
    sd = np.sqrt(1.01 - 0.01)
    assert res["mean_shift"][0, 0, 0, 0] == pytest.approx(0.01 / sd) and res["base_mean"][0, 0] == pytest.approx(5.1)
    assert res["mean_shift_se"][0, 0, 1, 1] == pytest.approx(0.004 / sd)
    assert res["ess_fraction"][0, 0, 0] == pytest.approx(1001.0 ** 2 / (1000.0 * 1003.0)) and np.all(res["non_finite"] == 0)
    rec = sn.json_record(res, 1, ["pIC50", "Hill", "sigma"])
    json.dumps(rec)
    assert set(rec) == {"delta", "bins", "threshold", "method", "columns", "weights", "flagged_columns"}
    assert rec["flagged_columns"] == ["pIC50", "Hill"] and rec["columns"]["pIC50"]["diagnosis"] == "prior-data conflict"
    assert set(rec["columns"]["Hill"]) == {"diagnosis", "draws", "non_finite", "prior", "likelihood"}
    assert set(rec["columns"]["Hill"]["prior"]) == {"D", "cjs", "mean_shift", "sd_ratio", "mean_shift_se"}
    assert rec["weights"]["likelihood"]["clamped"] == [4, 0] and rec["weights"]["prior"]["non_finite"] == 0
    line = sn.report_line(0, ["a", "b"], [sn.part_of(res, q) for q in range(2)])
    assert "2 pairs" in line and "1 pairs (1 columns) prior-data conflict" in line and "worst D 0.09" in line and "4 clamped" in line
    assert sn.report_line(3, [], []) == "sensitivity [rank 3]: no problems"
