"""Hierarchical dose-response bands without a GPU: the host build of phf_hier_bands.h (the uniforms exactly, the log-logistic and
logistic draws against scipy, their distribution, the random stream's counter domain), the C ABI's argument validation, the
command lines' flags and the "hierarchical_bands" record."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest
from scipy import stats

from conftest import REPO

CSRC = os.path.join(REPO, "pyhillfit_amd", "csrc")

SHIM = r"""
#include "phf_hier_bands.h"
#include "phf_ppc.h"
uint32_t band_domain(void) { return PHF_BAND_DOMAIN; }
uint32_t ppc_domain(void) { return PHF_PPC_DOMAIN; }
void v_uniform(int64_t n, const uint32_t* wa, const uint32_t* wb, double* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = phf_band_uniform(wa[i], wb[i]);
}
void v_logit(int64_t n, const double* u, double* out) { for (int64_t i = 0; i < n; ++i) out[i] = phf_band_logit(u[i]); }
/* the quantile functions at given uniforms: theta [4][n] */
void v_quantiles(int64_t n, const double* th, const double* uh, const double* up, double* out) {
  for (int64_t i = 0; i < n; ++i) {
    out[2 * i] = phf_band_hill_k(th[i], th[n + i], uh[i], phf_k_exp, phf_k_log);
    out[2 * i + 1] = phf_band_pic50_k(th[2 * n + i], th[3 * n + i], up[i], phf_k_log);
  }
}
void v_block(uint32_t cid, uint32_t pid, uint32_t row, uint64_t seed, uint32_t* w) {
  const phf_u32x4 b = phf_philox_mh(cid, pid, row, PHF_BAND_DOMAIN, (uint32_t)seed, (uint32_t)(seed >> 32));
  for (int k = 0; k < 4; ++k) w[k] = b.w[k];
}
/* phf_hier_band_draws on the host: theta [4][m], counter [m][3], out [m][2] */
void v_draws(int64_t m, const double* th, const uint32_t* ctr, uint64_t seed, double* out) {
  for (int64_t i = 0; i < m; ++i)
    phf_band_future(th[i], th[m + i], th[2 * m + i], th[3 * m + i], ctr[3 * i], ctr[3 * i + 1], ctr[3 * i + 2], (uint32_t)seed,
                    (uint32_t)(seed >> 32), &out[2 * i], &out[2 * i + 1]);
}
/* the value a band slot bins, kind 0 (underlying) | 1 (future experiment), at ln_dose */
void v_values(int kind, double ln_dose, int64_t m, const double* th, const uint32_t* ctr, uint64_t seed, double* out) {
  for (int64_t i = 0; i < m; ++i)
    out[i] = phf_band_value(kind, ln_dose, th[i], th[m + i], th[2 * m + i], th[3 * m + i], ctr[3 * i], ctr[3 * i + 1], ctr[3 * i + 2],
                            (uint32_t)seed, (uint32_t)(seed >> 32));
}
"""


def build_shim(directory):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler for the host build of phf_hier_bands.h")
    src, so = directory / "shim.c", directory / "libshim.so"
    src.write_text(SHIM)
    # the flags of oracle/Makefile: the host evaluates the operation sequence the kernels do
    subprocess.check_call([cc, "-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-shared",
                           "-I", CSRC, "-o", str(so), str(src), "-lm"])
    lib = C.CDLL(str(so))
    lib.band_domain.restype = C.c_uint32
    lib.ppc_domain.restype = C.c_uint32
    return lib


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shim(tmp_path_factory.mktemp("hier_bands"))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _u32(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint32)


def uniforms(lib, wa, wb):
    wa, wb = _u32(wa), _u32(wb)
    out = np.empty(wa.size)
    lib.v_uniform(C.c_int64(wa.size), _p(wa), _p(wb), _p(out))
    return out


def logit(lib, u):
    u = np.ascontiguousarray(u, dtype=np.float64)
    out = np.empty_like(u)
    lib.v_logit(C.c_int64(u.size), _p(u), _p(out))
    return out


def quantile_draws(lib, theta, uh, up):
    """theta [m][4], uniforms [m] -> (Hill*, pIC50*) [m][2]"""
    th = np.ascontiguousarray(np.asarray(theta, dtype=np.float64).reshape(-1, 4).T)
    uh, up = np.ascontiguousarray(uh, dtype=np.float64), np.ascontiguousarray(up, dtype=np.float64)
    out = np.empty((th.shape[1], 2))
    lib.v_quantiles(C.c_int64(th.shape[1]), _p(th), _p(uh), _p(up), _p(out))
    return out


def host_draws(lib, theta, counters, seed):
    """phf_hier_band_draws on the host: theta [m][4], counters [m][3] -> [m][2]"""
    th = np.ascontiguousarray(np.asarray(theta, dtype=np.float64).reshape(-1, 4).T)
    ct = _u32(np.asarray(counters).reshape(-1, 3))
    out = np.empty((th.shape[1], 2))
    lib.v_draws(C.c_int64(th.shape[1]), _p(th), _p(ct), C.c_uint64(seed), _p(out))
    return out


def host_values(lib, kind, ln_dose, theta, counters, seed):
    th = np.ascontiguousarray(np.asarray(theta, dtype=np.float64).reshape(-1, 4).T)
    ct = _u32(np.asarray(counters).reshape(-1, 3))
    out = np.empty(th.shape[1])
    lib.v_values(C.c_int(kind), C.c_double(ln_dose), C.c_int64(th.shape[1]), _p(th), _p(ct), C.c_uint64(seed), _p(out))
    return out


def host_band_values(lib, rows, ln_doses, problem_ids, chain_id_base, seed, first_row=0):
    """rows [n][Q][stride][C] (hierarchical: columns 0..3) -> the values of the 2 D band slots, [Q][2 D][n][C]: the underlying
    effect's D doses, then the future experiment's"""
    n, Q, _, Cn = rows.shape
    D = ln_doses.shape[1]
    out = np.empty((Q, 2 * D, n, Cn))
    r, c = np.meshgrid(np.arange(n), np.arange(Cn), indexing="ij")
    for q in range(Q):
        theta = rows[:, q, :4, :].transpose(0, 2, 1).reshape(-1, 4)
        ctr = np.stack([chain_id_base + c.ravel(), np.full(n * Cn, problem_ids[q]), first_row + r.ravel()], axis=1)
        for kind in (0, 1):
            for g in range(D):
                out[q, kind * D + g] = host_values(lib, kind, float(ln_doses[q, g]), theta, ctr, seed).reshape(n, Cn)
    return out


# ---- 1. the uniforms -----------------------------------------------------------------------------------------------------------
def test_uniforms_are_exact_and_open(shim):
    rng = np.random.default_rng(1)
    wa = np.concatenate([rng.integers(0, 2 ** 32, 4000), [0, 0xFFFFFFFF, 0, 0xFFFFFFFF, 63, 64]])
    wb = np.concatenate([rng.integers(0, 2 ** 32, 4000), [0, 0xFFFFFFFF, 0xFFFFFFFF, 0, 63, 64]])
    u = uniforms(shim, wa, wb)
    for a, b, x in zip(wa.tolist(), wb.tolist(), u.tolist()):
        k = (a >> 6) * 2 ** 26 + (b >> 6)
        want = Fraction(2 * k + 1, 2 ** 53)                              # (k + 1/2) 2^-52
        assert Fraction(x) == want
        assert Fraction(1.0 - x) == 1 - want                             # 1 - u is exact too
    assert u.min() >= 2.0 ** -53 and u.max() <= 1.0 - 2.0 ** -53
    ends = uniforms(shim, [0, 0xFFFFFFFF], [0, 0xFFFFFFFF])
    assert ends[0] == 2.0 ** -53 and ends[1] == 1.0 - 2.0 ** -53
    assert np.all(np.abs(logit(shim, ends)) <= 36.8)


# ---- 2. the draws against scipy ---------------------------------------------------------------------------------------------------
def _full_range_uniforms(rng, n):
    """uniforms of the generator's form (k + 1/2) 2^-52 over its whole range: both tails down to 2^-53, and the bulk"""
    k = np.concatenate([rng.integers(0, 2 ** 52, n), (2.0 ** rng.uniform(0, 52, n)).astype(np.int64),
                        2 ** 52 - 1 - (2.0 ** rng.uniform(0, 52, n)).astype(np.int64), [0, 2 ** 52 - 1, 2 ** 51]])
    k = np.clip(k, 0, 2 ** 52 - 1)
    return (k.astype(np.float64) + 0.5) * 2.0 ** -52                     # k < 2^52: k + 1/2 is exact


def test_draws_against_scipy(shim):
    """phf_log <= 2 ulp, phf_exp <= 1 ulp: |d logit| <= 8 ulp(max(|ln u|, |ln(1 - u)|)), so
    |d pIC50*| <= 1e-14 (|mu| + s max(1, |logit|)) and |d Hill*| / Hill* <= 1e-14 (1 + |logit| / beta), a factor ~10 over that"""
    rng = np.random.default_rng(2)
    uh, up = _full_range_uniforms(rng, 20000), _full_range_uniforms(rng, 20000)[::-1].copy()
    m = uh.size
    alpha, beta = rng.uniform(0.3, 3, m), rng.uniform(0.5, 20, m)
    mu, s = rng.uniform(2, 9, m), rng.uniform(0.05, 2, m)
    got = quantile_draws(shim, np.column_stack([alpha, beta, mu, s]), uh, up)
    assert np.all(np.isfinite(got))
    lh, lp = np.log(uh) - np.log1p(-uh), np.log(up) - np.log1p(-up)
    # scipy's fisk.ppf(q) is (1/q - 1)^(-1/c): 1/q - 1 cancels for q near 1 (at q = 1 - 2^-53 it is 2^-52, twice the truth, and
    # the quantile is off by 2^(1/c)), while its isf(q) = (1/q - 1)^(1/c) is accurate for small q — and 1 - u is exact here.  So the
    # reference is scipy's quantile function through the branch that is accurate: ppf(u) below 1/2, isf(1 - u) above.
    want_h = np.where(uh <= 0.5, stats.fisk.ppf(uh, c=beta, scale=alpha), stats.fisk.isf(1.0 - uh, c=beta, scale=alpha))
    want_p = stats.logistic.ppf(up, mu, s)
    assert np.all(np.abs(got[:, 1] - want_p) <= 1e-14 * (np.abs(mu) + s * np.maximum(1.0, np.abs(lp))))
    assert np.all(np.abs(got[:, 0] - want_h) / want_h <= 1e-14 * (1.0 + np.abs(lh) / beta))
    # logit is antisymmetric bit for bit under u <-> 1 - u (1 - u is exact)
    u = np.concatenate([uh, up])
    assert np.array_equal(logit(shim, 1.0 - u), -logit(shim, u))
    assert np.all(np.abs(logit(shim, u)) <= 36.8)


def test_invalid_parameters_give_nan(shim):
    good = [1.0, 3.0, 6.0, 0.3]
    ctr = [[5, 7, 11]]
    assert np.all(np.isfinite(host_draws(shim, [good], ctr, 25)))
    for i, bad in [(0, np.nan), (1, np.inf), (2, -np.inf), (3, np.nan), (0, 0.0), (0, -1.0), (1, 0.0), (1, -2.0), (3, 0.0), (3, -0.1)]:
        th = list(good)
        th[i] = bad
        assert np.all(np.isnan(host_draws(shim, [th], ctr, 25))), (i, bad)
        assert np.isnan(host_values(shim, 1, 0.0, [th], ctr, 25)[0])
        # the underlying effect needs no s > 0, only a finite one
        under = host_values(shim, 0, 0.0, [th], ctr, 25)[0]
        assert np.isnan(under) == (not (i == 3 and np.isfinite(bad))), (i, bad)
    # the underlying effect is the Hill curve at Hill = alpha, pIC50 = mu
    from pyhillfit_amd.quantiles import hill_curve
    v = host_values(shim, 0, np.log(3.0), [good], ctr, 25)[0]
    assert v == pytest.approx(float(hill_curve(2, np.log(3.0), 6.0, 1.0)), rel=1e-13)


def test_draws_are_addressed_by_the_counter(shim):
    """a draw is a function of (chain id, problem id, row, seed) alone; the block's words (0, 1) give Hill*, (2, 3) pIC50*"""
    th = [1.3, 4.0, 5.5, 0.4]
    base = host_draws(shim, [th], [[3, 9, 1234]], 25)[0]
    w = (C.c_uint32 * 4)()
    shim.v_block(C.c_uint32(3), C.c_uint32(9), C.c_uint32(1234), C.c_uint64(25), w)
    want = quantile_draws(shim, [th], uniforms(shim, [w[0]], [w[1]]), uniforms(shim, [w[2]], [w[3]]))[0]
    assert np.array_equal(base, want)
    for ctr, seed in (([4, 9, 1234], 25), ([3, 10, 1234], 25), ([3, 9, 1235], 25), ([3, 9, 1234], 26), ([3, 9, 1234], 25 + 2 ** 32)):
        other = host_draws(shim, [th], [ctr], seed)[0]
        assert other[0] != base[0] and other[1] != base[1]
    # every dose of a draw sees the same (Hill*, pIC50*)
    from pyhillfit_amd.quantiles import hill_curve
    for dose in (0.01, 1.0, 300.0):
        v = host_values(shim, 1, np.log(dose), [th], [[3, 9, 1234]], 25)[0]
        assert v == pytest.approx(float(hill_curve(2, np.log(dose), base[1], base[0])), rel=1e-12, abs=1e-12)


# ---- 3. the distribution ---------------------------------------------------------------------------------------------------------
def sup_distance(sample, cdf_of):
    """sup over a grid of |empirical CDF - cdf_of(grid)|"""
    x = np.sort(sample)
    grid = np.quantile(x, np.linspace(0.001, 0.999, 400))
    emp = np.searchsorted(x, grid, side="right") / x.size
    return float(np.max(np.abs(emp - cdf_of(grid))))


def test_distribution_of_the_draws(shim):
    """12 800 draws, 200 random rows x 64 chain ids, against the average of the rows' own log-logistic / logistic CDFs.  DKW for
    independent draws: P(sup > 0.03) <= 2 exp(-2 12800 0.03^2) ~ 2e-10 — a correct draw cannot fail at any seed"""
    rng = np.random.default_rng(3)
    R, Cn = 200, 64
    par = np.column_stack([rng.uniform(0.3, 3, R), rng.uniform(0.5, 20, R), rng.uniform(2, 9, R), rng.uniform(0.05, 2, R)])
    theta = np.repeat(par, Cn, axis=0)
    ctr = np.stack([np.tile(np.arange(Cn), R), np.full(R * Cn, 17), np.repeat(np.arange(R) + 1000, Cn)], axis=1)
    d = host_draws(shim, theta, ctr, 25)
    assert d.shape == (12800, 2) and np.all(np.isfinite(d))
    hill_cdf = lambda x: np.mean(stats.fisk.cdf(x[:, None], c=par[:, 1], scale=par[:, 0]), axis=1)
    pic50_cdf = lambda x: np.mean(stats.logistic.cdf(x[:, None], par[:, 2], par[:, 3]), axis=1)
    assert sup_distance(d[:, 0], hill_cdf) <= 0.03
    assert sup_distance(d[:, 1], pic50_cdf) <= 0.03
    # the two uniforms of a draw come from different words: not the same quantile of both distributions
    uh = stats.fisk.cdf(d[:, 0], c=theta[:, 1], scale=theta[:, 0])
    up = stats.logistic.cdf(d[:, 1], theta[:, 2], theta[:, 3])
    assert abs(np.corrcoef(uh, up)[0, 1]) < 0.05                          # 5.6 sigma of 1/sqrt(12800)


# ---- 4. the counter domain -------------------------------------------------------------------------------------------------------
def test_counter_domain_is_its_own(shim):
    from pyhillfit_amd.hierarchical import MAX_EXPTS
    dom, ppc = shim.band_domain(), shim.ppc_domain()
    assert dom == 0xC0000000
    # PHF_PPC_DOMAIN | b, b < 2^30, never sets bit 30; the band domain has it set
    assert ppc == 0x80000000 and (ppc | (2 ** 30 - 1)) & 0x40000000 == 0 and dom & 0x40000000
    assert all((ppc | b) != dom for b in (0, 1, 127, 2 ** 30 - 1))
    rx = re.search(r"#define PHF_RX_DOMAIN (0x[0-9a-fA-F]+)u", open(os.path.join(CSRC, "phf_replica_exchange.hip")).read())
    assert int(rx.group(1), 16) == 0x40000000 != dom
    assert (5 + 2 * MAX_EXPTS + 3) // 4 - 1 < 0x40000000                  # the samplers' largest block index
    # every sampler draw in the sources: word 3 is 0u or a block index (a small loop variable), never a domain constant
    calls = []
    for name in ("phf_model.h", "phf_hier_model.h", "phf_hierarchical.hip", "phf_single_level.hip"):
        src = open(os.path.join(CSRC, name)).read()
        calls += re.findall(r"phf_philox_mh\(([^;]*?)\);", src, flags=re.S)
    assert calls
    for c in calls:
        args = [a.strip() for a in c.split(",")]
        assert len(args) == 6, c
        assert "DOMAIN" not in args[3] and "0x" not in args[3].lower(), c
    # the band draws use it, and only through the header
    band = open(os.path.join(CSRC, "phf_hier_bands.h")).read()
    assert re.findall(r"phf_philox_mh\(([^;]*?)\);", band, flags=re.S) == ["chain_id, problem_id, row, PHF_BAND_DOMAIN, k0, k1"]


# ---- 5. the C ABI without a GPU --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from pyhillfit_amd import _lib
    return _lib.load()


def test_abi_validation(lib):
    fake, big = C.c_void_p(8), C.c_size_t(1 << 40)

    def acc(**kw):
        d = dict(rows=fake, n=10, Q=3, stride=8, chains=64, doses=fake, cols=4, D=5, B=1024, first=0, total=100, pid=fake, base=0,
                 seed=25, ws=fake, wsb=big)
        d.update(kw)
        return lib.phf_quantiles_accumulate_hier_curves(d["rows"], d["n"], d["Q"], d["stride"], d["chains"], d["doses"], d["cols"],
                                                        d["D"], d["B"], d["first"], d["total"], d["pid"], d["base"], d["seed"],
                                                        d["ws"], d["wsb"], None)
    assert acc(stride=3) == -1 and b"row_stride_cols" in lib.phf_last_error()
    assert acc(D=0) == -1 and b"num_doses" in lib.phf_last_error()
    assert acc(D=-2) == -1 and b"num_doses" in lib.phf_last_error()
    assert acc(doses=None) == -1 and b"ln_doses" in lib.phf_last_error()
    assert acc(pid=None) == -1 and b"problem_id" in lib.phf_last_error()
    assert acc(rows=None) == -1 and b"null rows" in lib.phf_last_error()
    assert acc(ws=None) == -1 and b"null workspace" in lib.phf_last_error()
    assert acc(wsb=C.c_size_t(8)) == -1 and b"smaller" in lib.phf_last_error()
    assert acc(B=1000) == -1 and b"power of two" in lib.phf_last_error()
    assert acc(Q=0) == -1 and b"num_problems" in lib.phf_last_error()
    assert acc(chains=0) == -1 and b"num_chains" in lib.phf_last_error()
    assert acc(first=95) == -1 and b"total_rows" in lib.phf_last_error()
    assert acc(n=-1) == -1 and b"total_rows" in lib.phf_last_error()
    assert acc(n=1 << 20, chains=4096, total=1 << 21) == -1 and b"2^31" in lib.phf_last_error()
    assert acc(n=0, total=(1 << 32) + 1) == -1 and b"32-bit row word" in lib.phf_last_error()
    assert acc(n=0, first=100) == 0                                       # nothing to do: no launch
    # the workspace of a band is the curve workspace of 2 D points
    S = 3 * (4 + 2 * 5)
    assert lib.phf_quantiles_workspace_bytes(3, 4, 2 * 5, 1024) == S * 1024 * 8 + S * 8 * 8 + S * 8
    assert acc(wsb=C.c_size_t(S * 1024 * 8 + S * 8 * 8 + S * 8 - 1)) == -1 and b"smaller" in lib.phf_last_error()

    def draws(m=1, th=fake, ctr=fake, out=fake):
        return lib.phf_hier_band_draws(m, th, ctr, 25, out, None)
    assert draws(m=-1) == -1 and b"phf_hier_band_draws" in lib.phf_last_error()
    assert draws(th=None) == -1 and b"non-null" in lib.phf_last_error()
    assert draws(ctr=None) == -1 and b"non-null" in lib.phf_last_error()
    assert draws(out=None) == -1 and b"non-null" in lib.phf_last_error()
    assert draws(m=0, th=None, ctr=None, out=None) == 0


def test_python_arguments():
    from pyhillfit_amd import quantiles as qn
    with pytest.raises(ValueError):
        qn.PosteriorQuantiles(1, 4, 4, 10, device="cpu", band_ln_doses=np.zeros((1, 3)))
    with pytest.raises(ValueError):
        qn.hier_band_draws([[1.0, 2.0, 5.0, 0.3]], [[0, 0, 0]], 25, device="cpu")
    assert qn.parse_band_concs("0.1, 10") == (0.1, 10.0)
    for bad in ("0", "-1,2", "", "nan", "inf", ",".join(["1"] * 65)):
        with pytest.raises(ValueError):
            qn.parse_band_concs(bad)
    d = qn.band_doses([0.1, 1.0, 30.0], 4, (0.5, 7.0))
    assert d.shape == (6,) and np.array_equal(d[:4], qn.curve_doses([0.1, 1.0, 30.0], 4)) and d[4:].tolist() == [0.5, 7.0]


# ---- 6. the flags ----------------------------------------------------------------------------------------------------------------
def test_parser_flags():
    from pyhillfit_amd import PyHillFit
    p = PyHillFit.build_parser()
    a = p.parse_args(["--data-file", "x.csv", "-m", "2"])
    PyHillFit.check_args(p, a)
    assert a.predictive_bands == 0 and a.band_concs is None
    a = p.parse_args(["--data-file", "x.csv", "-m", "2", "--hierarchical", "--quantiles", "--predictive-bands", "8", "--band-concs", "0.1,10"])
    PyHillFit.check_args(p, a)
    assert a.predictive_bands == 8 and a.band_concs == (0.1, 10.0)
    a = p.parse_args(["--data-file", "x.csv", "-m", "2", "--hierarchical", "--quantiles", "--predictive-bands", "1"])
    PyHillFit.check_args(p, a)
    assert a.predictive_bands == 1 and a.band_concs is None


@pytest.mark.parametrize("extra,flag", [
    (["--quantiles", "--predictive-bands", "8"], "--predictive-bands"),
    (["--hierarchical", "--predictive-bands", "8"], "--predictive-bands"),
    (["--hierarchical", "--quantiles", "--band-concs", "1"], "--band-concs"),
    (["--hierarchical", "--quantiles", "--predictive-bands", "8", "--band-concs", "0"], "--band-concs"),
    (["--hierarchical", "--quantiles", "--predictive-bands", "-1"], "--predictive-bands"),
    (["--hierarchical", "--quantiles", "--predictive-bands", "8", "--band-concs", ",".join(["1"] * 65)], "--band-concs"),
])
def test_flag_refusals(extra, flag, capsys):
    from pyhillfit_amd import PyHillFit
    with pytest.raises(SystemExit) as e:
        PyHillFit.main(["--data-file", "does-not-exist.csv", "-m", "2"] + extra)
    assert e.value.code == 2
    assert flag in capsys.readouterr().err


def test_chain_tool_refusals(capsys):
    from pyhillfit_amd import chain_quantiles
    for argv, flag in ((["x.txt", "--hier-bands", "8", "--data-file", "d.csv", "--exact"], "--exact"),
                       (["x.txt", "--hier-bands", "8"], "--data-file"),
                       (["x.txt", "--band-concs", "1"], "--band-concs"),
                       (["x.txt", "--hier-bands", "8", "--data-file", "d.csv", "--band-concs", "-3"], "--band-concs"),
                       (["x.txt", "--hier-bands", "-2", "--data-file", "d.csv"], "--hier-bands")):
        with pytest.raises(SystemExit) as e:
            chain_quantiles.main(argv)
        assert e.value.code == 2 and flag in capsys.readouterr().err
    assert chain_quantiles.pair_of_file_name("/a/b/crumb_data_Amiodarone_hERG_hierarchical_chain.txt", ["Amiodarone", "Bepridil"],
                                             ["hERG", "Cav1.2"]) == ("Amiodarone", "hERG")
    # a channel named with '/' is cleaned as the writers clean it; the longest match wins
    assert chain_quantiles.pair_of_file_name("d_X_Kv4.3_KChIP_hierarchical_chain.txt", ["X", "X_Kv4.3"], ["KChIP", "Kv4.3/KChIP"]) \
        == ("X", "Kv4.3/KChIP")
    with pytest.raises(SystemExit):
        chain_quantiles.pair_of_file_name("nothing.txt", ["A"], ["B"])


# ---- 7. the record ---------------------------------------------------------------------------------------------------------------
def test_hier_band_record():
    from pyhillfit_amd import quantiles as qn
    P = qn.DEFAULT_PROBS
    cols, D = 2, 3
    v = np.arange(2 * (cols + 2 * D) * len(P), dtype=float).reshape(2, cols + 2 * D, len(P))
    shape = (2, cols + 2 * D)
    nf = np.zeros(shape)
    nf[1, cols + D + 1] = 4
    res = {"value": v, "lo": v - 0.5, "hi": v + 0.5, "min": np.zeros(shape), "max": np.full(shape, 99.0), "draws": np.full(shape, 1000.0),
           "non_finite": nf, "bin_width": np.full(shape, 0.01), "probs": np.array(P), "columns": cols, "curve_points": 2 * D,
           "band_doses": D, "seed": 25}
    rec = qn.hier_band_record(res, 1, [0.1, 1.0, 7.5], 2)
    assert set(rec) == {"doses", "probs", "grid_points", "named_concentrations", "seed", "method", "underlying", "future_experiment"}
    assert rec["doses"] == [0.1, 1.0, 7.5] and rec["grid_points"] == 2 and rec["named_concentrations"] == [7.5] and rec["seed"] == 25
    assert rec["probs"] == list(P)
    assert "0xC0000000" in rec["method"] and "logit" in rec["method"] and "log-logistic" in rec["method"]
    fields = {"value", "lo", "hi", "min", "max", "bin_width", "ci90", "ci95", "non_finite"}
    for name, first in (("underlying", cols), ("future_experiment", cols + D)):
        part = rec[name]
        assert set(part) == fields
        assert all(len(part[k]) == D for k in fields)
        assert part["value"] == [list(v[1, first + g]) for g in range(D)]
        assert part["lo"][2] == list(v[1, first + 2] - 0.5) and part["hi"][0] == list(v[1, first] + 0.5)
        assert part["ci95"][1] == [v[1, first + 1, 0], v[1, first + 1, 6]] and part["ci90"][1] == [v[1, first + 1, 1], v[1, first + 1, 5]]
        assert part["max"] == [99.0] * D and part["bin_width"] == [0.01] * D
    assert rec["underlying"]["non_finite"] == [0, 0, 0] and rec["future_experiment"]["non_finite"] == [0, 4, 0]
    json.dumps(rec, allow_nan=False)
    with pytest.raises(ValueError):
        qn.hier_band_record(res, 1, [0.1, 1.0], 2)
    # the rank's report line gains the band's non-finite count only when there is a band
    parts = [(np.array([0.01]), np.array([0.0]), np.array([1.0]), np.array([3]))]
    assert qn.report_line(0, ["a + b"], parts).endswith("3 non-finite draws")
    assert qn.report_line(0, ["a + b"], parts, 4).endswith("3 non-finite draws; 4 non-finite band draws")
