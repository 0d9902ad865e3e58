"""Batch means on a dyadic ladder without a GPU: the host build of phf_batch_means.h (the twin of the kernel) against an independent
numpy restatement bit for bit, bit-identity however the rows are cut, finalize() on AR(1) chains of known autocorrelation time, chains
that sit apart, degenerate inputs, the C ABI's argument validation and the command lines' flags."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO

CSRC = os.path.join(REPO, "pyhillfit_amd", "csrc")

SHIM = r"""
#include "phf_batch_means.h"
int v_levels(int64_t h) { return phf_bm_levels(h); }
int v_fields(int nl) { return PHF_BM_FIELDS(nl); }
int v_s1(int nl, int half, int l) { return phf_bm_s1(nl, half, l); }
int v_s2(int nl, int half, int l) { return phf_bm_s2(nl, half, l); }
int v_x0(int half) { return phf_bm_x0(half); }
/* one accumulate call as the device entry cuts it: rows [num_rows][stride][C] = rows first_row.. of total_rows, columns 0..cols-1,
 * st [cols][fields][C] */
void v_accumulate(const double* rows, int64_t num_rows, int64_t first_row, int64_t total_rows, int stride, int cols, int C, double* st) {
  const int nl = phf_bm_levels(total_rows / 2);
  for (int half = 0; half < 2; ++half) {
    phf_half_segment seg;
    if (!phf_half_cut(total_rows, first_row, num_rows, half, &seg)) continue;
    for (int j = 0; j < cols; ++j)
      for (int c = 0; c < C; ++c)
        phf_bm_rows(rows + ((size_t)seg.offset * stride + j) * C + c, (size_t)stride * C, seg.nr, seg.m0, half,
                    st + (size_t)j * PHF_BM_FIELDS(nl) * C + c, (size_t)C, nl);
  }
}
/* row by row through phf_bm_push alone: x [total_rows][C], st [fields][C] */
void v_push_all(const double* x, int64_t total_rows, int C, double* st) {
  const int nl = phf_bm_levels(total_rows / 2);
  for (int64_t n = 0; n < total_rows; ++n) {
    int64_t m;
    const int half = phf_half_of(total_rows, n, &m);
    if (half < 0) continue;
    for (int c = 0; c < C; ++c) {
      double* s = st + c;
      if (m == 0) s[(size_t)phf_bm_x0(half) * C] = x[n * C + c];
      phf_bm_push(s, (size_t)C, nl, half, m, x[n * C + c] - s[(size_t)phf_bm_x0(half) * C]);
    }
  }
}
double v_variance(double s1, double s2, double n, double b) { return phf_bm_block_mean_variance(s1, s2, n, b); }
"""


def build_shim(directory):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler for the host build of phf_batch_means.h")
    src, so = directory / "shim.c", directory / "libshim.so"
    src.write_text(SHIM)
    # the flags of oracle/Makefile: the host evaluates the operation sequence the kernels do
    subprocess.check_call([cc, "-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-shared",
                           "-I", CSRC, "-o", str(so), str(src), "-lm"])
    lib = C.CDLL(str(so))
    lib.v_variance.restype = C.c_double
    lib.v_variance.argtypes = [C.c_double] * 4
    return lib


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shim(tmp_path_factory.mktemp("batch_means"))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def levels_of(h):
    return int(h).bit_length()


def host_state(lib, rows, cols, cuts=None):
    """the host twin on rows [N][stride][C]: the state [cols][5 NL + 2][C] after feeding the rows in calls that end at `cuts`"""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    N, stride, Cn = rows.shape
    nl = levels_of(N // 2)
    st = np.zeros((cols, 5 * nl + 2, Cn))
    cuts = [N] if cuts is None else sorted(set(int(c) for c in cuts if 0 < c < N)) + [N]
    first = 0
    for end in cuts:
        seg = np.ascontiguousarray(rows[first:end])
        lib.v_accumulate(_p(seg), C.c_int64(end - first), C.c_int64(first), C.c_int64(N), C.c_int(stride), C.c_int(cols), C.c_int(Cn), _p(st))
        first = end
    return st


def numpy_ladder(x):
    """the restatement on x [N][...]: (x0 [2][...], S1 [2][NL][...], S2 [2][NL][...]).  Block sums by repeated a[0::2] + a[1::2]
    (left + right), S1 and S2 by sequential sums (cumsum adds one term after the other) starting from 0."""
    x = np.asarray(x, dtype=np.float64)
    N = x.shape[0]
    h = N // 2
    nl = levels_of(h)
    x0 = np.zeros((2,) + x.shape[1:])
    S1 = np.zeros((2, nl) + x.shape[1:])
    S2 = np.zeros_like(S1)
    zero = np.zeros((1,) + x.shape[1:])
    for half in (0, 1):
        seg = x[:h] if half == 0 else x[N - h:]
        x0[half] = seg[0]
        a = seg - seg[0]
        for l in range(nl):
            S1[half, l] = np.cumsum(np.concatenate([zero, a]), axis=0)[-1]
            S2[half, l] = np.cumsum(np.concatenate([zero, a * a]), axis=0)[-1]
            n2 = 2 * (a.shape[0] // 2)
            a = a[0:n2:2] + a[1:n2:2]
    return x0, S1, S2


def numpy_reduced(x):
    """what phf_batch_means_reduce writes for ONE column, x [N][C], from the restated S1 and S2: [NL + 1]"""
    x0, S1, S2 = numpy_ladder(x)
    N, Cn = x.shape
    h = N // 2
    nl = levels_of(h)
    out = np.zeros(nl + 1)
    for l in range(nl - 1):
        n, b = float(h >> l), float(1 << l)
        v = (S2[:, l] - S1[:, l] * S1[:, l] / n) / ((n - 1.0) * (b * b))                # [2][C]
        out[l] = v.sum() / (2.0 * Cn)
    means = x0 + S1[:, 0] / float(h)
    out[nl - 1] = means.mean()
    out[nl] = means.var(ddof=1)
    return out


def state_fields(lib, st, nl):
    """(x0 [2][C], S1 [2][NL][C], S2 [2][NL][C]) of one column's state [fields][C]"""
    x0 = np.stack([st[lib.v_x0(half)] for half in (0, 1)])
    S1 = np.stack([np.stack([st[lib.v_s1(nl, half, l)] for l in range(nl)]) for half in (0, 1)])
    S2 = np.stack([np.stack([st[lib.v_s2(nl, half, l)] for l in range(nl)]) for half in (0, 1)])
    return x0, S1, S2


def make_rows(N, cols, stride, chains, seed):
    """rows [N][stride][chains]: column 0 a pIC50-like 4.548 +- 0.002 (the shift matters), column 1 a log-target near -40, the others
    unit normal random walks' increments"""
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((N, stride, chains))
    rows[:, 0] = 4.548 + 0.002 * rows[:, 0]
    if stride > 1:
        rows[:, 1] = -40.0 + np.cumsum(rows[:, 1], axis=0) * 0.1
    return rows


def ar1(phi, chains, n, seed, offset_sd=0.0):
    """[n][chains]: stationary AR(1) of unit innovation variance, started in its stationary law; + a per-chain offset"""
    rng = np.random.default_rng(seed)
    x = np.empty((n, chains))
    x[0] = rng.standard_normal(chains) / np.sqrt(1.0 - phi * phi)
    e = rng.standard_normal((n, chains))
    for t in range(1, n):
        x[t] = phi * x[t - 1] + e[t]
    if offset_sd:
        x += offset_sd / np.sqrt(1.0 - phi * phi) * rng.standard_normal(chains)
    return x


# ---- 1. the twin against the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("odd", [0, 1])
@pytest.mark.parametrize("h", [1, 2, 3, 31, 32, 33, 513])
def test_twin_against_numpy(shim, h, odd):
    N = 2 * h + odd
    nl = levels_of(h)
    assert shim.v_levels(C.c_int64(h)) == nl and shim.v_fields(nl) == 5 * nl + 2
    rows = make_rows(N, 2, 2, 3, seed=100 + N)
    want = [numpy_ladder(rows[:, j]) for j in range(2)]
    by_row = host_state(shim, rows, 2, cuts=range(1, N))                     # fed row by row
    pushed = np.zeros((2, 5 * nl + 2, 3))
    for j in range(2):
        shim.v_push_all(_p(np.ascontiguousarray(rows[:, j])), C.c_int64(N), C.c_int(3), _p(pushed[j]))
    whole = host_state(shim, rows, 2)                                        # one call: the aligned groups of 32 rows
    for j in range(2):
        got = state_fields(shim, by_row[j], nl)
        for g, w, name in zip(got, want[j], ("x0", "S1", "S2")):
            assert _same_bits(g, w), (name, h, odd, j)
    assert _same_bits(by_row, pushed) and _same_bits(by_row, whole)
    if h >= 2:
        assert np.all(want[0][2][:, 0] > 0)                                  # the columns moved


def test_cut_anywhere_same_bits(shim):
    """the same rows in one call, in calls of 1, 31, 32, 33 rows, cut at h-1, h, h+1 and around the second half's start"""
    for N in (70, 1027, 2048):
        h = N // 2
        rows = make_rows(N, 3, 5, 2, seed=N)
        whole = host_state(shim, rows, 3)
        for cuts in (range(1, N), range(31, N, 31), range(32, N, 32), range(33, N, 33), [h - 1], [h], [h + 1], [N - h - 1, N - h, N - h + 1],
                     [5, 37, h - 1, h + 40]):
            assert _same_bits(host_state(shim, rows, 3, cuts), whole), (N, list(cuts)[:4])


def test_ladder_is_the_variance_of_batch_means(shim):
    """the reduced ladder from S1 and S2 against numpy's variance of the batch means themselves (no shift, no running sums): the two
    differ by the cancellation in S2 - S1^2/n, at most ~ 2^-52 * (rows of a half) * (mean shift / sd)^2 * batches, far below 1e-9 here"""
    x = ar1(0.9, 4, 2 * 513 + 1, seed=3)
    N, Cn = x.shape
    h = N // 2
    red = numpy_reduced(x)
    for l in range(levels_of(h) - 1):
        b, n = 1 << l, h >> l
        v = [seg[:n * b].reshape(n, b, Cn).mean(axis=1).var(axis=0, ddof=1) for seg in (x[:h], x[N - h:])]
        assert abs(red[l] / np.mean(v) - 1.0) < 1e-9, l
    assert shim.v_variance(10.0, 60.0, 2.0, 4.0) == (60.0 - 100.0 / 2.0) / (1.0 * 16.0)


# ---- 2. the estimator ----------------------------------------------------------------------------------------------------------------
def reduced_of(x):
    """[cols][NL+1] of x [N][cols][C]"""
    return np.stack([numpy_reduced(x[:, j]) for j in range(x.shape[1])])


AR_CHAINS, AR_ROWS = 64, 16384
AR_SEEDS = {0.0: 11, 0.5: 12, 0.9: 13, 0.99: 14}


@pytest.fixture(scope="module")
def ar_data():
    return {phi: ar1(phi, AR_CHAINS, AR_ROWS, seed) for phi, seed in AR_SEEDS.items()}


@pytest.mark.parametrize("phi", sorted(AR_SEEDS))
def test_finalize_on_ar1(ar_data, phi):
    """|tau_hat / tau - 1| <= 4 tau_rel_se + tau / (2 batch_rows): four of the estimate's own standard errors + the first-order bias"""
    from pyhillfit_amd import batch_means as bm
    x = ar_data[phi]
    res = bm.finalize(reduced_of(x[:, None, :]), AR_ROWS // 2, 2 * AR_CHAINS)
    tau = (1.0 + phi) / (1.0 - phi)
    got, rel, rows = float(res["tau"][0]), float(res["tau_rel_se"][0]), int(res["batch_rows"][0])
    print("phi %g: tau %.2f, tau_hat %.2f (ratio %.3f), rel se %.4f, batch rows %d, lugsail %.2f" % (phi, tau, got, got / tau, rel, rows,
                                                                                                   float(res["tau_lugsail"][0])))
    assert bool(res["plateau_reached"][0]) and bool(res["chains_agree"][0])
    assert abs(got / tau - 1.0) <= 4.0 * rel + tau / (2.0 * rows)
    n_draws = AR_CHAINS * 2 * (AR_ROWS // 2)
    assert float(res["ess"][0]) == n_draws / got
    h = AR_ROWS // 2
    varp = np.mean([s.var(axis=0, ddof=1) for s in (x[:h], x[h:])]) * (h - 1.0) / h + np.concatenate([x[:h].mean(0), x[h:].mean(0)]).var(ddof=1)
    assert abs(float(res["mcse_mean"][0]) / np.sqrt(varp * got / n_draws) - 1.0) < 1e-9
    assert rows == 1 << int(res["level"][0]) or rows == h
    assert np.isnan(res["ess_upper_bound"][0])


def geyer_inputs(x, lags):
    """mean over the half-chains of acov(k), k = 0..lags, and the variance of their means, as phf_diagnostics_reduce gives them"""
    N, Cn = x.shape
    h = N // 2
    halves = np.concatenate([x[:h], x[N - h:]], axis=1)
    means = halves.mean(axis=0)
    y = halves - means
    acov = np.array([np.mean(np.sum(y[:h - k] * y[k:], axis=0) / h) for k in range(lags + 1)])
    return acov, means.var(ddof=1), h, 2 * Cn


def test_geyer_at_256_lags_gives_up_where_the_ladder_does_not(ar_data):
    """the gap being closed: phi = 0.99 (tau = 199) has no ESS from 256 lags"""
    from pyhillfit_amd import diagnostics as dg
    acov, bh, h, M = geyer_inputs(ar_data[0.99], 256)
    rhat, ess, mcse, limit = dg.finalize(acov[None], np.array([bh]), h, M)
    assert np.isnan(ess[0]) and np.isnan(mcse[0]) and bool(limit[0]) and np.isfinite(rhat[0])
    acov, bh, h, M = geyer_inputs(ar_data[0.9], 256)                          # where Geyer works, the two agree
    ess9 = dg.finalize(acov[None], np.array([bh]), h, M)[1][0]
    from pyhillfit_amd import batch_means as bm
    res = bm.finalize(reduced_of(ar_data[0.9][:, None, :]), h, M)
    assert abs(float(res["ess"][0]) / ess9 - 1.0) < 4.0 * float(res["tau_rel_se"][0]) + 19.0 / (2.0 * int(res["batch_rows"][0]))


def test_chains_that_sit_apart():
    from pyhillfit_amd import batch_means as bm
    x = ar1(0.5, AR_CHAINS, AR_ROWS, seed=21, offset_sd=5.0)
    res = bm.finalize(reduced_of(x[:, None, :]), AR_ROWS // 2, 2 * AR_CHAINS)
    assert bool(res["plateau_reached"][0]) and not bool(res["chains_agree"][0])
    assert np.isnan(res["ess"][0]) and np.isnan(res["mcse_mean"][0]) and np.isnan(res["tau"][0])
    bound = float(res["ess_upper_bound"][0])
    assert np.isfinite(bound) and 0 < bound < 2 * AR_CHAINS * 4                # about one draw per chain, far below the 10^6 rows
    rec = bm.json_record({k: v[None] for k, v in res.items()}, 0)
    assert rec["ess"] == [None] and rec["chains_agree"] == [False] and rec["ess_upper_bound"] == [bound] and "method" in rec
    assert sorted(rec) == sorted(bm.FIELDS + ("method",))


def test_constant_column_and_shapes():
    from pyhillfit_amd import batch_means as bm
    x = np.stack([np.full((200, 4), 3.25), ar1(0.3, 4, 200, seed=5)], axis=1)      # [200][2][4]
    res = bm.finalize(reduced_of(x), 100, 8)
    for k in ("ess", "mcse_mean", "tau", "tau_rel_se", "tau_lugsail", "ess_upper_bound"):
        assert np.isnan(res[k][0]), k
    assert not res["plateau_reached"][0] and not res["chains_agree"][0]
    rec = bm.json_record({k: v[None] for k, v in res.items()}, 0)
    assert [rec[k][0] for k in bm.FIELDS if k not in ("plateau_reached", "chains_agree")] == [None] * 8
    assert np.isfinite(res["ess"][1]) and rec["ess"][1] == float(res["ess"][1])
    assert bm.levels(200) == 7 and bm.levels(4) == 2 and bm.levels(2 * 513 + 1) == 10
    with pytest.raises(ValueError):
        bm.finalize(np.zeros((1, 5)), 100, 8)                                 # NL + 1 = 8 values expected
    with pytest.raises(ValueError):
        bm.finalize(np.zeros((1, 8)), 100, 1)
    line = bm.report_line(2, ["A + x", "B + y"], [np.array([np.nan, 5.0]), np.array([np.nan, 7.0])],
                          [np.array([10.0, 5.0]), np.array([np.nan, 7.0])], [np.array([3.0, 1.0]), np.array([np.nan, 40.0])], 5)
    assert "rank 2" in line and "1 of 2" in line and "200 iterations (B + y)" in line


# ---- 3. the C ABI without a GPU --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from pyhillfit_amd import _lib
    return _lib.load()


def test_abi_validation(lib):
    fake = C.c_void_p(8)
    big = C.c_size_t(1 << 40)
    for h in (2, 3, 31, 32, 513, 100000):
        nl = levels_of(h)
        assert lib.phf_batch_means_levels(2 * h + 1) == nl
        assert lib.phf_batch_means_workspace_bytes(3, 5, 70, 2 * h) == 3 * 5 * 70 * (5 * nl + 2) * 8
    for bad in ((0, 1, 1, 100), (1, 0, 1, 100), (1, 1, 0, 100), (-1, 1, 1, 100), (1, -2, 1, 100), (1, 1, -64, 100)):
        assert lib.phf_batch_means_workspace_bytes(*bad) == 0 and b"positive" in lib.phf_last_error()
        assert lib.phf_batch_means_init(*bad, fake, big, None) == -1
        assert lib.phf_batch_means_reduce(*bad, fake, big, fake, None) == -1
    for rows in (3, 0, -8):
        assert lib.phf_batch_means_workspace_bytes(1, 1, 1, rows) == 0 and b"total_rows" in lib.phf_last_error()
        assert lib.phf_batch_means_levels(rows) == -1
    need = lib.phf_batch_means_workspace_bytes(2, 3, 64, 100)
    assert lib.phf_batch_means_init(2, 3, 64, 100, None, big, None) == -1 and b"null workspace" in lib.phf_last_error()
    assert lib.phf_batch_means_init(2, 3, 64, 100, fake, C.c_size_t(need - 1), None) == -1 and b"workspace smaller" in lib.phf_last_error()

    def acc(rows=fake, n=10, Q=2, stride=5, chains=64, cols=3, first=0, total=100, ws=fake, wb=big):
        return lib.phf_batch_means_accumulate(rows, n, Q, stride, chains, cols, first, total, ws, wb, None)

    assert acc(n=101) == -1 and b"must lie in [0, total_rows)" in lib.phf_last_error()
    assert acc(first=95) == -1 and acc(first=-1) == -1 and acc(n=-1) == -1
    assert acc(stride=2) == -1 and b"row_stride_cols" in lib.phf_last_error()
    assert acc(rows=None) == -1 and acc(ws=None) == -1 and b"null pointer" in lib.phf_last_error()
    assert acc(wb=C.c_size_t(need - 1)) == -1 and b"workspace smaller" in lib.phf_last_error()
    assert acc(Q=0) == -1 and acc(total=3) == -1
    assert acc(n=0) == 0                                                        # nothing to do: no launch
    assert lib.phf_batch_means_reduce(2, 3, 64, 100, None, big, fake, None) == -1 and b"null pointer" in lib.phf_last_error()
    assert lib.phf_batch_means_reduce(2, 3, 64, 100, fake, big, None, None) == -1
    assert lib.phf_batch_means_reduce(2, 3, 64, 100, fake, C.c_size_t(need - 1), fake, None) == -1 and b"workspace smaller" in lib.phf_last_error()
    from pyhillfit_amd import batch_means as bm
    assert bm.workspace_bytes(2, 3, 64, 100) == need
    with pytest.raises(ValueError, match="total_rows"):
        bm.workspace_bytes(2, 3, 64, 2)
    with pytest.raises(ValueError, match="GPU device"):
        bm.BatchMeans(1, 64, 3, 100, device="cpu")


# ---- 4. the flags ----------------------------------------------------------------------------------------------------------------
def test_parser_flags():
    from pyhillfit_amd import PyHillFit, PyHillTemp, chain_diagnostics
    p = PyHillFit.build_parser()
    a = p.parse_args(["--data-file", "x.csv", "-m", "2"])
    PyHillFit.check_args(p, a)
    assert a.diagnostic_batch_means is False
    for extra in ([], ["--hierarchical"]):
        a = p.parse_args(["--data-file", "x.csv", "-m", "2", "--diagnostics", "--diagnostic-batch-means"] + extra)
        PyHillFit.check_args(p, a)
        assert a.diagnostic_batch_means is True and a.diagnostics is True
    t = PyHillTemp.build_parser()
    base = ["--data-file", "x.csv", "-m", "2", "-d", "0", "-c", "0"]
    assert t.parse_args(base).diagnostic_batch_means is False
    assert t.parse_args(base + ["--diagnostics", "--diagnostic-batch-means"]).diagnostic_batch_means is True
    assert "batch_means" in chain_diagnostics.diagnose_file.__code__.co_varnames


@pytest.mark.parametrize("tool,argv", [
    ("PyHillFit", ["--data-file", "does-not-exist.csv", "-m", "2", "--diagnostic-batch-means"]),
    ("PyHillFit", ["--data-file", "does-not-exist.csv", "-m", "2", "--hierarchical", "--diagnostic-batch-means"]),
    ("PyHillTemp", ["--data-file", "does-not-exist.csv", "-m", "2", "-d", "0", "-c", "0", "--diagnostic-batch-means"]),
])
def test_flag_needs_diagnostics(tool, argv, capsys):
    import importlib
    mod = importlib.import_module("pyhillfit_amd." + tool)
    with pytest.raises(SystemExit) as e:
        mod.main(argv)
    assert e.value.code == 2
    assert "--diagnostic-batch-means needs --diagnostics" in capsys.readouterr().err
