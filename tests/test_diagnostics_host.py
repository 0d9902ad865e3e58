"""Convergence diagnostics, host half (no GPU): a direct numpy restatement of split-R-hat / multi-chain ESS / MCSE checked against
known answers, the product's finalize() checked against the restatement, and the C ABI's argument validation."""
import ctypes as C

import numpy as np
import pytest


def restated(x, K=256):
    """x [chains][rows] -> (rhat, ess, mcse, lag_limit_reached, margin): the estimators written out with direct lagged sums.
    margin = smallest |P_t| Geyer's truncation looked at (how far the cut is from flipping)."""
    x = np.asarray(x, dtype=np.float64)
    Cn, N = x.shape
    h = N // 2
    halves = []
    for m in range(Cn):
        halves.append(x[m, :h])
        halves.append(x[m, N - h:])
    M = len(halves)
    L = min(K, h - 1)
    means = np.array([v.mean() for v in halves])
    acov = np.zeros((M, L + 1))
    for i, v in enumerate(halves):
        d = v - means[i]
        for k in range(L + 1):
            acov[i, k] = np.dot(d[:h - k], d[k:]) / h
    W = np.mean(acov[:, 0] * h / (h - 1))
    if W == 0:
        return np.nan, np.nan, np.nan, False, np.inf
    B_h = np.sum((means - means.mean()) ** 2) / (M - 1)
    varp = (h - 1) / h * W + B_h
    rhat = np.sqrt(varp / W)
    rho = [1.0] + [1 - (W - acov[:, k].mean()) / varp for k in range(1, L + 1)]
    P, margin, T, cut = [], np.inf, None, False
    t = 0
    while 2 * t + 1 <= L:
        Pt = rho[2 * t] + rho[2 * t + 1]
        if t > 0:
            margin = min(margin, abs(Pt))
            if Pt <= 0:
                cut = True
                break
        P.append(Pt)
        t += 1
    if not cut and L < h - 1:
        return rhat, np.nan, np.nan, True, margin
    for t in range(1, len(P)):
        P[t] = min(P[t], P[t - 1])
    tau = max(-1 + 2 * sum(P), 1 / np.log10(M * h))
    ess = M * h / tau
    return rhat, ess, np.sqrt(varp / ess), False, margin


def ar1(rng, chains, rows, phi, shift=None):
    x = np.empty((chains, rows))
    x[:, 0] = rng.standard_normal(chains) / np.sqrt(1 - phi ** 2)
    e = rng.standard_normal((chains, rows))
    for n in range(1, rows):
        x[:, n] = phi * x[:, n - 1] + e[:, n]
    if shift is not None:
        x += np.asarray(shift)[:, None]
    return x


def reduced(x, K=256):
    """what phf_diagnostics_reduce returns, computed in numpy: mean acov(0..L) over the half-chains, variance of their means"""
    Cn, N = x.shape
    h = N // 2
    hv = np.concatenate([x[:, :h], x[:, N - h:]], axis=0)
    L = min(K, h - 1)
    d = hv - hv.mean(axis=1, keepdims=True)
    acov = np.array([np.mean(np.sum(d[:, :h - k] * d[:, k:], axis=1) / h) for k in range(L + 1)])
    return acov, np.var(hv.mean(axis=1), ddof=1), h, 2 * Cn


def test_restatement_iid():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((8, 4000))
    rhat, ess, mcse, flag, _ = restated(x)
    assert 0.99 <= rhat <= 1.01
    assert 0.9 <= ess / (16 * 2000) <= 1.1
    assert not flag


@pytest.mark.parametrize("phi", [0.5, 0.9])
def test_restatement_ar1(phi):
    rng = np.random.default_rng(2)
    x = ar1(rng, 16, 8000, phi)
    _, ess, _, flag, _ = restated(x)
    expect = 32 * 4000 * (1 - phi) / (1 + phi)
    assert not flag
    assert abs(ess / expect - 1) < 0.1, (ess, expect)


def test_restatement_shifted_means():
    rng = np.random.default_rng(3)
    x = ar1(rng, 4, 2000, 0.5, shift=[0, 0, 3, 3])
    assert restated(x)[0] > 1.1


@pytest.mark.parametrize("seed,chains,rows,phi,K", [(4, 4, 1000, 0.5, 256), (5, 1, 801, 0.7, 256), (6, 3, 60, 0.3, 256),
                                                    (7, 8, 3001, 0.9, 40)])
def test_finalize_matches_restatement(seed, chains, rows, phi, K):
    from pyhillfit_amd.diagnostics import finalize
    rng = np.random.default_rng(seed)
    x = ar1(rng, chains, rows, phi) - 40.0
    want = restated(x, K)
    acov, bh, h, M = reduced(x, K)
    rhat, ess, mcse, flag = finalize(acov, bh, h, M)
    assert abs(rhat / want[0] - 1) < 1e-12
    assert bool(flag) == want[3]
    if want[3]:
        assert np.isnan(ess) and np.isnan(mcse)
    else:
        assert abs(ess / want[1] - 1) < 1e-12 and abs(mcse / want[2] - 1) < 1e-12


def test_finalize_undetermined():
    from pyhillfit_amd.diagnostics import finalize
    x = np.full((2, 100), 3.5)                                           # a column that never moved: W = 0
    rhat, ess, mcse, flag = finalize(*reduced(x))
    assert np.isnan(rhat) and np.isnan(ess) and np.isnan(mcse) and not flag
    rng = np.random.default_rng(8)
    x = ar1(rng, 4, 4000, 0.995)                                         # tau far beyond K = 8 lags
    rhat, ess, mcse, flag = finalize(*reduced(x, K=8))
    assert flag and np.isnan(ess) and np.isnan(mcse) and np.isfinite(rhat)
    want = restated(x, K=8)
    assert want[3] and np.isnan(want[1])


def test_finalize_vectorised_over_problems():
    from pyhillfit_amd.diagnostics import finalize
    rng = np.random.default_rng(9)
    xs = [ar1(rng, 3, 500, phi) for phi in (0.1, 0.6, 0.8)]
    parts = [reduced(x, 64) for x in xs]
    acov = np.stack([p[0] for p in parts]).reshape(3, 1, -1)
    bh = np.array([p[1] for p in parts]).reshape(3, 1)
    rhat, ess, _, _ = finalize(acov, bh, 250, 6)
    for i, x in enumerate(xs):
        want = restated(x, 64)
        assert abs(rhat[i, 0] / want[0] - 1) < 1e-12 and abs(ess[i, 0] / want[1] - 1) < 1e-12


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from pyhillfit_amd import _lib
    return _lib.load()


def test_abi_validation_without_gpu(lib):
    fake = C.c_void_p(0x1000)          # never dereferenced: every call below must fail its checks before any launch
    assert lib.phf_diagnostics_workspace_bytes(2, 4, 64, 1000, 256) == 2 * 4 * 64 * (4 * 256 + 6) * 8
    assert lib.phf_diagnostics_workspace_bytes(1, 3, 1, 9, 256) == 3 * (4 * 3 + 6) * 8         # h = 4: L = 3
    assert lib.phf_diagnostics_effective_lags(1001, 256) == 256 and lib.phf_diagnostics_effective_lags(100, 256) == 49
    for args, word in (((0, 4, 64, 1000, 256), b"positive"), ((1, 4, 64, 1000, 0), b"lag limit"), ((1, 4, 64, 1000, -3), b"lag limit"),
                       ((1, 4, 64, 7, 256), b"h = floor")):
        assert lib.phf_diagnostics_workspace_bytes(*args) == 0 and word in lib.phf_last_error()
    big = 1 << 40
    assert lib.phf_diagnostics_init(1, 4, 64, 1000, 0, fake, big, None) == -1 and b"lag limit" in lib.phf_last_error()
    assert lib.phf_diagnostics_init(1, 4, 64, 7, 256, fake, big, None) == -1 and b"h = floor" in lib.phf_last_error()
    assert lib.phf_diagnostics_init(1, 4, 64, 1000, 256, None, big, None) == -1 and b"null" in lib.phf_last_error()
    assert lib.phf_diagnostics_init(1, 4, 64, 1000, 256, fake, 8, None) == -1 and b"workspace smaller" in lib.phf_last_error()
    acc = lib.phf_diagnostics_accumulate
    assert acc(fake, 10, 1, 4, 64, 4, 0, 1000, 0, fake, big, None) == -1 and b"lag limit" in lib.phf_last_error()
    assert acc(fake, 10, 1, 4, 64, 4, 0, 6, 256, fake, big, None) == -1 and b"h = floor" in lib.phf_last_error()
    assert acc(fake, 10, 0, 4, 64, 4, 0, 1000, 256, fake, big, None) == -1 and b"positive" in lib.phf_last_error()
    assert acc(fake, 10, 1, 4, 0, 4, 0, 1000, 256, fake, big, None) == -1 and b"positive" in lib.phf_last_error()
    assert acc(fake, 10, 1, 4, 64, 4, 995, 1000, 256, fake, big, None) == -1 and b"first_row" in lib.phf_last_error()
    assert acc(fake, -1, 1, 4, 64, 4, 0, 1000, 256, fake, big, None) == -1 and b"first_row" in lib.phf_last_error()
    assert acc(fake, 10, 1, 3, 64, 4, 0, 1000, 256, fake, big, None) == -1 and b"row_stride_cols" in lib.phf_last_error()
    assert acc(None, 10, 1, 4, 64, 4, 0, 1000, 256, fake, big, None) == -1 and b"null" in lib.phf_last_error()
    assert acc(fake, 10, 1, 4, 64, 4, 0, 1000, 256, None, big, None) == -1 and b"null" in lib.phf_last_error()
    assert acc(fake, 10, 1, 4, 64, 4, 0, 1000, 256, fake, 8, None) == -1 and b"workspace smaller" in lib.phf_last_error()
    red = lib.phf_diagnostics_reduce
    assert red(1, 4, 64, 1000, 256, fake, big, None, None) == -1 and b"null" in lib.phf_last_error()
    assert red(1, 4, 64, 1000, 256, None, big, fake, None) == -1 and b"null" in lib.phf_last_error()
    assert red(1, 4, 64, 1000, -1, fake, big, fake, None) == -1 and b"lag limit" in lib.phf_last_error()
    assert red(1, 4, 64, 5, 256, fake, big, fake, None) == -1 and b"h = floor" in lib.phf_last_error()
    assert red(1, 4, 64, 1000, 256, fake, 16, fake, None) == -1 and b"workspace smaller" in lib.phf_last_error()


def test_chain_file_reader_drops_hierarchical_burn_in(tmp_path):
    from pyhillfit_amd import chainio
    from pyhillfit_amd.chain_diagnostics import load_rows
    rows = np.arange(40 * 12, dtype=np.float64).reshape(40, 12) / 7.0
    p = tmp_path / "chain.txt"
    chainio.save_hierarchical_chain(str(p), rows)
    got, kind = load_rows(str(p))
    assert kind == "hierarchical text" and np.array_equal(got[:, :, 0], rows[10:])
    q = tmp_path / "x_all_chains.npy"
    arr = np.random.default_rng(0).standard_normal((30, 4, 5))
    np.save(str(q), arr)
    got, kind = load_rows(str(q))
    assert kind == "all chains" and np.array_equal(got, arr)


def test_report_line_takes_groups_of_different_columns():
    from pyhillfit_amd.diagnostics import report_line
    line = report_line(0, ["a + x", "b + y"], [np.array([1.0, 1.002]), np.array([1.0, 1.03, 1.0, 1.0])],
                       [np.array([900., 800.]), np.array([50., np.nan, 70., 80.])])
    assert "1 of 2 with R-hat > 1.01" in line and "1 with an ESS not determined" in line and "b + y (R-hat 1.0300)" in line
