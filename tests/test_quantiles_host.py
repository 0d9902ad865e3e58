"""Posterior quantiles without a GPU: a numpy restatement of the histogram grid (bin function, level rule, merge) and of the reduce,
checked against np.quantile(method="inverted_cdf"), segmentation invariance of the counts, the C ABI's argument validation and the
command lines' flags."""
import ctypes as C

import numpy as np
import pytest

PROBS = (0.0, 0.025, 0.05, 0.25, 0.5, 0.75, 0.95, 0.975, 1.0)


# ---- the restatement (pyhillfit_amd/csrc/phf_quantiles.hip) ------------------------------------------------------------------------
def base_width(a):
    """w0 = 2^(floor(log2 max(|a|, 2^-30)) - 40)"""
    m = max(abs(float(a)), 2.0 ** -30)
    return float(np.ldexp(1.0, int(np.frexp(m)[1]) - 1 - 40))


def t_of(x, a, w0):
    return (np.asarray(x, dtype=np.float64) - a) * (1.0 / w0)


def holds(tmin, tmax, k, B):
    return np.floor(np.ldexp(tmin, -k)) >= -(B // 2) and np.floor(np.ldexp(tmax, -k)) < B // 2


def bin_of(t, k, B):
    f = np.floor(np.ldexp(t, -k)) + B // 2
    return np.clip(f, 0, B - 1).astype(np.int64)


class Histogram(object):
    """one slot; feed(values) takes a segment's values in (row, chain) order"""

    def __init__(self, B):
        self.B = B
        self.counts = np.zeros(B, dtype=np.uint64)
        self.anchored, self.a, self.w0, self.k = False, 0.0, 1.0, 0
        self.mn = self.mx = np.nan
        self.nonfinite = 0

    def feed(self, values):
        x = np.asarray(values, dtype=np.float64).ravel()
        if not self.anchored:
            fin = np.flatnonzero(np.isfinite(x))
            if fin.size:
                self.a = float(x[fin[0]])
                self.w0 = base_width(self.a)
                self.anchored, self.mn, self.mx, self.k = True, self.a, self.a, 0
        if not self.anchored:
            self.nonfinite += x.size
            return
        t = t_of(x, self.a, self.w0)
        ok = np.isfinite(t)
        if ok.any():
            self.mn = min(self.mn, float(x[ok].min()))
            self.mx = max(self.mx, float(x[ok].max()))
        k1 = self.k
        tmin, tmax = t_of(self.mn, self.a, self.w0), t_of(self.mx, self.a, self.w0)
        while not holds(tmin, tmax, k1, self.B) and k1 < 1100:
            k1 += 1
        if k1 > self.k:
            D = min(k1 - self.k, int(np.log2(self.B)))
            half = self.B // 2
            j = np.arange(self.B, dtype=np.int64)
            merged = np.zeros(self.B, dtype=np.uint64)
            np.add.at(merged, ((j - half) >> D) + half, self.counts)
            self.counts, self.k = merged, k1
        np.add.at(self.counts, bin_of(t[ok], self.k, self.B), np.uint64(1))
        self.nonfinite += int((~ok).sum())

    @property
    def width(self):
        return float(np.ldexp(self.w0, self.k))

    def quantiles(self, probs):
        """(value, lo, hi, bin) per p, as phf_quantiles_reduce computes them"""
        N = int(self.counts.sum())
        out = np.full((len(probs), 4), np.nan)
        if N == 0:
            return out
        cum = np.cumsum(self.counts.astype(np.int64))
        half = self.B // 2
        for i, p in enumerate(probs):
            r = int(min(max(np.ceil(p * N), 1.0), N))
            j = int(np.searchsorted(cum, r))                      # first bin with cum >= r
            before = int(cum[j] - self.counts[j])
            e = float(j - half) * self.width
            lo, hi = max(self.a + e, self.mn), min(self.a + (e + self.width), self.mx)
            lo = min(lo, hi)
            v = lo + (hi - lo) * ((r - before - 0.5) / float(self.counts[j]))
            out[i] = v, lo, hi, j
        return out


def histogram_of(values, B=16384, cuts=None):
    h = Histogram(B)
    x = np.asarray(values, dtype=np.float64).ravel()
    for seg in np.split(x, cuts or []):
        h.feed(seg)
    return h


def exact(values, probs):
    v = np.asarray(values, dtype=np.float64).ravel()
    v = v[np.isfinite(v)]
    return np.quantile(v, probs, method="inverted_cdf")


def check_brackets(h, values, probs=PROBS, slack=0.0):
    q = h.quantiles(probs)
    want = exact(values, probs)
    tol = slack * np.maximum(np.abs(want), 1.0)
    assert np.all(q[:, 1] <= want + tol) and np.all(want <= q[:, 2] + tol), (q, want)
    assert np.all(q[:, 1] <= q[:, 0]) and np.all(q[:, 0] <= q[:, 2])
    if h.k > 0:                                                   # the resolution bound
        assert h.width <= 4.0 * (h.mx - h.mn) / h.B * (1 + 1e-12)
    return q


CASES = {
    "normal": lambda r: r.normal(5.7, 0.3, 20000),
    "skewed": lambda r: np.exp(r.normal(0.0, 1.5, 20000)),
    "ties": lambda r: np.round(r.normal(3.0, 1.0, 5000), 1),
    "heavy_ties": lambda r: r.integers(0, 3, 4000).astype(float) * 0.5 + 7.0,
    "constant": lambda r: np.full(1000, 10.0),
    "single": lambda r: np.array([-3.25]),
    "near_bound": lambda r: np.minimum(10.0, 10.0 - np.abs(r.normal(0, 1e-3, 8000))),
    "far_outlier": lambda r: np.concatenate([r.normal(0.0, 1.0, 9999), [1e9]]),
    "negative_tiny": lambda r: r.normal(-1e-12, 1e-14, 3000),
    "zero_anchor": lambda r: np.concatenate([[0.0], r.normal(0.0, 1.0, 3000)]),
}


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("B", [64, 16384])
def test_brackets_hold_the_exact_quantile(case, B):
    x = CASES[case](np.random.default_rng(7))
    h = histogram_of(x, B)
    assert int(h.counts.sum()) == x.size and h.nonfinite == 0
    assert h.mn == x.min() and h.mx == x.max()
    q = check_brackets(h, x)
    if case in ("constant", "single"):
        assert np.all(q[:, 0] == x[0]) and np.all(q[:, 1] == x[0]) and np.all(q[:, 2] == x[0])


def test_p0_and_p1_are_min_and_max():
    x = np.random.default_rng(1).normal(size=777)
    q = histogram_of(x).quantiles((0.0, 1.0))
    assert q[0, 1] == x.min() and q[1, 2] == x.max()


def test_non_finite_counted_apart():
    rng = np.random.default_rng(2)
    x = rng.normal(2.0, 1.0, 3000)
    x[[0, 5, 17, 400]] = [np.nan, np.inf, -np.inf, np.nan]
    h = histogram_of(x, 4096, cuts=[3, 1000])
    assert h.nonfinite == 4 and int(h.counts.sum()) == 2996
    assert h.a == x[1]                                            # the first finite value anchors the grid
    check_brackets(h, x)
    h = histogram_of(np.full(10, np.nan), 64)
    assert h.nonfinite == 10 and int(h.counts.sum()) == 0 and np.all(np.isnan(h.quantiles(PROBS)))


def test_bin_function_is_the_division():
    """(x - a) * (1/w0) is the same double as (x - a) / w0, and the bins are monotone in x"""
    rng = np.random.default_rng(3)
    for a in (5.7, -1e-9, 0.0, 1234.5, 1e-40):
        w0 = base_width(a)
        x = a + rng.normal(0, max(abs(a), 1e-6), 10000)
        assert np.array_equal(t_of(x, a, w0), (x - a) / w0)
        for k in (0, 3, 17):
            j = bin_of(t_of(np.sort(x), a, w0), k, 1 << 20)
            assert np.all(np.diff(j) >= 0)
    assert base_width(5.7) == 2.0 ** (2 - 40) and base_width(0.0) == 2.0 ** (-30 - 40) and base_width(-8.0) == 2.0 ** (3 - 40)


@pytest.mark.parametrize("case", ["normal", "skewed", "heavy_ties", "far_outlier"])
def test_segmentation_invariance(case):
    x = CASES[case](np.random.default_rng(11))
    ref = histogram_of(x, 1024)
    for cuts in ([1], [7, 8, 9, 5000], list(range(97, x.size, 997)), [x.size // 2]):
        h = histogram_of(x, 1024, cuts=cuts)
        assert np.array_equal(h.counts, ref.counts) and h.k == ref.k and (h.mn, h.mx, h.a) == (ref.mn, ref.mx, ref.a)
    # ... and equal to binning everything at the final level at once
    direct = np.zeros(1024, dtype=np.uint64)
    np.add.at(direct, bin_of(t_of(x, ref.a, ref.w0), ref.k, 1024), np.uint64(1))
    assert np.array_equal(direct, ref.counts)


def test_growing_range_merges():
    """a range that grows segment by segment raises the level several times"""
    x = np.concatenate([np.random.default_rng(4).normal(1.0, s, 500) for s in (1e-6, 1e-3, 1.0, 1e3)])
    h = histogram_of(x, 256, cuts=[500, 1000, 1500])
    assert h.k > 20
    check_brackets(h, x)


# ---- the C ABI without a GPU ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from pyhillfit_amd import _lib
    return _lib.load()


def test_abi_validation(lib):
    S = 3 * (4 + 5)
    assert lib.phf_quantiles_workspace_bytes(3, 4, 5, 1024) == S * 1024 * 8 + S * 8 * 8 + S * 8
    for bad in [(3, 4, 0, 1000), (3, 4, 0, 32), (3, 4, 0, 65536), (0, 4, 0, 1024), (3, 0, 0, 1024), (3, -1, 2, 1024)]:
        assert lib.phf_quantiles_workspace_bytes(*bad) == 0, bad
        assert lib.phf_last_error()
    assert lib.phf_quantiles_workspace_bytes(3, 4, 0, 1000) == 0 and b"power of two" in lib.phf_last_error()
    fake = C.c_void_p(8)
    big = C.c_size_t(1 << 40)
    assert lib.phf_quantiles_init(3, 4, 0, 1024, None, big, None) == -1 and b"null" in lib.phf_last_error()
    assert lib.phf_quantiles_init(3, 4, 0, 1024, fake, C.c_size_t(16), None) == -1 and b"smaller" in lib.phf_last_error()

    def acc(n=10, Q=3, stride=4, chains=64, cols=4, G=0, B=1024, first=0, total=100, ws=fake, wsb=big, rows=fake):
        return lib.phf_quantiles_accumulate(rows, n, Q, stride, chains, cols, G, B, first, total, ws, wsb, None)
    assert acc(B=1000) == -1 and b"power of two" in lib.phf_last_error()
    assert acc(stride=3) == -1 and b"row_stride_cols" in lib.phf_last_error()
    assert acc(first=95) == -1 and b"total_rows" in lib.phf_last_error()
    assert acc(n=101) == -1 and b"total_rows" in lib.phf_last_error()
    assert acc(n=1 << 20, chains=4096, total=1 << 21) == -1 and b"2^31" in lib.phf_last_error()
    assert acc(wsb=C.c_size_t(8)) == -1 and b"smaller" in lib.phf_last_error()
    assert acc(ws=None) == -1 and b"null" in lib.phf_last_error()
    assert acc(rows=None) == -1 and b"null rows" in lib.phf_last_error()
    assert acc(n=0, first=100) == 0                                # nothing to do: no launch

    def curves(model=2, stride=4, G=8, doses=fake, n=10, first=0):
        return lib.phf_quantiles_accumulate_curves(fake, n, 3, stride, 64, model, doses, 4, G, 1024, first, 100, fake, big, None)
    assert curves(model=3) == -1 and b"model" in lib.phf_last_error()
    assert curves(G=0) == -1 and b"curve points" in lib.phf_last_error()
    assert curves(doses=None) == -1 and b"ln_doses" in lib.phf_last_error()
    assert curves(model=2, stride=1) == -1 and b"row_stride_cols" in lib.phf_last_error()
    assert curves(n=200) == -1 and b"total_rows" in lib.phf_last_error()

    probs = (C.c_double * 3)(0.1, 0.5, 0.9)
    out = fake
    assert lib.phf_quantiles_reduce(3, 4, 0, 1024, probs, 0, fake, big, out, None) == -1
    assert lib.phf_quantiles_reduce(3, 4, 0, 1024, probs, 65, fake, big, out, None) == -1
    assert lib.phf_quantiles_reduce(3, 4, 0, 1024, (C.c_double * 1)(1.5), 1, fake, big, out, None) == -1 and b"[0, 1]" in lib.phf_last_error()
    assert lib.phf_quantiles_reduce(3, 4, 0, 1024, probs, 3, fake, big, None, None) == -1 and b"null" in lib.phf_last_error()
    assert lib.phf_quantiles_reduce(3, 4, 0, 1000, probs, 3, fake, big, out, None) == -1 and b"power of two" in lib.phf_last_error()


# ---- the command lines' flags ------------------------------------------------------------------------------------------------------
def test_parser_flags():
    from pyhillfit_amd import PyHillFit
    p = PyHillFit.build_parser()
    a = p.parse_args(["--data-file", "x.csv", "-m", "2"])
    assert not a.quantiles and a.quantile_bins == 16384 and a.curve_bands == 0
    assert tuple(a.quantile_probs) == (0.025, 0.05, 0.25, 0.5, 0.75, 0.95, 0.975)
    a = p.parse_args(["--data-file", "x.csv", "-m", "2", "--quantiles", "--quantile-probs", "0.1,0.5,0.9", "--quantile-bins", "4096",
                      "--curve-bands", "32"])
    assert a.quantiles and a.quantile_probs == (0.1, 0.5, 0.9) and a.quantile_bins == 4096 and a.curve_bands == 32
    for bad in (["--quantile-bins", "1000"], ["--quantile-bins", "32"], ["--quantile-probs", "0.5,1.5"], ["--quantile-probs", ""]):
        with pytest.raises(SystemExit):
            p.parse_args(["--data-file", "x.csv", "-m", "2"] + bad)


@pytest.mark.parametrize("extra", [["--hierarchical", "--quantiles", "--curve-bands", "16"], ["--curve-bands", "16"],
                                   ["--quantiles", "--curve-bands", "-1"]])
def test_curve_band_refusals(extra, capsys):
    from pyhillfit_amd import PyHillFit
    with pytest.raises(SystemExit) as e:
        PyHillFit.main(["--data-file", "does-not-exist.csv", "-m", "2"] + extra)
    assert e.value.code == 2
    assert "--curve-bands" in capsys.readouterr().err


def test_json_record_and_intervals():
    from pyhillfit_amd import quantiles as qn
    P = qn.DEFAULT_PROBS
    v = np.arange(2 * 3 * len(P), dtype=float).reshape(2, 3, len(P))
    res = {"value": v, "lo": v - 0.5, "hi": v + 0.5, "min": np.zeros((2, 3)), "max": np.full((2, 3), 99.0),
           "draws": np.full((2, 3), 1000.0), "non_finite": np.zeros((2, 3)), "bin_width": np.full((2, 3), 0.01),
           "probs": np.array(P), "columns": 2, "curve_points": 1}
    rec = qn.json_record(res, 1, ["pIC50", "sigma"], 16384)
    assert set(rec) == {"pIC50", "sigma", "probs", "bins", "method"}
    c = rec["sigma"]
    assert c["value"] == list(v[1, 1]) and c["draws"] == 1000
    assert c["ci95"] == [v[1, 1, 0], v[1, 1, 6]] and c["ci90"] == [v[1, 1, 1], v[1, 1, 5]]
    assert c["ci95_bracket"] == [v[1, 1, 0] - 0.5, v[1, 1, 6] + 0.5]
    band = qn.curve_band_record(res, 0, [0.5])
    assert band["doses"] == [0.5] and band["value"] == [list(v[0, 2])] and len(band["ci90"]) == 1
    assert qn.report_line(0, ["a + b"], [(np.array([0.01]), np.array([0.0]), np.array([1.0]), np.array([3]))]).startswith("quantiles [rank 0]: 1 pairs")


def test_hill_curve_and_doses():
    from pyhillfit_amd import quantiles as qn
    d = qn.curve_doses([0.1, 1.0, 30.0, 0.0], 5)
    assert d[0] == pytest.approx(0.01) and d[-1] == pytest.approx(300.0) and np.all(np.diff(np.log(d)) > 0)
    # at the IC50 the curve is 50 %; model 1 ignores Hill
    assert qn.hill_curve(2, np.log(10.0 ** (6 - 6.0)), 6.0, 1.7) == pytest.approx(50.0)
    assert qn.hill_curve(1, np.log(3.0), 5.5, 9.0) == qn.hill_curve(1, np.log(3.0), 5.5, 1.0)
