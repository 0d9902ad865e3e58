"""The histogram grid's scalar rule without a GPU: the C build of pyhillfit_amd/csrc/phf_grid.h (what the quantile and sensitivity
kernels compile), reached through the oracle, against the numpy restatement of tests/test_quantiles_host.py, to the bit."""
import itertools

import numpy as np
import pytest

from test_quantiles_host import base_width, bin_of, holds, t_of

ANCHORS = {"zero": 0.0, "floor": 2.0 ** -30, "minus_floor": -2.0 ** -30, "subnormal": 3e-310, "negative": -123.456, "huge": 1e300}
LEVELS, BINS = (0, 1, 7), (64, 4096)


@pytest.fixture(scope="module")
def co():
    from oracle import c_oracle
    c_oracle.build()
    return c_oracle


def values_for(a):
    """the anchor, anchor +- w0, the edges anchor +- (B/2) w0 2^k with the doubles one ulp inside and outside them, +-inf, NaN, and
    finite values so far out that t overflows to inf: +-1.7e308 and +-1e300 on every grid but the coarsest, and there (anchor 1e300)
    the largest double of the other sign, whose difference from the anchor already overflows"""
    w0 = base_width(a)
    big = np.finfo(np.float64).max
    v = [a, a + w0, a - w0, np.inf, -np.inf, np.nan, 1.7e308, -1.7e308, 1e300, -1e300, big, -big]
    for k, B in itertools.product(LEVELS, BINS):
        for sign in (1.0, -1.0):
            e = a + sign * (B // 2) * w0 * 2.0 ** k
            v += [e, np.nextafter(e, np.inf), np.nextafter(e, -np.inf)]
    return np.array(v, dtype=np.float64)


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("name", sorted(ANCHORS))
def test_scalar_rule_equals_the_restatement(co, name):
    a = ANCHORS[name]
    w0 = base_width(a)
    assert co.grid_w0(a) == w0
    if name in ("zero", "subnormal"):
        assert w0 == 2.0 ** -70                                   # the 2^-30 floor
    x = values_for(a)
    with np.errstate(all="ignore"):
        t_want = t_of(x, a, w0)
    ok = np.isfinite(t_want)
    assert ok[0] and not ok[3:6].any() and (name == "huge" or not ok[6:8].any())
    assert (np.isfinite(x) & ~ok).any() and np.isinf(t_want[11])  # on every grid some finite value's t overflows
    for k, B in itertools.product(LEVELS, BINS):
        t, binned, j = co.grid_bins(a, k, B, x)
        assert np.array_equal(bits(t), bits(t_want))
        assert np.array_equal(binned, ok)
        assert np.array_equal(j[ok], bin_of(t_want[ok], k, B)) and np.all(j[~ok] == -1)
        assert j[0] == B // 2
        # holds: every ordered pair of the finite coordinates (the edges one ulp inside and outside among them)
        ts = np.unique(t_want[ok])
        seen = set()
        for tmin, tmax in itertools.combinations_with_replacement(ts, 2):
            want = bool(holds(tmin, tmax, k, B))
            assert co.grid_holds(tmin, tmax, k, B) == want, (tmin, tmax, k, B)
            seen.add(want)
        assert seen == {True, False}
