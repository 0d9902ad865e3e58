"""phf_sl_log_target_sampler (the steady iteration's target: no -inf selects, `outside` returned as a predicate, the Hill
exponentials' lower clamp optional) against phf_sl_log_target_shared, both built for the host exactly as the twin in oracle/ is: inside the prior's
support the same lik, prior and untempered log-likelihood bits; `outside` true exactly where the reference prior is -inf, where the
reference's lik + prior is -inf or NaN (what makes both accept tests reject); over every Crumb pair and synthetic pairs with every share
mask, models 1 and 2, temperatures 1, 0.5 and 0.  No GPU."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO
from test_sl_shared_denominators import _p, _thetas, share_map, synthetic_pairs

SHIM = r"""
#include <stdint.h>
#include <stddef.h>
#include "phf_model.h"

/* out[3 i + 0..2] = lik, prior, ll1 of theta row i (d doubles per row) */
void shared_batch(int model, const double* lc, const double* y, const double* w, int n_other, int n_cens, double nop, double ssw,
                  double pib, double temp, const double* th, int d, int64_t m, unsigned mask, const int* den_off, double* out) {
  double slots[64];
  for (int64_t i = 0; i < m; ++i) {
    for (int k = 0; k < 64; ++k) slots[k] = -12345.0;
    phf_sl_log_target_shared(model, lc, y, w, n_other, n_cens, nop, ssw, pib, temp, th + d * i, phf_k_exp, phf_k_log,
                             mask, den_off, slots, 1, out + 3 * i, out + 3 * i + 1, out + 3 * i + 2);
  }
}

/* out[4 i + 0..3] = lik, prior, ll1, lt; outside[i] = the returned predicate */
void sampler_batch(int model, const double* lc, const double* y, const double* w, int n_other, int n_cens, double nop, double ssw,
                   double pib, double temp, int lower_clamp, const double* th, int d, int64_t m, unsigned mask, const int* den_off,
                   double* out, int* outside) {
  double slots[64];
  for (int64_t i = 0; i < m; ++i) {
    for (int k = 0; k < 64; ++k) slots[k] = -12345.0;
    outside[i] = phf_sl_log_target_sampler(model, lc, y, w, n_other, n_cens, nop, ssw, pib, temp, lower_clamp, th + d * i, phf_k_exp,
                                           phf_k_log, mask, den_off, slots, 1, out + 4 * i, out + 4 * i + 1, out + 4 * i + 2,
                                           out + 4 * i + 3);
  }
}

void constants(double* out) {
  out[0] = PHF_SIGMA_FLOOR; out[1] = PHF_SIGMA_LOC; out[2] = PHF_PIC50_LOWER; out[3] = PHF_HILL_UPPER; out[4] = PHF_LN10;
  out[5] = PHF_HILL_ARG_CAP; out[6] = PHF_LN_CONC_NOCLAMP;
}
"""

TEMPS = (1.0, 0.5, 0.0)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler for the host build of the model header")
    d = tmp_path_factory.mktemp("sl_lean")
    src, so = d / "shim.c", d / "libshim.so"
    src.write_text(SHIM)
    # the flags of oracle/Makefile: the host evaluates the operation sequence the kernels do
    subprocess.check_call([cc, "-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-shared",
                           "-I", os.path.join(REPO, "pyhillfit_amd", "csrc"), "-o", str(so), str(src), "-lm"])
    return C.CDLL(str(so))


@pytest.fixture(scope="module")
def crumb():
    from pyhillfit_amd import doseresponse as dr
    dr.setup(os.path.join(REPO, "data", "crumb_dataset.json"))
    return dr.pack_single_level([(d, c) for d in dr.drugs for c in dr.channels])


def _inside(model, th):
    """the prior's support, written out from the reference's bounds (a NaN coordinate fails no bound: the reference's tests are
    `x < lower`, `x <= loc`, `x > upper`)"""
    pic50, sigma = th[:, 0], th[:, -1]
    out = (pic50 < -3.0) | (sigma <= 1e-3)
    if model == 2:
        out |= (th[:, 1] < 0.0) | (th[:, 1] > 10.0)
    return ~out


def _both(lib, model, lc, y, w, n_other, n_cens, extra, temp, theta, mask, src):
    lc, y, w = (np.ascontiguousarray(a, dtype=np.float64) for a in (lc, y, w))
    th = np.ascontiguousarray(theta, dtype=np.float64)
    m, d = th.shape
    nop, ssw, pib = (float(v) for v in extra)
    ref = np.empty((m, 3)); got = np.empty((m, 4)); outside = np.empty(m, dtype=np.int32)
    off = np.array([max(s, 0) for s in src] + [0] * (8 - len(src)), dtype=np.int32)
    head = (C.c_int(model), _p(lc), _p(y), _p(w), C.c_int(n_other), C.c_int(n_cens), C.c_double(nop), C.c_double(ssw), C.c_double(pib),
            C.c_double(temp))
    tail = (_p(th), C.c_int(d), C.c_int64(m), C.c_uint(mask), _p(off))
    lib.shared_batch(*head, *tail, _p(ref))
    # the lower clamp of the Hill exponentials is dropped wherever the kernels may drop it: every ln_conc >= PHF_LN_CONC_NOCLAMP
    lower_clamp = int(not (lc >= -50.0).all())
    lib.sampler_batch(*head, C.c_int(lower_clamp), *tail, _p(got), _p(outside))
    if not lower_clamp:                     # and with it kept: the same bits everywhere the result is read (inside the support)
        kept = np.empty((m, 4)); outside_kept = np.empty(m, dtype=np.int32)
        lib.sampler_batch(*head, C.c_int(1), *tail, _p(kept), _p(outside_kept))
        ins = outside == 0
        assert np.array_equal(outside, outside_kept)
        assert np.array_equal(np.ascontiguousarray(kept[ins]).view(np.uint64), np.ascontiguousarray(got[ins]).view(np.uint64))
    return ref, got, outside.astype(bool)


def _compare(ref, got, outside, model, th, temp, where):
    inside = _inside(model, th)
    assert np.isfinite(th).all()
    assert np.array_equal(outside, ~inside), where                                        # the predicate is the support's complement ...
    assert np.array_equal(outside, np.isneginf(ref[:, 1])), where                         # ... which is where the reference prior is -inf
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)
    assert np.array_equal(bits(got[inside, :3]), bits(ref[inside])), where                # inside: the same lik, prior, ll1 bits
    lt_ref = ref[:, 0] + ref[:, 1]
    assert np.array_equal(bits(got[inside, 3]), bits(lt_ref[inside])), where              # and lt = lik + prior
    assert (np.isneginf(lt_ref[outside]) | np.isnan(lt_ref[outside])).all(), where        # outside: the reference can only be rejected
    assert (np.isneginf(ref[ref[:, 2] == -np.inf, 1])).all(), where                       # the likelihood's own -inf lies within `outside`
    if temp == 0.0:
        assert (got[inside, 0] == 0.0).all() and not np.signbit(got[inside, 0]).any(), where


def test_every_crumb_pair(shim, crumb):
    rng = np.random.default_rng(11)
    for p in range(crumb.num_pairs):
        ko, nz, nh = (int(v) for v in crumb.counts[p][:3])
        kc, n = nz + nh, ko + nz + nh
        lc, y, w = crumb.ln_conc[p, :n], crumb.response[p, :n], crumb.weight[p, :n]
        src = share_map(lc, ko, kc)
        mask = sum(1 << m for m, s in enumerate(src) if s >= 0)
        extra = (crumb.extra[p, 0], crumb.extra[p, 1], crumb.pi_bit[p])
        for model in (1, 2):
            th = _thetas(model, rng, 1500)
            for temp in TEMPS:
                ref, got, outside = _both(shim, model, lc, y, w, ko, kc, extra, temp, th, mask, src)
                _compare(ref, got, outside, model, th, temp, (p, model, temp))
    assert crumb.num_pairs == 210


def test_synthetic_pairs_with_every_share_mask(shim):
    from pyhillfit_amd.doseresponse import PackedPoints
    cases = synthetic_pairs()
    packed = PackedPoints([(c, y) for _, c, y in cases])
    rng = np.random.default_rng(13)
    th = {model: _thetas(model, rng, 200) for model in (1, 2)}
    seen = set()
    for p, ((ko, kc, mask, dose0), _, _) in enumerate(cases):
        n = ko + kc
        lc, y, w = packed.ln_conc[p, :n], packed.response[p, :n], packed.weight[p, :n]
        src = share_map(lc, ko, kc)
        assert sum(1 << m for m, s in enumerate(src) if s >= 0) == mask
        seen.add((ko, kc, mask))
        extra = (packed.extra[p, 0], packed.extra[p, 1], packed.pi_bit[p])
        for model in (1, 2):
            for temp in TEMPS:
                ref, got, outside = _both(shim, model, lc, y, w, ko, kc, extra, temp, th[model], mask, src)
                _compare(ref, got, outside, model, th[model], temp, (ko, kc, mask, dose0, model, temp))
    assert len(seen) >= 150


def _straddle(x):
    """x itself, its two neighbours, and points a little and far to either side"""
    return [x, np.nextafter(x, -np.inf), np.nextafter(x, np.inf), x - 1e-9, x + 1e-9, x - 1.0, x + 1.0]


def test_outside_is_exactly_where_the_reference_prior_is_minus_infinity(shim, crumb):
    """a grid across each of the four bounds, the values exactly on them (sigma = 1e-3 is outside; Hill = 0, Hill = 10 and pIC50 = -3 are
    inside), infinities and NaN in every coordinate"""
    special = [np.nan, np.inf, -np.inf]
    pic50s = _straddle(-3.0) + [6.0] + special
    hills = _straddle(0.0) + _straddle(10.0) + [1.0] + special
    sigmas = _straddle(1e-3) + [0.0, -1.0, 5.0] + special
    for p in (0, 57, 209):
        ko, nz, nh = (int(v) for v in crumb.counts[p][:3])
        kc, n = nz + nh, ko + nz + nh
        lc, y, w = crumb.ln_conc[p, :n], crumb.response[p, :n], crumb.weight[p, :n]
        src = share_map(lc, ko, kc)
        mask = sum(1 << m for m, s in enumerate(src) if s >= 0)
        extra = (crumb.extra[p, 0], crumb.extra[p, 1], crumb.pi_bit[p])
        for model in (1, 2):
            grid = [[a, s] for a in pic50s for s in sigmas] if model == 1 else [[a, h, s] for a in pic50s for h in hills for s in sigmas]
            th = np.array(grid)
            on_bounds = np.array([[-3.0, 5.0], [6.0, 1e-3]] if model == 1 else [[-3.0, 0.0, 5.0], [-3.0, 10.0, 5.0], [6.0, 1.0, 1e-3]])
            assert _inside(model, on_bounds).tolist() == [True] * (len(on_bounds) - 1) + [False]
            for temp in TEMPS:
                ref, got, outside = _both(shim, model, lc, y, w, ko, kc, extra, temp, th, mask, src)
                where = (p, model, temp)
                no_inf = ~np.isinf(th).any(axis=1)       # (an infinite pIC50 or sigma makes the prior -inf or NaN by itself)
                assert np.array_equal(outside[no_inf], np.isneginf(ref[no_inf, 1])), where
                assert np.array_equal(outside, ~_inside(model, th)), where
                lt_ref = ref[:, 0] + ref[:, 1]
                assert (np.isneginf(lt_ref[outside]) | np.isnan(lt_ref[outside])).all(), where
                # inside the bounds, NaN and infinite coordinates included: the same bits (NaN payloads included)
                ins = ~outside
                assert np.array_equal(np.ascontiguousarray(got[ins, :3]).view(np.uint64),
                                      np.ascontiguousarray(ref[ins]).view(np.uint64)), where


def test_bounds_from_the_constants(shim, crumb):
    """sigma's floor is the prior's location (so the likelihood's -inf lies within `outside`); and inside the support no Hill exponential
    argument of a pair with every ln_conc >= PHF_LN_CONC_NOCLAMP reaches the lower clamp -746: hill <= PHF_HILL_UPPER, ln_ic50 = ln 10
    (6 - pic50) <= ln 10 (6 - PHF_PIC50_LOWER), so a = hill (ln_conc - ln_ic50) >= PHF_HILL_UPPER (PHF_LN_CONC_NOCLAMP - 9 ln 10)"""
    k = np.empty(7)
    shim.constants(_p(k))
    floor, loc, pic50_lower, hill_upper, ln10, cap, lc_min = k
    assert floor == loc == 1e-3 and pic50_lower == -3.0 and hill_upper == 10.0 and ln10 == math.log(10.0) and lc_min == -50.0
    ln_ic50_max = ln10 * (6.0 - pic50_lower)
    assert hill_upper >= 1.0                                            # model 1 (Hill = 1) is covered by the same bound
    assert hill_upper * (lc_min - ln_ic50_max) > -746.0 + 30.0          # -707.2: thirty units of margin against a few roundings
    n = crumb.counts[:, :3].sum(axis=1)
    smallest = min(crumb.ln_conc[p, :n[p]].min() for p in range(crumb.num_pairs))
    assert smallest >= lc_min and abs(smallest - math.log(1e-4)) < 1e-9  # every Crumb pair keeps its straight-line body
