"""phf_sl_log_target_shared (censored entries take the Hill denominator of an uncensored entry at the same ln_conc bits) against
phf_sl_log_target, both built for the host exactly as the twin in oracle/ is (gcc -ffp-contract=off): identical lik, prior and
untempered log-likelihood bits, over every Crumb pair and over synthetic pairs that cover every share mask.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO

SHIM = r"""
#include <stdint.h>
#include <stddef.h>
#include "phf_model.h"

/* out[3 i + 0..2] = lik, prior, ll1 of theta row i (d doubles per row) */
void plain_batch(int model, const double* lc, const double* y, const double* w, int n_other, int n_cens, double nop, double ssw,
                 double pib, double temp, const double* th, int d, int64_t m, double* out) {
  for (int64_t i = 0; i < m; ++i)
    phf_sl_log_target(model, lc, y, w, n_other, n_cens, nop, ssw, pib, temp, th + d * i, phf_k_exp, phf_k_log,
                      out + 3 * i, out + 3 * i + 1, out + 3 * i + 2);
}

void shared_batch(int model, const double* lc, const double* y, const double* w, int n_other, int n_cens, double nop, double ssw,
                  double pib, double temp, const double* th, int d, int64_t m, unsigned mask, const int* den_off, double* out) {
  double slots[64];
  for (int64_t i = 0; i < m; ++i) {
    for (int k = 0; k < 64; ++k) slots[k] = -12345.0;     /* nothing left over from the previous row */
    phf_sl_log_target_shared(model, lc, y, w, n_other, n_cens, nop, ssw, pib, temp, th + d * i, phf_k_exp, phf_k_log,
                             mask, den_off, slots, 1, out + 3 * i, out + 3 * i + 1, out + 3 * i + 2);
  }
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler for the host build of the model header")
    d = tmp_path_factory.mktemp("sl_shared")
    src, so = d / "shim.c", d / "libshim.so"
    src.write_text(SHIM)
    # the flags of oracle/Makefile: the host evaluates the operation sequence the kernels do
    subprocess.check_call([cc, "-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-shared",
                           "-I", os.path.join(REPO, "pyhillfit_amd", "csrc"), "-o", str(so), str(src), "-lm"])
    lib = C.CDLL(str(so))
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def share_map(lc, n_other, n_cens):
    """censored entry m -> the first uncensored entry with the same ln_conc bits, or -1 (what the kernel derives when it stages)"""
    bits = np.ascontiguousarray(lc, dtype=np.float64).view(np.uint64)
    src = []
    for m in range(n_cens):
        hit = [j for j in range(n_other) if bits[j] == bits[n_other + m]]
        src.append(hit[0] if hit else -1)
    return src


def _run(lib, model, lc, y, w, n_other, n_cens, extra, theta, mask, src):
    lc, y, w = (np.ascontiguousarray(a, dtype=np.float64) for a in (lc, y, w))
    th = np.ascontiguousarray(theta, dtype=np.float64)
    m, d = th.shape
    nop, ssw, pib, temp = (float(v) for v in extra)
    a = np.empty((m, 3)); b = np.empty((m, 3))
    args = (C.c_int(model), _p(lc), _p(y), _p(w), C.c_int(n_other), C.c_int(n_cens), C.c_double(nop), C.c_double(ssw),
            C.c_double(pib), C.c_double(temp), _p(th), C.c_int(d), C.c_int64(m))
    lib.plain_batch(*args, _p(a))
    off = np.array([max(s, 0) for s in src] + [0] * (8 - len(src)), dtype=np.int32)
    lib.shared_batch(*args, C.c_uint(mask), _p(off), _p(b))
    return a, b


def _thetas(model, rng, n):
    """typical draws plus the edges: sigma at / below its floor, Hill < 0 and > 10, pIC50 < -3 and >> 20 (the -746 exp clamp)"""
    pic50 = np.concatenate([rng.uniform(2.0, 9.0, n), [-3.0, -3.5, -40.0, 25.0, 80.0, 400.0, 1e4, 6.0, 6.0, 6.0, 6.0, 6.0, 6.0]])
    hill = np.concatenate([rng.uniform(0.2, 3.0, n), [1.0, 1.0, 1.0, 1.0, 4.0, 0.5, 1.0, -0.5, 10.5, 0.0, 10.0, 1.0, 1.0]])
    sigma = np.concatenate([rng.uniform(0.5, 20.0, n), [5.0, 5.0, 5.0, 5.0, 5.0, 5.0, 5.0, 5.0, 5.0, 5.0, 1e-3, 9e-4, 1e-3 + 1e-12]])
    k = len(pic50)
    wild = rng.integers(0, k, k // 10)                                     # some rows far out in every coordinate at once
    pic50[wild] = rng.uniform(-60.0, 700.0, len(wild))
    hill[wild] = rng.uniform(-5.0, 40.0, len(wild))
    return np.column_stack([pic50, sigma] if model == 1 else [pic50, hill, sigma])


@pytest.fixture(scope="module")
def crumb():
    from pyhillfit_amd import doseresponse as dr
    dr.setup(os.path.join(REPO, "data", "crumb_dataset.json"))
    return dr.pack_single_level([(d, c) for d in dr.drugs for c in dr.channels])


def test_every_crumb_pair_bit_identical(shim, crumb):
    rng = np.random.default_rng(7)
    shared_entries = 0
    for p in range(crumb.num_pairs):
        ko, nz, nh = (int(v) for v in crumb.counts[p][:3])
        kc = nz + nh
        n = ko + kc
        lc, y, w = crumb.ln_conc[p, :n], crumb.response[p, :n], crumb.weight[p, :n]
        src = share_map(lc, ko, kc)
        mask = sum(1 << m for m, s in enumerate(src) if s >= 0)
        shared_entries += bin(mask).count("1")
        for model in (1, 2):
            for temp in (1.0, 0.3):
                extra = (crumb.extra[p, 0], crumb.extra[p, 1], crumb.pi_bit[p], temp)
                a, b = _run(shim, model, lc, y, w, ko, kc, extra, _thetas(model, rng, 10000 if temp == 1.0 else 500), mask, src)
                assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (p, model, temp)
    assert crumb.num_pairs == 210 and shared_entries == 310


def _zero_counts(ko, kc, mask):
    """numbers of y == 0 entries with which mask can be built: one class never repeats a dose (entries merge per class), so each
    class shares at most ko entries"""
    return [nz for nz in range(kc + 1) if bin(mask & ((1 << nz) - 1)).count("1") <= ko and bin(mask >> nz).count("1") <= ko]


def _synthetic(ko, kc, mask, rng, dose0):
    """concentrations and responses whose packing has ko uncensored and kc censored entries (zeros first), censored entry m at the
    dose of a random uncensored entry when bit m of mask is set and at a dose of its own otherwise; dose0: entry 0 at dose 0"""
    doses = 10.0 ** np.linspace(-3, 3, 16)
    if dose0:
        doses[0] = 0.0
    unc = [doses[1 + i] for i in rng.permutation(7)[:ko]]
    if dose0 and ko:
        unc[0] = 0.0
    concs, y = [], []
    for k, dc in enumerate(unc):
        for _ in range(int(rng.integers(1, 3))):
            concs.append(dc); y.append(float(np.clip(12.0 * (k + 1) + rng.normal(0, 4), 1.0, 99.0)))
    options = _zero_counts(ko, kc, mask)
    nz = options[int(rng.integers(0, len(options)))]
    own = iter(doses[8:] if not dose0 or ko else doses[[0] + list(range(9, 16))])
    cens = []
    for m in range(kc):
        cls = 0.0 if m < nz else 100.0
        if (mask >> m) & 1:
            # a y == 0 and a y == 100 entry may share one dose (one class never repeats a dose: entries merge per class)
            used = [dc for dc, c in cens if c == cls]
            free = [dc for dc in unc if dc not in used]
            cens.append((free[int(rng.integers(0, len(free)))], cls))
        else:
            cens.append((next(own), cls))
    for dc, cls in cens:
        for _ in range(int(rng.integers(1, 3))):
            concs.append(dc); y.append(cls)
    return np.array(concs), np.array(y)


def synthetic_pairs(seed=3):
    """every share mask of every shape ko <= 5 uncensored x kc <= 4 censored, with and without dose-0 entries"""
    rng = np.random.default_rng(seed)
    out = []
    for ko in range(6):
        for kc in range(5):
            if ko + kc == 0:
                continue
            for mask in range(1 << kc if ko else 1):
                if not _zero_counts(ko, kc, mask):
                    continue                                     # e.g. one uncensored dose: at most one zero and one hundred on it
                for dose0 in (False, True):
                    concs, y = _synthetic(ko, kc, mask, rng, dose0)
                    out.append(((ko, kc, mask, dose0), concs, y))
    return out


def test_synthetic_pairs_cover_every_share_mask(shim):
    from pyhillfit_amd.doseresponse import PackedPoints
    cases = synthetic_pairs()
    packed = PackedPoints([(c, y) for _, c, y in cases])
    rng = np.random.default_rng(5)
    seen = set()
    for p, ((ko, kc, mask, dose0), _, _) in enumerate(cases):
        assert (int(packed.counts[p][0]), int(packed.counts[p][1] + packed.counts[p][2])) == (ko, kc)
        n = ko + kc
        lc, y, w = packed.ln_conc[p, :n], packed.response[p, :n], packed.weight[p, :n]
        src = share_map(lc, ko, kc)
        got = sum(1 << m for m, s in enumerate(src) if s >= 0)
        assert got == mask, (ko, kc, mask, dose0, src)
        if dose0:
            assert np.isneginf(lc).any()
        seen.add((ko, kc, mask))
        th = {model: _thetas(model, rng, 300) for model in (1, 2)}
        # the kernels may share fewer entries than the map allows (a shape's bodies offer a few masks): every sub-mask
        sub = mask
        while True:
            for model in (1, 2):
                extra = (packed.extra[p, 0], packed.extra[p, 1], packed.pi_bit[p], 1.0)
                a, b = _run(shim, model, lc, y, w, ko, kc, extra, th[model], sub, src)
                assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (ko, kc, mask, sub, dose0, model)
            if sub == 0:
                break
            sub = (sub - 1) & mask
    assert all((ko, kc, m) in seen for ko in range(1, 6) for kc in range(5) for m in range(1 << kc) if _zero_counts(ko, kc, m))
    assert len(seen) >= 150
