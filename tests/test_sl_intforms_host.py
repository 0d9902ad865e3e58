"""The three-input bit forms the device takes in place of the host's text in phf_normal_u32 and phf_log_ndtr_tab (phf_math.h, "round 10":
the mantissa's re-bias (hi & 0xfffff) | 0x3ff00000 and the normal's sign transfer, one v_bitop3_b32 each), built for the host with the
flags of oracle/Makefile and compared with the twin's expressions as bit patterns.  The shim restates the twin's expressions from the
header text; the forms are the header's own functions.  No GPU.  The argument sets below are shared with tests/test_gpu_sl_intforms.py,
which gives them — the logarithm's too — to the device's functions."""
import ctypes as C
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import REPO

SHIM = r"""
#include <stdint.h>
#include <stddef.h>
#include "phf_model.h"

/* bit 0: re-biased mantissa; bit 1: sign transfer; bit 2: the whole normal */
static int normal_one(uint32_t v) {
  const uint64_t ab = phf_bits((double)((v << 1) | 1u));
  const uint32_t hi = (uint32_t)(ab >> 32);
  const uint64_t mb = (ab & 0x000fffffffffffffull) | 0x3ff0000000000000ull;                  /* the twin's re-biased mantissa */
  const double z = phf_normal_u32(v), zi = phf_normal_u32_int(v);
  /* the twin's result with the OTHER sign, as a polynomial value of either sign may come: the select must give the twin's result back */
  const uint64_t zb = phf_bits(z) ^ 0x8000000000000000ull;
  const uint64_t want = (zb & 0x7fffffffffffffffull) | ((uint64_t)(v & 0x80000000u) << 32);   /* the twin's expression */
  const uint64_t got = ((uint64_t)phf_bit_select_u32((uint32_t)(zb >> 32), v, 0x7fffffffu) << 32) | (uint32_t)zb;
  int bad = 0;
  bad |= (phf_bits(phf_from_words(phf_and_or_u32(hi, 0x000fffffu, 0x3ff00000u), (uint32_t)ab)) != mb) << 0;
  bad |= (want != got || want != phf_bits(z)) << 1;
  bad |= (phf_bits(z) != phf_bits(zi)) << 2;
  return bad;
}

int normal_range(uint64_t first, uint64_t count) {
  int bad = 0;
  for (uint64_t i = 0; i < count; ++i) bad |= normal_one((uint32_t)(first + i));
  return bad;
}

int normal_words(const uint32_t* w, int64_t n) {
  int bad = 0;
  for (int64_t i = 0; i < n; ++i) bad |= normal_one(w[i]);
  return bad;
}

int64_t logphi_diff(const double* y, int64_t n, int64_t* first_bad) {
  int64_t bad = 0;
  for (int64_t i = 0; i < n; ++i) {
    const uint64_t vb = phf_bits(y[i] + 1.0);
    const uint64_t sb = (vb & 0x000fffffffffffffull) | 0x3ff0000000000000ull;                /* the twin's line (sft = this - 1.0) */
    const uint64_t sb2 = phf_bits(phf_from_words(phf_and_or_u32((uint32_t)(vb >> 32), 0x000fffffu, 0x3ff00000u), (uint32_t)vb));
    if (sb != sb2) { if (!bad) *first_bad = i; ++bad; }
  }
  return bad;
}

/* the two identities over arbitrary words */
int64_t identities_diff(const uint32_t* a, const uint32_t* b, const uint32_t* m, int64_t n) {
  int64_t bad = 0;
  for (int64_t i = 0; i < n; ++i)
    bad += phf_and_or_u32(a[i], m[i], b[i]) != ((a[i] & m[i]) | b[i]) || phf_bit_select_u32(a[i], b[i], m[i]) != ((a[i] & m[i]) | (b[i] & ~m[i]));
  return bad;
}

void constants(double* out) { out[0] = PHF_LOGPHI_Y_MAX; out[1] = PHF_LOGPHI_TAB_N; out[2] = PHF_DBL_MIN; out[3] = PHF_INV_SQRT2; }
"""

SQRT_HALF_BITS = 0x3fe6a09e667f3bcd
LOGPHI_Y_MAX = 131071.0


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler for the host build of the model header")
    d = tmp_path_factory.mktemp("sl_intforms")
    src, so = d / "shim.c", d / "libshim.so"
    src.write_text(SHIM)
    # the flags of oracle/Makefile: the host evaluates the operation sequence the kernels do
    subprocess.check_call([cc, "-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-shared",
                           "-I", os.path.join(REPO, "pyhillfit_amd", "csrc"), "-o", str(so), str(src), "-lm"])
    lib = C.CDLL(str(so))
    for f in (lib.logphi_diff, lib.identities_diff):
        f.restype = C.c_int64
    k = np.empty(4)
    lib.constants(k.ctypes.data_as(C.c_void_p))
    assert k[0] == LOGPHI_Y_MAX and k[1] == 136 and k[2] == 2.0 ** -1022
    assert np.array([SQRT_HALF_BITS], dtype=np.uint64).view(np.float64)[0] == k[3]
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- argument sets (also what tests/test_gpu_sl_intforms.py gives the device) ---------------------------------------------------------
def normal_edge_words():
    """every (exponent, top mantissa bit, sign) cell of a = 2 w + 1 at its first and last words +- 2, and the words 0, 1, 0x7fffffff,
    0x80000000, 0xffffffff"""
    w = [0, 1, 0x7fffffff, 0x80000000, 0xffffffff]
    for e in range(32):                                    # a in [2^e, 2^(e+1)); the top mantissa bit splits the binade at 3 * 2^(e-1)
        for a_first in (1 << e, 3 << (e - 1) if e else 1):
            a_last = (3 << (e - 1)) - 1 if (a_first == 1 << e and e) else (2 << e) - 1
            for a in (a_first, a_last):
                for s in (0, 0x80000000):
                    for k in range(-2, 3):
                        w.append((((a | 1) - 1) // 2 + k) % (1 << 31) | s)
    return np.unique(np.array(w, dtype=np.uint64)).astype(np.uint32)


def log_edge_args():
    """sqrt(1/2) and its neighbours in every tenth binade, every power of two and its neighbours, PHF_DBL_MIN, 1e-3, 6 - 1e-3"""
    u = []
    for k in range(-1021, 1024, 10):
        b = SQRT_HALF_BITS + ((k + 1) << 52)
        if 0 < (b >> 52) < 2047:
            u += [b + d for d in range(-2, 3)]
    for k in range(1, 2047):
        u += [(k << 52) + d for d in range(-2, 3)]
    x = np.array(u, dtype=np.uint64).view(np.float64)
    x = np.concatenate([x, [2.0 ** -1022, 1e-3, 6.0 - 1e-3, 1.0, np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0)]])
    return x[np.isfinite(x) & (x >= 2.0 ** -1022)]


def log_random_args(n, seed=101):
    """positive doubles spread over 2^-1000 .. 2^1000 with random mantissas"""
    rng = np.random.default_rng(seed)
    return (rng.integers(23, 2024, n, dtype=np.uint64) << np.uint64(52) | rng.integers(0, 1 << 52, n, dtype=np.uint64)).view(np.float64)


def logphi_y_args():
    """y = -x / sqrt 2 of phf_log_ndtr_tab: a grid over [0, PHF_LOGPHI_Y_MAX] dense in every interval of the table (y + 1 = 2^E m: eight
    intervals per binade, 17 binades), the interval ends and their neighbours, values beyond the table, negative ones, +-0, infinities, NaN"""
    ys = [np.linspace(0.0, 2.0, 4001)]
    for e in range(18):
        for k in range(8):
            lo = 2.0 ** e * (1 + k / 8.0) - 1.0
            hi = 2.0 ** e * (1 + (k + 1) / 8.0) - 1.0
            ys.append(np.linspace(lo, hi, 61))
            for v in (lo, hi):
                ys.append(np.array([np.nextafter(v, -np.inf), v, np.nextafter(v, np.inf)]))
    ys.append(np.array([LOGPHI_Y_MAX, np.nextafter(LOGPHI_Y_MAX, np.inf), np.nextafter(LOGPHI_Y_MAX, 0.0), 131072.0, 2e5, 1e9, 1e300, 1.7e308,
                        0.0, -0.0, 5e-324, 1e-300, -1e-300, -0.5, -1.0, np.nextafter(-1.0, 0.0), -2.0, -1e5, -1e300, np.inf, -np.inf, np.nan]))
    return np.concatenate(ys)


# ---- the tests -------------------------------------------------------------------------------------------------------------------------
def test_normal_draw_every_word(shim):
    """re-biased mantissa, sign transfer and the signed result over all 2^32 words (the index is the twin's own expression)"""
    edge = normal_edge_words()
    assert len(edge) > 500 and shim.normal_words(_p(edge), C.c_int64(len(edge))) == 0
    parts = 256
    step = (1 << 32) // parts
    with ThreadPoolExecutor(max_workers=max(1, min(8, os.cpu_count() or 1))) as ex:        # (ctypes releases the interpreter lock)
        bad = list(ex.map(lambda i: shim.normal_range(C.c_uint64(i * step), C.c_uint64(step)), range(parts)))
    assert not any(bad), [(hex(i * step), b) for i, b in enumerate(bad) if b][:8]


def test_log_phi_shifted_mantissa(shim):
    y = np.ascontiguousarray(logphi_y_args())
    first = C.c_int64(-1)
    assert len(y) > 12000
    assert shim.logphi_diff(_p(y), C.c_int64(len(y)), C.byref(first)) == 0, y[first.value]


def test_the_two_identities_on_arbitrary_words(shim):
    rng = np.random.default_rng(7)
    n = 1 << 20
    a, b, m = (np.ascontiguousarray(rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)) for _ in range(3))
    for arr in (a, b, m):
        arr[:4] = [0, 0xffffffff, 0x80000000, 0x7fffffff]
    assert shim.identities_diff(_p(a), _p(b), _p(m), C.c_int64(n)) == 0
