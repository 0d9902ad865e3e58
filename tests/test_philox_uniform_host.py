"""phf_philox_mh_t_uniform (phf_philox.h, "round 11": the block of counter (chain, problem, t, 0) with round 1's wave-uniform word and round
2's product spelled for the scalar unit, which the steady bodies of the two-wavefront build draw from) against phf_philox_mh, both built
for the host with the flags of oracle/Makefile, once per round count the header is built with (7: what the samplers draw with; 10).  All
four words, as bit patterns.  No GPU."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO

SHIM = r"""
#include <stdint.h>
#include <stddef.h>
#include "phf_philox.h"

int rounds(void) { return PHF_PHILOX_ROUNDS; }

/* a[5 i + 0..4] = chain, problem, t, seed low word, seed high word; the helper's own words go to out[4 i + 0..3]; returns how many tuples
 * differ from phf_philox_mh in any word */
int64_t uniform_diff(const uint32_t* a, int64_t n, uint32_t* out) {
  int64_t bad = 0;
  for (int64_t i = 0; i < n; ++i) {
    const uint32_t* x = a + 5 * i;
    const phf_u32x4 want = phf_philox_mh(x[0], x[1], x[2], 0u, x[3], x[4]);
    const phf_u32x4 got = phf_philox_mh_t_uniform(x[0], x[1], x[2], x[3], x[4], x[3], x[4] + 0xBB67AE85u);
    int d = 0;
    for (int k = 0; k < 4; ++k) { out[4 * i + k] = got.w[k]; d |= got.w[k] != want.w[k]; }
    bad += d;
  }
  return bad;
}
"""

# Random123 kat_vectors (philox4x32 7 and philox4x32 10): counter words 0..3 and key words 0, 1; answers of the all-zero line, whose fourth
# counter word is the 0 the samplers use
KAT_COUNTER_KEY = [[0, 0, 0, 0, 0, 0], [0xffffffff] * 6, [0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344, 0xa4093822, 0x299f31d0]]
KAT_ZERO_ANSWER = {7: [0x5f6fb709, 0x0d893f64, 0x4f121f81, 0x4f730a48], 10: [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]}

CHAINS = (0, 1, 63, 2 ** 31, 2 ** 32 - 1)
PROBLEMS = (0, 209, 2 ** 32 - 1)
TS = (1, 2, 2 ** 32 - 1)
SEED_WORDS = (0, 2 ** 32 - 1)


@pytest.fixture(scope="module", params=[7, 10])
def shim(request, tmp_path_factory):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler for the host build of the Philox header")
    d = tmp_path_factory.mktemp("philox_uniform_%d" % request.param)
    src, so = d / "shim.c", d / "libshim.so"
    src.write_text(SHIM)
    subprocess.check_call([cc, "-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-shared",
                           "-DPHF_PHILOX_ROUNDS=%d" % request.param, "-I", os.path.join(REPO, "pyhillfit_amd", "csrc"),
                           "-o", str(so), str(src), "-lm"])
    lib = C.CDLL(str(so))
    lib.uniform_diff.restype = C.c_int64
    assert lib.rounds() == request.param
    return lib, request.param


def _run(lib, tuples):
    a = np.ascontiguousarray(np.asarray(tuples, dtype=np.uint64).astype(np.uint32).reshape(-1, 5))
    out = np.empty((len(a), 4), dtype=np.uint32)
    bad = lib.uniform_diff(a.ctypes.data_as(C.c_void_p), C.c_int64(len(a)), out.ctypes.data_as(C.c_void_p))
    return bad, out


def test_known_answer_counters(shim):
    lib, rounds = shim
    bad, out = _run(lib, [ck[:3] + ck[4:] for ck in KAT_COUNTER_KEY])
    assert bad == 0
    assert out[0].tolist() == KAT_ZERO_ANSWER[rounds]          # counter (0, 0, 0, 0), key (0, 0): the published block itself


def test_edge_chains_problems_iterations_and_seeds(shim):
    lib, _ = shim
    tuples = list(itertools.product(CHAINS, PROBLEMS, TS, SEED_WORDS, SEED_WORDS))
    assert len(tuples) == 180
    bad, _ = _run(lib, tuples)
    assert bad == 0


def test_random_tuples(shim):
    lib, _ = shim
    rng = np.random.default_rng(11)
    bad, out = _run(lib, rng.integers(0, 2 ** 32, (100000, 5), dtype=np.uint64))
    assert bad == 0
    assert len(np.unique(out[:, 0])) > 99000                    # (the words were computed, not left at one value)
