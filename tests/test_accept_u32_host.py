"""The single-level sampler's accept test for d = 3 (phf_mh_accept_u32, pyhillfit_amd/csrc/phf_model.h) decides
phf_log_pos_k(u_w) < x, u_w = (w + 1/2) / 2^32, from an fp32 estimate of the threshold word and a band around it.  Its proof
 needs two facts about the logarithm on these 2^32 arguments, established here exhaustively on the host build
of phf_math.h (the same operation sequence as the device's, bit for bit: tests/test_gpu_parity.py):
  - E = max over all w of |phf_log_pos_k(u_w) - ln u_w| (against logl: 64-bit significand, ~1e-19 relative), recorded below;
  - phf_log_pos_k(u_w) < 0 for every w (x >= 0 always accepts).
And that phf_mh_draws_w3 draws what phf_mh_draws draws: the same normals, and the word whose logarithm phf_mh_draws returns."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# max |phf_log_pos_k(u_w) - ln u_w| over all 2^32 words, at w = 268 (about one ulp of ln u there); DESIGN.md section 3 uses E < 4e-15
E_RECORDED = 3.544040e-15

SRC = r'''
#include <math.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "phf_model.h"
typedef struct { uint64_t lo, hi, wmax, nonneg; long double emax; } job;
static void* sweep(void* p) {
  job* j = (job*)p;
  PHF_KFETCH_V(k, phf_k_log, PHF_K_LOG_N);
  for (uint64_t w = j->lo; w < j->hi; ++w) {
    const double u = phf_unit_open32((uint32_t)w);
    const double l = phf_log_pos_k(u, k);
    j->nonneg += !(l < 0.0);
    const long double e = fabsl((long double)l - logl((long double)u));
    if (e > j->emax) { j->emax = e; j->wmax = w; }
  }
  return 0;
}
int main(int argc, char** argv) {
  const int nt = atoi(argv[1]);
  pthread_t th[16];
  job jb[16];
  const uint64_t n = 1ull << 32;
  for (int i = 0; i < nt; ++i) {
    jb[i] = (job){n * i / nt, n * (i + 1) / nt, 0, 0, 0.0L};
    if (pthread_create(&th[i], 0, sweep, &jb[i])) return 2;
  }
  long double em = 0.0L;
  uint64_t wm = 0, nonneg = 0;
  for (int i = 0; i < nt; ++i) {
    pthread_join(th[i], 0);
    nonneg += jb[i].nonneg;
    if (jb[i].emax > em) { em = jb[i].emax; wm = jb[i].wmax; }
  }
  /* the two draw functions: same Philox block, same normals, the word of the returned logarithm */
  PHF_KFETCH_V(k, phf_k_log, PHF_K_LOG_N);
  long bad = 0, draws = 0;
  for (uint32_t c = 0; c < 300; c += 7)
    for (uint32_t t = 1; t < 3000; t += 13) {
      double z[3], zw[3];
      const uint32_t s_lo = 25u + 977u * c, s_hi = t * 2654435761u;
      const double lu = phf_mh_draws(3, c, c % 5, t, s_lo, s_hi, k, z);
      const uint32_t w = phf_mh_draws_w3(c, c % 5, t, s_lo, s_hi, zw);
      bad += memcmp(z, zw, sizeof z) != 0 || phf_log_pos_k(phf_unit_open32(w), k) != lu || (lu < 0.5) != phf_mh_accept_u32(0.5, w, k);
      ++draws;
    }
  printf("E %.6Le at %llu nonneg %llu draws %ld bad %ld\n", em, (unsigned long long)wm, (unsigned long long)nonneg, draws, bad);
  return 0;
}
'''


def _threads():
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    return max(1, min(16, n))


def test_log_of_every_accept_word_within_recorded_bound_and_negative(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "accept_u32.c"
    src.write_text(SRC)
    exe = tmp_path / "accept_u32"
    cmd = ["gcc", "-O2", "-std=gnu11", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-pthread",
           "-I", os.path.join(REPO, "pyhillfit_amd", "csrc"), str(src), "-o", str(exe), "-lm"]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe), str(_threads())], capture_output=True, text=True, timeout=3000)
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
    m = re.match(r"E (\S+) at (\d+) nonneg (\d+) draws (\d+) bad (\d+)", run.stdout)
    assert m, run.stdout
    e, nonneg, draws, bad = float(m.group(1)), int(m.group(3)), int(m.group(4)), int(m.group(5))
    assert nonneg == 0                                 # phf_log_pos_k(u_w) < 0 for all 2^32 words
    assert abs(e - E_RECORDED) <= 1e-6 * E_RECORDED, e  # the bound the proof quotes is the one this build has
    assert e < 4e-15
    assert draws == 9933 and bad == 0
