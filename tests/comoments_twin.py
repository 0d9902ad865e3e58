"""The host build of pyhillfit_amd/csrc/phf_comoments.h, the twin of the co-moment kernels: shared by tests/test_correlations_host.py
and tests/test_gpu_correlations.py (not a test module)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO

CSRC = os.path.join(REPO, "pyhillfit_amd", "csrc")

SHIM = r"""
#include "phf_comoments.h"
void v_accumulate(const double* rows, int64_t num_rows, int Q, int stride, int C, int d, int64_t first_row, int64_t total_rows, double* ws) {
  phf_cm_accumulate_host(rows, num_rows, Q, stride, C, d, first_row, total_rows, ws);
}
void v_reduce(const double* ws, int Q, int C, int d, int64_t total_rows, double* out) { phf_cm_reduce_host(ws, Q, C, d, total_rows, out); }
int v_fields(int d) { return PHF_CM_FIELDS(d); }
int v_out_doubles(int d) { return PHF_CM_OUT_DOUBLES(d); }
int v_pair(int d, int i, int j) { return phf_cm_pair(d, i, j); }
int v_half_of(int64_t total_rows, int64_t n) { int64_t m; return phf_half_of(total_rows, n, &m); }
"""


def build_shim(directory):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler for the host build of phf_comoments.h")
    src, so = directory / "shim.c", directory / "libshim.so"
    src.write_text(SHIM)
    # the flags of oracle/Makefile: the host evaluates the operation sequence the kernels do
    subprocess.check_call([cc, "-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-shared",
                           "-I", CSRC, "-o", str(so), str(src), "-lm"])
    return C.CDLL(str(so))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def twin_accumulate(lib, rows, d, total_rows, first_row=0, ws=None):
    """rows [n][Q][stride][C], the rows first_row.. of total_rows -> ws [Q][2][F][C] (ws: continued)"""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    n, Q, stride, Cn = rows.shape
    assert stride >= d and first_row + n <= total_rows
    if ws is None:
        ws = np.zeros((Q, 2, lib.v_fields(d), Cn))
    lib.v_accumulate(_p(rows), C.c_int64(n), C.c_int(Q), C.c_int(stride), C.c_int(Cn), C.c_int(d), C.c_int64(first_row),
                     C.c_int64(total_rows), _p(ws))
    return ws


def twin_in_calls(lib, rows, d, cuts):
    """the whole run cut into calls at the row indices `cuts`"""
    N, ws, lo = rows.shape[0], None, 0
    for hi in list(cuts) + [N]:
        ws = twin_accumulate(lib, rows[lo:hi], d, N, lo, ws)
        lo = hi
    return ws


def twin_reduce(lib, ws, d, total_rows):
    """ws [Q][2][F][C] -> out [Q][out_doubles(d)]"""
    ws = np.ascontiguousarray(ws)
    Q, _, _, Cn = ws.shape
    out = np.full((Q, lib.v_out_doubles(d)), np.nan)
    lib.v_reduce(_p(ws), C.c_int(Q), C.c_int(Cn), C.c_int(d), C.c_int64(total_rows), _p(out))
    return out


def normal_rows(Q, d, Cn, N, seed, stride=None, fill=0.0):
    """rows [N][Q][stride][C]: column j of problem q is mu_qj + z, z ~ N(0, 1) cut at +-4 (so that a half-chain's first row is within
    4 sd of the mean: the cancellation ratio 1 + shift^2 / variance of the shifted sums is at most 17); columns past d hold `fill`"""
    rng = np.random.default_rng(seed)
    stride = d if stride is None else stride
    rows = np.full((N, Q, stride, Cn), fill, dtype=np.float64)
    mu = rng.uniform(-40.0, 8.0, (Q, d))
    rows[:, :, :d, :] = mu[None, :, :, None] + np.clip(rng.standard_normal((N, Q, d, Cn)), -4.0, 4.0)
    return rows
