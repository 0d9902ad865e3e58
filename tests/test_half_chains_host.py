"""The split of a chain into half-chains without a GPU (pyhillfit_amd/csrc/phf_half_chains.h): the cut of a call's rows into one
sub-segment per half holds exactly the rows the per-row rule assigns to that half, in order, for every call of every short chain."""
import ctypes as C
import shutil
import subprocess

import pytest

from conftest import REPO

SHIM = r"""
#include "phf_half_chains.h"
int v_half_of(int64_t total_rows, int64_t n, int64_t* m) { return phf_half_of(total_rows, n, m); }
/* out[0..3] = offset, nr, m0, closes; returns whether any row of the call falls into the half */
int v_cut(int64_t total_rows, int64_t first_row, int64_t num_rows, int half, int64_t* out) {
  phf_half_segment s = {-1, -1, -1, -1};
  const int any = phf_half_cut(total_rows, first_row, num_rows, half, &s);
  out[0] = s.offset; out[1] = s.nr; out[2] = s.m0; out[3] = s.closes;
  return any;
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler for the host build of phf_half_chains.h")
    d = tmp_path_factory.mktemp("half_chains")
    (d / "shim.c").write_text(SHIM)
    subprocess.check_call([cc, "-O2", "-std=c11", "-fPIC", "-shared", "-Wall", "-Werror", "-I", REPO + "/pyhillfit_amd/csrc", "-o",
                           str(d / "libshim.so"), str(d / "shim.c")])
    return C.CDLL(str(d / "libshim.so"))


def rule(shim, N, n):
    m = C.c_int64(-7)
    return shim.v_half_of(C.c_int64(N), C.c_int64(n), C.byref(m)), m.value


@pytest.mark.parametrize("N", range(2, 14))
def test_cut_holds_the_rows_of_the_rule(shim, N):
    h = N // 2
    halves = [rule(shim, N, n) for n in range(N)]
    assert [hf for hf, _ in halves] == [0] * h + [-1] * (N - 2 * h) + [1] * h                # the middle row of an odd N: neither half
    assert [m for hf, m in halves if hf == 0] == list(range(h)) and [m for hf, m in halves if hf == 1] == list(range(h))
    for first in range(N + 1):
        for num in range(N - first + 1):
            seen = []
            for half in (0, 1):
                out = (C.c_int64 * 4)()
                any_rows = shim.v_cut(C.c_int64(N), C.c_int64(first), C.c_int64(num), half, out)
                want = [(n, halves[n][1]) for n in range(first, first + num) if halves[n][0] == half]      # (row, index in the half)
                assert bool(any_rows) == bool(want), (N, first, num, half)
                if not want:
                    continue
                offset, nr, m0, closes = list(out)
                got = [(first + offset + r, m0 + r) for r in range(nr)]
                assert got == want, (N, first, num, half)
                assert closes == (want[-1][1] == h - 1), (N, first, num, half)
                seen += [n for n, _ in got]
            assert seen == [n for n in range(first, first + num) if halves[n][0] >= 0], (N, first, num)
            if N % 2:
                assert h not in seen                                                       # the dropped middle row
