"""The host build of pyhillfit_amd/csrc/phf_drug_profile.h — the twin of the kernels of phf_drug_profile.hip — for the drug-profile
tests: every slot's value in every draw, the tallies, and the histograms those values give on the numpy restatement of the grid
(test_quantiles_host.Histogram)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO

CSRC = os.path.join(REPO, "pyhillfit_amd", "csrc")
GOLDEN = os.path.join(REPO, "tests", "golden", "drug_profile")
CRUMB_CHANNELS = ["hERG", "Nav1.5-peak", "Nav1.5-late", "Cav1.2", "KvLQT1_mink", "Kv4.3", "Kir2.1"]   # the data file's order
VERAPAMIL_CMAX_UM = 0.045

SHIM = r"""
#include "phf_drug_profile.h"
/* values [drugs][D][K + 1][n C] (NaN in the slots that are never fed), tally [drugs][D][2][K + 3], live [drugs][D][K + 1] */
void v_profile(int model, const double* rows, int64_t n, int Q, int stride, int C, int drugs, int K, int D, const int32_t* map,
               const double* weight, const double* ln_dose, double* values, int64_t* tally, int32_t* live) {
  PHF_KFETCH_V(k_exp, phf_k_exp, PHF_K_EXP_N);
  phf_dp_view v;
  v.rows = rows; v.map = map; v.weight = weight; v.ln_dose = ln_dose;
  v.Q = Q; v.stride = stride; v.C = C; v.K = K; v.D = D;
  const int T = PHF_DP_TALLIES(K);
  for (int d = 0; d < drugs; ++d)
    for (int j = 0; j < D; ++j) {
      for (int comp = 0; comp <= K; ++comp) {
        const size_t s = ((size_t)d * D + j) * (K + 1) + comp;
        live[s] = phf_dp_slot_live(&v, d, j, comp);
        for (int64_t r = 0; r < n; ++r)
          for (int c = 0; c < C; ++c)
            values[s * n * C + r * C + c] = live[s] ? phf_dp_slot_value(model, &v, d, j, comp, r, c, k_exp) : PHF_NAN;
      }
      if (!phf_dp_dose_live(&v, d, j)) continue;
      for (int64_t r = 0; r < n; ++r)
        for (int c = 0; c < C; ++c) {
          double net;
          int dominant;
          const int ok = phf_dp_draw(model, &v, d, j, r, c, k_exp, &net, &dominant);
          for (int t = 0; t < T; ++t)
            tally[(((size_t)d * D + j) * 2 + (c & 1)) * T + t] += phf_dp_tally_hit(t, K, ok, net, dominant);
        }
    }
}
double v_weight(const char* name) { return phf_dp_default_weight(name); }
int v_max_channels(void) { return PHF_DP_MAX_CHANNELS; }
int v_max_doses(void) { return PHF_DP_MAX_DOSES; }
"""


def build_shim(directory, extra=()):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler for the host build of phf_drug_profile.h")
    src, so = directory / "shim.c", directory / "libshim.so"
    src.write_text(SHIM)
    # the flags of oracle/Makefile: the host evaluates the operation sequence the kernels do
    subprocess.check_call([cc, "-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-shared", *extra,
                           "-I", CSRC, "-o", str(so), str(src), "-lm"])
    lib = C.CDLL(str(so))
    lib.v_weight.restype = C.c_double
    lib.v_weight.argtypes = [C.c_char_p]
    return lib


@pytest.fixture(scope="session")
def shim(tmp_path_factory):
    return build_shim(tmp_path_factory.mktemp("drug_profile"))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def twin_profile(lib, model, rows, channel_problem, weights, doses):
    """rows [n][Q][stride][C]; -> (values [drugs][D][K + 1][n][C], tally [drugs][D][2][K + 3], live [drugs][D][K + 1])"""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    n, Q, stride, Cn = rows.shape
    cp = np.ascontiguousarray(channel_problem, dtype=np.int32)
    drugs, K = cp.shape
    ln_dose = np.ascontiguousarray(np.log(np.asarray(doses, dtype=np.float64)))
    D = ln_dose.shape[1]
    w = np.ascontiguousarray(weights, dtype=np.float64)
    values = np.zeros((drugs, D, K + 1, n, Cn))
    tally = np.zeros((drugs, D, 2, K + 3), dtype=np.int64)
    live = np.zeros((drugs, D, K + 1), dtype=np.int32)
    lib.v_profile(C.c_int(model), _p(rows), C.c_int64(n), C.c_int(Q), C.c_int(stride), C.c_int(Cn), C.c_int(drugs), C.c_int(K),
                  C.c_int(D), _p(cp), _p(w), _p(ln_dose), _p(values), _p(tally), _p(live))
    return values, tally, live


def twin_histograms(values, bins, cuts=()):
    """values [drugs][D][K + 1][n][C] -> the Histogram of every slot, fed the rows in the segments cut at `cuts`"""
    from test_quantiles_host import Histogram
    out = np.empty(values.shape[:3], dtype=object)
    for idx in np.ndindex(*values.shape[:3]):
        h = Histogram(bins)
        for part in np.split(np.arange(values.shape[3]), list(cuts)):
            if part.size:
                h.feed(values[idx][part])
        out[idx] = h
    return out


def verapamil():
    """(Hill [7][500], pIC50 [7][500]) of the fixture, in the data file's channel order"""
    tabs = [np.loadtxt(os.path.join(GOLDEN, "Verapamil_%s_hill_pic50_samples.txt" % ch)) for ch in CRUMB_CHANNELS]
    return np.array([t[:, 0] for t in tabs]), np.array([t[:, 1] for t in tabs])


def verapamil_rows():
    """the fixture as model-2 rows [500][7][2][1] (pIC50, Hill): problem k is channel k, one chain"""
    hill, pic50 = verapamil()
    rows = np.zeros((500, 7, 2, 1))
    rows[:, :, 0, 0] = pic50.T
    rows[:, :, 1, 0] = hill.T
    return rows


def numpy_block(ln_c, hill, pic50):
    """100 (1 - 1/(1 + exp(min(h (ln c - ln IC50), 40))))"""
    with np.errstate(over="ignore"):
        return 100.0 * (1.0 - 1.0 / (1.0 + np.exp(np.minimum(hill * (ln_c - np.log(10.0) * (6.0 - pic50)), 40.0))))
