"""Posterior predictive checks without a GPU: finalize()'s mid-p values, means and PIT from hand-made sums, the summary record and the
report line, the host build of phf_ppc.h (the inverse normal CDF against scipy, the random stream's counter domain), the C ABI's
argument validation and the --ppc flag of the command lines."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from scipy.special import ndtri

from conftest import REPO
from pyhillfit_amd import ppc as pp
from pyhillfit_amd import waic as wc

CSRC = os.path.join(REPO, "pyhillfit_amd", "csrc")

SHIM = r"""
#include "phf_ppc.h"
void v_ndtri(int64_t n, const double* p, double* out) { for (int64_t i = 0; i < n; ++i) out[i] = phf_ndtri(p[i]); }
void v_ndtr(int64_t n, const double* x, double* out) { for (int64_t i = 0; i < n; ++i) out[i] = phf_ndtr(x[i]); }
uint32_t ppc_domain(void) { return PHF_PPC_DOMAIN; }
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler for the host build of phf_ppc.h")
    d = tmp_path_factory.mktemp("ppc")
    src, so = d / "shim.c", d / "libshim.so"
    src.write_text(SHIM)
    # the flags of oracle/Makefile: the host evaluates the operation sequence the kernels do
    subprocess.check_call([cc, "-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-shared",
                           "-I", CSRC, "-o", str(so), str(src), "-lm"])
    lib = C.CDLL(str(so))
    lib.ppc_domain.restype = C.c_uint32
    return lib


def _vec(lib, name, x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty_like(x)
    getattr(lib, name)(C.c_int64(x.size), x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return out


# ---- the inverse normal CDF ------------------------------------------------------------------------------------------------------
def test_ndtri_against_scipy(shim):
    rng = np.random.default_rng(1)
    p = np.concatenate([10.0 ** rng.uniform(-300, -0.3, 100000), rng.uniform(0, 1, 100000), 1 - 10.0 ** rng.uniform(-16, -0.3, 100000),
                        [1e-300, 1e-16, 0.075, 0.425, 0.5 - 1e-12, 0.5 + 1e-12, 0.925, 1 - 1e-16]])
    p = p[(p >= 1e-300) & (p <= 1 - 1e-16)]
    got, want = _vec(shim, "v_ndtri", p), ndtri(p)
    f = want != 0.0
    assert np.max(np.abs(got[f] - want[f]) / np.abs(want[f])) <= 1e-14
    assert np.all(got[~f] == 0.0)
    assert np.all(np.diff(got[np.argsort(p)]) >= 0.0)                     # monotone


def test_ndtri_round_trip_and_edges(shim):
    rng = np.random.default_rng(2)
    p = np.concatenate([10.0 ** rng.uniform(-300, 0, 50000), rng.uniform(1e-9, 1 - 1e-9, 50000)])
    p = p[p < 1.0]
    x = _vec(shim, "v_ndtri", p)
    back = _vec(shim, "v_ndtr", x)
    # Phi(x) is as accurate as x allows: a relative error e in x moves Phi by about x^2 e relative
    assert np.all(np.abs(back - p) / p <= 4e-15 * (1.0 + x * x))
    e = _vec(shim, "v_ndtri", [0.0, -1.0, 1.0, 2.0, np.nan, 0.5])
    assert e[0] == -np.inf and e[1] == -np.inf and e[2] == np.inf and e[3] == np.inf and np.isnan(e[4]) and e[5] == 0.0


# ---- the random stream's counter domain ------------------------------------------------------------------------------------------
def test_counter_domain_disjoint_from_samplers(shim):
    """the replicates' blocks set the top bit of counter word 3; the samplers put a block index there, at most a few"""
    from pyhillfit_amd.hierarchical import MAX_EXPTS
    dom = shim.ppc_domain()
    assert dom == 0x80000000
    ppc_src = open(os.path.join(CSRC, "phf_ppc.hip")).read()
    assert "PHF_PPC_DOMAIN | (uint32_t)b" in ppc_src
    # the largest word 3 any sampler uses: the last Philox block of the widest hierarchical parameter vector
    widest = 5 + 2 * MAX_EXPTS
    assert (widest + 3) // 4 - 1 < dom
    # every sampler draw in the sources: word 3 is 0u or a block index (a small loop variable), never a constant with the top bit
    calls = []
    for name in ("phf_model.h", "phf_hier_model.h", "phf_hierarchical.hip", "phf_single_level.hip"):
        src = open(os.path.join(CSRC, name)).read()
        calls += re.findall(r"phf_philox_mh\(([^;]*?)\);", src, flags=re.S)
    assert calls
    for c in calls:
        args = [a.strip() for a in c.split(",")]
        assert len(args) == 6, c
        assert "DOMAIN" not in args[3] and "0x8" not in args[3], c


# ---- finalize, the record, the report line ---------------------------------------------------------------------------------------
def _sums(stats, invalid, pit):
    v = np.zeros(pp.HEAD + len(pit))
    for s, (gt, eq, srep, sobs) in enumerate(stats):
        v[4 * s:4 * s + 4] = gt, eq, srep, sobs
    v[pp.HEAD - 1] = invalid
    v[pp.HEAD:] = pit
    return v


def test_finalize_mid_p_and_pit():
    S_all, invalid = 400, 10
    S = S_all - invalid
    stats = [(100, 0, 390 * 30.0, 390 * 31.0), (150, 40, 390 * 50.0, 390 * 50.0), (390, 0, 390 * 20.0, 390 * 10.0),
             (0, 390, 390 * 2.0, 390 * 2.0), (0, 2, 0.0, 390 * 1.0)]
    pit = np.array([0.5, 0.001, 0.999, 0.0049, 0.9951, 0.005, 0.995]) * S
    r = pp.finalize(_sums(stats, invalid, np.concatenate([pit, [7.0, 9.0]])), 7, S_all)
    assert r["draws"] == S and r["invalid"] == invalid and r["n_points"] == 7
    st = r["statistics"]
    assert st["deviance"]["p"] == 100 / S
    assert st["mean"]["p"] == (150 + 20) / S and st["mean"]["n_greater"] == 150 and st["mean"]["n_equal"] == 40
    assert st["sd"]["p"] == 1.0 and st["zeros"]["p"] == 0.5 and st["hundreds"]["p"] == 1 / S
    assert st["deviance"]["mean_rep"] == pytest.approx(30.0) and st["deviance"]["mean_obs"] == pytest.approx(31.0)
    assert isinstance(st["zeros"]["n_equal"], int)
    np.testing.assert_allclose(r["pit"], pit / S)
    assert r["flagged"].tolist() == [False, True, True, True, True, False, False]
    assert r["n_flagged"] == 4
    assert r["extreme"] == ["sd", "hundreds"]
    empty = pp.finalize(_sums(stats, S_all, np.zeros(2)), 2, S_all)
    assert empty["draws"] == 0 and math.isnan(empty["statistics"]["mean"]["p"]) and np.all(np.isnan(empty["pit"]))


def _points():
    expts = [np.array([[0.1, 0.0], [1.0, 20.0], [10.0, 100.0], [100.0, 120.0]]), np.array([[0.3, 55.5]])]
    return wc.Points.single_level([expts], [[3, 7]])


def test_json_record_and_report_line():
    pts = _points()
    assert pts.count[0] == 4                                               # the response above 100 is dropped, as WAIC drops it
    stats = [(2, 0, 20.0, 22.0), (1, 1, 10.0, 10.0), (0, 0, 4.0, 5.0), (0, 10, 1.0, 1.0), (0, 9, 1.0, 1.0)]
    res = pp.finalize(_sums(stats, 0, [0.5 * 10, 0.001 * 10, 0.7 * 10, 0.3 * 10]), 4, 10)
    rec = pp.json_record(res, pts, 0)
    assert rec["draws"] == 10 and rec["invalid"] == 0 and rec["n_flagged"] == 1
    assert rec["statistics"]["deviance"] == {"p": 0.2, "n_greater": 2, "n_equal": 0, "mean_rep": 2.0, "mean_obs": 2.2}
    assert rec["points"]["experiment"] == [3, 3, 3, 7] and rec["points"]["response"] == [0.0, 20.0, 100.0, 55.5]
    assert rec["points"]["flagged"] == [False, True, False, False]
    assert rec["points"]["pit"][1] == pytest.approx(0.001)
    assert rec["extreme_statistics"] == ["sd"] and "method" in rec
    import json
    json.dumps(rec, allow_nan=False)
    res2 = pp.finalize(_sums([(5, 0, 0, 0)] * 5, 0, [5.0, 5.0, 5.0, 5.0]), 4, 10)
    line = pp.report_line(1, ["A + hERG", "B + Cav1.2"], [res, res2])
    assert line.startswith("ppc [rank 1]: 2 problems, 1 with some p outside [0.01, 0.99]")
    assert "A + hERG (sd p = 0)" in line and "1 of 8 points with PIT outside [0.005, 0.995]" in line
    assert pp.report_line(0, [], []) == "ppc [rank 0]: no problems"


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from pyhillfit_amd import _lib
    return _lib.load()


def test_abi_validation(lib):
    assert lib.phf_ppc_workspace_bytes(3, 7, 65, 100) == 3 * (21 + 7) * 65 * 8
    for bad in ((0, 7, 65, 100), (3, 0, 65, 100), (3, 7, 0, 100), (3, 7, 65, 0), (3, 513, 65, 100)):
        assert lib.phf_ppc_workspace_bytes(*bad) == 0
        assert lib.phf_last_error()
    with pytest.raises(ValueError):
        pp.workspace_bytes(1, 1, 1, 0)
    assert lib.phf_ppc_init(3, 7, 65, 100, None, C.c_size_t(1 << 20), None) == -1 and b"null" in lib.phf_last_error()
    assert lib.phf_ppc_init(3, 7, 65, 100, C.c_void_p(8), C.c_size_t(16), None) == -1 and b"smaller" in lib.phf_last_error()
    assert lib.phf_ppc_reduce(3, 7, 65, 100, C.c_void_p(8), C.c_size_t(16), C.c_void_p(8), None) == -1
    assert lib.phf_ppc_reduce(3, 7, 65, 100, None, C.c_size_t(1 << 20), C.c_void_p(8), None) == -1 and b"null" in lib.phf_last_error()
    from pyhillfit_amd._lib import PointwisePoints
    p = PointwisePoints(2, 4, 8, 8, 8, 8)
    fake, big = C.c_void_p(8), C.c_size_t(1 << 30)
    args = lambda **kw: [kw.get(k, v) for k, v in (("pts", C.byref(p)), ("lik", 2), ("ne", 0), ("rows", fake), ("n", 10), ("Q", 2),
                                                   ("stride", 4), ("C", 64), ("first", 0), ("total", 10), ("pid", fake), ("base", 0),
                                                   ("seed", 25), ("ws", fake), ("wsb", big), ("s", None))]
    assert lib.phf_ppc_accumulate(*args(lik=4)) == -1 and b"likelihood" in lib.phf_last_error()
    assert lib.phf_ppc_accumulate(*args(lik=0)) == -1 and b"likelihood" in lib.phf_last_error()
    assert lib.phf_ppc_accumulate(*args(lik=3)) == -1 and b"num_expts" in lib.phf_last_error()
    assert lib.phf_ppc_accumulate(*args(lik=3, ne=2)) == -1 and b"row_stride_cols" in lib.phf_last_error()
    assert lib.phf_ppc_accumulate(*args(stride=2)) == -1 and b"row_stride_cols" in lib.phf_last_error()
    assert lib.phf_ppc_accumulate(*args(first=5)) == -1 and b"total_rows" in lib.phf_last_error()
    assert lib.phf_ppc_accumulate(*args(n=-1)) == -1 and b"total_rows" in lib.phf_last_error()
    assert lib.phf_ppc_accumulate(*args(Q=3)) == -1 and b"one row per problem" in lib.phf_last_error()
    assert lib.phf_ppc_accumulate(*args(wsb=C.c_size_t(8))) == -1 and b"smaller" in lib.phf_last_error()
    assert lib.phf_ppc_accumulate(*args(rows=None)) == -1 and b"null" in lib.phf_last_error()
    assert lib.phf_ppc_accumulate(*args(pid=None)) == -1 and b"null" in lib.phf_last_error()
    assert lib.phf_ppc_accumulate(*args(pts=None)) == -1 and b"null points" in lib.phf_last_error()
    assert lib.phf_ppc_accumulate(*args(n=0, first=10)) == 0                # nothing to do: no launch
    wide = PointwisePoints(2, 600, 8, 8, 8, 8)
    assert lib.phf_ppc_accumulate(*args(pts=C.byref(wide))) == -1 and b"at most 512" in lib.phf_last_error()
    rep = lambda **kw: [kw.get(k, v) for k, v in (("pts", C.byref(p)), ("lik", 2), ("ne", 0), ("m", 1), ("pi", fake), ("th", fake),
                                                  ("ctr", fake), ("seed", 25), ("y", fake), ("st", fake), ("s", None))]
    assert lib.phf_ppc_replicate(*rep(lik=5)) == -1 and b"likelihood" in lib.phf_last_error()
    assert lib.phf_ppc_replicate(*rep(lik=3)) == -1 and b"num_expts" in lib.phf_last_error()
    assert lib.phf_ppc_replicate(*rep(m=-1)) == -1
    assert lib.phf_ppc_replicate(*rep(ctr=None)) == -1 and b"non-null" in lib.phf_last_error()
    assert lib.phf_ppc_replicate(*rep(pts=None)) == -1 and b"null points" in lib.phf_last_error()
    assert lib.phf_ppc_replicate(*rep(m=0, pi=None, th=None, ctr=None, y=None, st=None)) == 0


def test_python_arguments():
    with pytest.raises(ValueError):
        pp.PosteriorPredictiveCheck(_points(), 2, 1, 4, 10, device="cpu")
    with pytest.raises(ValueError):
        pp.replicate(_points(), 2, [0], [[5.0, 1.0]], [[0, 0, 0]], device="cpu")     # model 2 reads 3 columns


# ---- the command lines ----------------------------------------------------------------------------------------------------------
def test_cli_flag():
    from pyhillfit_amd.PyHillFit import build_parser, check_args
    parser = build_parser()
    for extra in ([], ["--hierarchical"]):
        a = parser.parse_args(["--data-file", "x.csv", "-m", "2", "--ppc"] + extra)
        check_args(parser, a)
        assert a.ppc is True and a.hierarchical == bool(extra)
        b = parser.parse_args(["--data-file", "x.csv", "-m", "1"] + extra)
        assert b.ppc is False


def test_chain_ppc_arguments():
    from pyhillfit_amd import chain_ppc
    with pytest.raises(SystemExit):
        chain_ppc.main(["--seed", "3"])                                    # no data file, no chain file
