"""Integrated leave-one-experiment-out without a GPU: the host build of phf_hier_marginal.h (the twin of the kernel) against an
independent numpy/scipy restatement of the rule, its convergence in the node count on the golden posteriors, the point-mass limit
(a known answer), the C ABI's argument validation, the command lines' flags, the "loo_experiment" record and
compare_models --criterion logo."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
from scipy import stats
from scipy.special import erfc, expit, logsumexp

from conftest import REPO
from test_waic_host import HALF_LN_2PI, hier_loglik

CSRC = os.path.join(REPO, "pyhillfit_amd", "csrc")

SHIM = r"""
#include "phf_hier_marginal.h"
/* experiment with the n points (ln_conc, y) at the m draws phi [5][m] = alpha, beta, mu, s, sigma: out [m][2] = m_i, g_i */
void v_marginal(int Q, const double* nodes, int n, const double* ln_conc, const double* y, int64_t m, const double* phi, double* out) {
  for (int64_t i = 0; i < m; ++i)
    phf_mg_experiment(Q, nodes, n, ln_conc, y, phi[i], phi[m + i], phi[2 * m + i], phi[3 * m + i], phi[4 * m + i], &out[2 * i]);
}
int v_nodes_ok(int Q) { return phf_mg_nodes_ok(Q); }
double v_half_width(void) { return PHF_MG_HALF_WIDTH; }
int v_default_nodes(void) { return PHF_MG_DEFAULT_NODES; }
"""


def build_shim(directory):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler for the host build of phf_hier_marginal.h")
    src, so = directory / "shim.c", directory / "libshim.so"
    src.write_text(SHIM)
    # the flags of oracle/Makefile: the host evaluates the operation sequence the kernels do
    subprocess.check_call([cc, "-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-shared",
                           "-I", CSRC, "-o", str(so), str(src), "-lm"])
    lib = C.CDLL(str(so))
    lib.v_half_width.restype = C.c_double
    return lib


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shim(tmp_path_factory.mktemp("hier_marginal"))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def twin(lib, nodes, ln_conc, y, phi):
    """the host twin: one experiment's points, draws phi [m][5] = (alpha, beta, mu, s, sigma) -> (m_i, g_i), [m] each"""
    from pyhillfit_amd import marginal as mg
    table = np.ascontiguousarray(mg.node_table(nodes))
    lc, yy = np.ascontiguousarray(ln_conc, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    ph = np.ascontiguousarray(np.asarray(phi, dtype=np.float64).reshape(-1, 5).T)
    out = np.empty((ph.shape[1], 2))
    lib.v_marginal(C.c_int(int(nodes)), _p(table), C.c_int(lc.size), _p(lc), _p(yy), C.c_int64(ph.shape[1]), _p(ph), _p(out))
    return out[:, 0].copy(), out[:, 1].copy()


def twin_points(lib, nodes, points, problem_index, theta, threads=16):
    """what MarginalLogLik computes, on the host: theta [m][5 + 2 Ne] -> (m, g), [m][Ne] each.  The (problem, experiment, block of
    vectors) jobs run on a few threads (ctypes releases the interpreter lock): every number is still computed by one serial call"""
    from concurrent.futures import ThreadPoolExecutor
    theta = np.atleast_2d(np.asarray(theta, dtype=np.float64))
    ne = points.num_expts
    m_out, g_out = np.empty((theta.shape[0], ne)), np.empty((theta.shape[0], ne))
    phi = theta[:, [0, 1, 2, 3, 4 + 2 * ne]]
    pi = np.asarray(problem_index)
    jobs = []
    for q in range(points.num_problems):
        rows = np.nonzero(pi == q)[0]
        n = points.count[q]
        for e in range(ne):
            sel = points.tag[q, :n] == e
            for part in np.array_split(rows, max(1, rows.size // 8)):
                if part.size:
                    jobs.append((part, e, points.ln_conc[q, :n][sel], points.response[q, :n][sel]))

    def run(job):
        part, e, lc, y = job
        m_out[part, e], g_out[part, e] = twin(lib, nodes, lc, y, phi[part])

    with ThreadPoolExecutor(max_workers=max(1, min(threads, os.cpu_count() or 1))) as ex:
        list(ex.map(run, jobs))
    return m_out, g_out


# ---- the restatements ---------------------------------------------------------------------------------------------------------------
def rule_nodes(Q, L):
    """nodes and normalised log-weights of the rule, and the even nodes' own normalisation"""
    x = -L + np.arange(Q) * (2.0 * L / Q)
    ld = stats.logistic.logpdf(x)
    return x, ld - logsumexp(ld), ld - logsumexp(ld[::2])


def rule_numpy(Q, conc, y, phi, L=16.0):
    """(m_i, g_i) of the rule from hier_loglik: every (Hill node, pIC50 node) is one 'experiment' of a long hierarchical vector"""
    alpha, beta, mu, s, sigma = [float(v) for v in phi]
    conc, y = np.asarray(conc, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = conc.size
    x, lw, lwc = rule_nodes(Q, L)
    hill, pic50 = alpha * np.exp(x / beta), mu + s * x
    k, l = [v.ravel() for v in np.meshgrid(np.arange(Q), np.arange(Q), indexing="ij")]
    theta = np.concatenate([[alpha, beta, mu, s], np.column_stack([pic50[l], hill[k]]).ravel(), [sigma]])
    if n:
        ll = hier_loglik(np.tile(conc, Q * Q), np.tile(y, Q * Q), np.repeat(np.arange(Q * Q), n), theta).reshape(Q, Q, n).sum(axis=2)
    else:
        ll = np.zeros((Q, Q))
    out = pic50[None, :] < -2.0
    with np.errstate(invalid="ignore"):
        fine = logsumexp(np.where(out, -np.inf, lw[:, None] + lw[None, :] + ll))
        coarse = logsumexp(np.where(out, -np.inf, lwc[:, None] + lwc[None, :] + ll)[::2, ::2])
    return fine, (0.0 if fine == coarse else abs(fine - coarse))


def reference_numpy(conc, y, phi, Q=2048, L=40.0, chunk=128):
    """m_i by the same kind of rule at Q = 2048 nodes a side over [-40, 40): vectorised, pIC50 nodes in chunks"""
    alpha, beta, mu, s, sigma = [float(v) for v in phi]
    x, lw, _ = rule_nodes(Q, L)
    hill, pic50 = alpha * np.exp(x / beta), mu + s * x
    parts = []
    for a in range(0, Q, chunk):
        p = pic50[a:a + chunk]
        ll = np.zeros((Q, p.size))
        for c, yy in zip(conc, y):
            pred = 100.0 * expit(np.minimum(hill[:, None] * (np.log(c) - np.log(10.0) * (6.0 - p[None, :])), 40.0))
            mass = 1.0 - 0.5 * (erfc((100.0 - pred) / sigma / np.sqrt(2.0)) + erfc(pred / sigma / np.sqrt(2.0)))
            ll += -HALF_LN_2PI - np.log(sigma) - (yy - pred) ** 2 / (2.0 * sigma ** 2) - np.log(mass)
        parts.append(logsumexp(np.where(p[None, :] < -2.0, -np.inf, lw[:, None] + lw[a:a + chunk][None, :] + ll)))
    return logsumexp(parts)


def synthetic_experiment(rng, n):
    conc = 10.0 ** rng.uniform(-2, 2, n)
    y = np.clip(100.0 / (1.0 + (3.0 / conc) ** 0.9) + rng.normal(0, 6, n), 0.5, 99.5)
    return conc, y


def random_phi(rng, m):
    """(alpha, beta, mu, s, sigma) from the ranges of test_batch_hierarchical (tests/test_gpu_waic.py)"""
    return np.column_stack([rng.uniform(0.5, 2, m), rng.uniform(2.5, 5, m), rng.uniform(3, 8, m), rng.uniform(0.05, 1, m),
                            rng.uniform(0.5, 40, m)])


# ---- 1. the twin against the restatement -------------------------------------------------------------------------------------------
def test_constants(shim):
    from pyhillfit_amd import marginal as mg
    assert shim.v_half_width() == mg.HALF_WIDTH == 16.0
    assert shim.v_default_nodes() == mg.DEFAULT_NODES == 128
    assert [q for q in range(1, 600) if shim.v_nodes_ok(q)] == list(mg.NODE_CHOICES) == [32, 64, 128, 256]


def test_node_table():
    from pyhillfit_amd import marginal as mg
    for Q in mg.NODE_CHOICES:
        t = mg.node_table(Q)
        x, lw, lwc = rule_nodes(Q, 16.0)
        assert t.shape == (3, Q) and t.dtype == np.float64
        assert np.array_equal(t[0], x) and t[0, 0] == -16.0 and t[0, Q // 2] == 0.0
        assert np.allclose(t[1], lw, rtol=0, atol=1e-13) and np.allclose(t[2, ::2], lwc[::2], rtol=0, atol=1e-13)
        assert np.all(np.isneginf(t[2, 1::2]))
        assert abs(logsumexp(t[1])) < 1e-13 and abs(logsumexp(t[2, ::2])) < 1e-13
    with pytest.raises(ValueError):
        mg.node_table(100)
    with pytest.raises(ValueError):
        mg.check_nodes(48)


@pytest.mark.parametrize("Q", [32, 128])
@pytest.mark.parametrize("n", [1, 4, 5, 13])
def test_twin_against_restatement(shim, Q, n):
    """1e-10 relative to max(|want|, 1): the project's figure for accumulated log-sum-exps"""
    rng = np.random.default_rng(100 * Q + n)
    conc, y = synthetic_experiment(rng, n)
    phi = np.vstack([random_phi(rng, 3),
                     [1.0, 3.0, -1.9, 0.5, 8.0],                       # many pIC50 nodes below -2: left out
                     [1.2, 4.0, 5.0, 0.3, 1e-3],                       # the sigma floor: -inf
                     [1.2, 4.0, 5.0, 0.0, 8.0]])                       # s = 0: NaN
    m, g = twin(shim, Q, np.log(conc), y, phi)
    for i in range(4):
        want_m, want_g = rule_numpy(Q, conc, y, phi[i])
        assert np.isfinite(want_m)
        assert abs(m[i] - want_m) <= 1e-10 * max(abs(want_m), 1.0), (i, m[i], want_m)
        # the gap is a difference of two such numbers
        assert abs(g[i] - want_g) <= 2e-10 * max(abs(want_m), 1.0), (i, g[i], want_g)
    x = rule_nodes(Q, 16.0)[0]
    assert np.sum(-1.9 + 0.5 * x < -2.0) >= Q // 2 - 1                     # the fourth draw does leave out half the nodes
    assert rule_numpy(Q, conc, y, phi[4])[0] == -np.inf
    assert m[4] == -np.inf and g[4] == 0.0
    assert np.isnan(m[5]) and np.isnan(g[5])


def test_invalid_parameters(shim):
    conc, y = synthetic_experiment(np.random.default_rng(5), 4)
    good = [1.0, 3.0, 6.0, 0.3, 8.0]
    m, g = twin(shim, 32, np.log(conc), y, [good])
    assert np.isfinite(m[0]) and np.isfinite(g[0]) and g[0] >= 0
    for i, bad in [(0, np.nan), (1, np.inf), (2, -np.inf), (3, np.nan), (0, 0.0), (0, -1.0), (1, 0.0), (1, -2.0), (3, 0.0), (3, -0.1),
                   (4, np.nan)]:
        phi = list(good)
        phi[i] = bad
        m, g = twin(shim, 32, np.log(conc), y, [phi])
        assert np.isnan(m[0]) and np.isnan(g[0]), (i, bad)
    for sigma in (1e-3, 1e-4, 0.0, -1.0):
        m, g = twin(shim, 32, np.log(conc), y, [good[:4] + [sigma]])
        assert m[0] == -np.inf and g[0] == 0.0
    # no points: the log of the mass of the nodes kept
    m, g = twin(shim, 64, np.zeros(0), np.zeros(0), [good, [1.0, 3.0, -1.9, 0.5, 8.0]])
    x, lw, _ = rule_nodes(64, 16.0)
    assert abs(m[0]) < 1e-12 and abs(m[1] - logsumexp(lw[-1.9 + 0.5 * x >= -2.0])) < 1e-12


# ---- 2. convergence on the golden posteriors -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden_cases():
    """the six pairs of g10_hier_posteriors.json at their pooled posterior means: (name, conc, y, phi, reference) per experiment"""
    from pyhillfit_amd import doseresponse as dr
    dr.setup(os.path.join(REPO, "data", "crumb_dataset.json"))
    with open(os.path.join(REPO, "tests", "golden", "g10_hier_posteriors.json")) as f:
        pairs = json.load(f)
    assert len(pairs) == 6
    cases = []
    for p in pairs:
        ne, _, expts = dr.load_crumb_data(p["drug"], p["channel"])
        assert ne == p["Ne"]
        mean = np.array(p["pooled"]["mean"])
        phi = mean[[0, 1, 2, 3, 4 + 2 * ne]]
        for i, x in enumerate(expts):
            x = np.asarray(x, dtype=np.float64)
            cases.append(("%s %s experiment %d" % (p["drug"], p["channel"], i + 1), x[:, 0], x[:, 1], phi,
                          reference_numpy(x[:, 0], x[:, 1], phi)))
    return cases


def test_convergence_at_256(shim, golden_cases):
    """the twin at Q = 256 against numpy at Q = 2048, L = 40: within 1e-3"""
    worst = 0.0
    for name, conc, y, phi, ref in golden_cases:
        m, _ = twin(shim, 256, np.log(conc), y, [phi])
        err = abs(m[0] - ref)
        print("%-40s Q=256 m=%.6f reference=%.6f error=%.3g" % (name, m[0], ref, err))
        worst = max(worst, err)
        assert err <= 1e-3, (name, m[0], ref)
    print("worst error at Q = 256: %.3g" % worst)


def test_gap_bounds_the_error_at_128(shim, golden_cases):
    """the twin's gap at Q = 128 bounds its error: error <= 1.5 g + 1e-6"""
    for name, conc, y, phi, ref in golden_cases:
        m, g = twin(shim, 128, np.log(conc), y, [phi])
        err = abs(m[0] - ref)
        print("%-40s Q=128 m=%.6f error=%.3g gap=%.3g" % (name, m[0], err, g[0]))
        assert err <= 1.5 * g[0] + 1e-6, (name, err, g[0])


# ---- 3. the point-mass limit -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", [32, 128])
def test_point_mass_limit(shim, Q):
    """beta = 1e9 and s = 1e-9: the population is the point (alpha, mu) (the nodes move H and P by at most 1.6e-8), so m_i is the sum
    of the conditional point terms at (Hill, pIC50) = (alpha, mu) to 1e-4 absolute and g_i < 1e-4"""
    rng = np.random.default_rng(Q)
    for n in (1, 5, 13):
        conc, y = synthetic_experiment(rng, n)
        for alpha, mu, sigma in ((0.9, 5.6, 6.0), (1.7, 6.3, 12.0), (0.6, 4.9, 3.0)):
            m, g = twin(shim, Q, np.log(conc), y, [[alpha, 1e9, mu, 1e-9, sigma]])
            want = float(np.sum(hier_loglik(conc, y, np.zeros(n, dtype=int), [alpha, 1e9, mu, 1e-9, mu, alpha, sigma])))
            assert abs(m[0] - want) <= 1e-4, (n, alpha, mu, sigma, m[0], want)
            assert g[0] < 1e-4


# ---- 4. the C ABI without a GPU --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from pyhillfit_amd import _lib
    return _lib.load()


def _points(stride=8, problems=3, null=None):
    from pyhillfit_amd import _lib
    fake = 8
    p = _lib.PointwisePoints(problems, stride, fake, fake, fake, fake)
    if null:
        setattr(p, null, None)
    return p


def test_abi_validation(lib):
    fake = C.c_void_p(8)

    def batch(pts=None, ne=3, nodes=fake, nq=128, m=10, pi=fake, th=fake, out=fake):
        return lib.phf_hier_marginal_loglik(C.byref(pts or _points()), ne, nodes, nq, m, pi, th, out, None)
    assert batch(pts=_points(null="tag")) == -1 and b"null points" in lib.phf_last_error()
    assert batch(pts=_points(stride=0)) == -1 and b"stride" in lib.phf_last_error()
    assert batch(pts=_points(stride=513)) == -1 and b"512 points" in lib.phf_last_error()
    assert batch(ne=0) == -1 and b"num_expts" in lib.phf_last_error()
    assert batch(ne=65) == -1 and b"num_expts" in lib.phf_last_error()
    for nq in (0, 16, 48, 100, 512):
        assert batch(nq=nq) == -1 and b"num_nodes" in lib.phf_last_error()
    assert batch(nodes=None) == -1 and b"null nodes" in lib.phf_last_error()
    assert batch(m=-1) == -1 and b"phf_hier_marginal_loglik" in lib.phf_last_error()
    for k in ("pi", "th", "out"):
        assert batch(**{k: None}) == -1 and b"non-null" in lib.phf_last_error()
    assert batch(m=0, pi=None, th=None, out=None) == 0                    # nothing to do: no launch

    def rows(pts=None, ne=3, nodes=fake, nq=32, x=fake, n=10, Q=3, stride=14, chains=64, first=0, every=1, ll=fake, gap=fake, gmax=fake):
        return lib.phf_hier_marginal_rows(C.byref(pts or _points()), ne, nodes, nq, x, n, Q, stride, chains, first, every, ll, gap, gmax, None)
    assert rows(Q=2) == -1 and b"one row per problem" in lib.phf_last_error()
    assert rows(chains=0) == -1 and b"num_chains" in lib.phf_last_error()
    assert rows(stride=10) == -1 and b"row_stride_cols" in lib.phf_last_error()
    assert rows(every=0) == -1 and b"every" in lib.phf_last_error()
    assert rows(n=-1) == -1 and b"num_rows" in lib.phf_last_error()
    assert rows(first=-1) == -1 and b"first_row" in lib.phf_last_error()
    assert rows(nq=33) == -1 and b"num_nodes" in lib.phf_last_error()
    for k in ("x", "ll", "gap", "gmax"):
        assert rows(**{k: None}) == -1 and b"null pointer" in lib.phf_last_error()
    assert rows(n=0) == 0
    assert rows(first=1, n=6, every=7, x=None, ll=None, gap=None, gmax=None) == 0     # no row of the call is used: no launch
    # the rows a call uses
    used = lib.phf_hier_marginal_rows_used
    for first, n, every in ((0, 61, 1), (0, 61, 7), (1, 6, 7), (1, 7, 7), (7, 1, 7), (8, 100, 7), (0, 0, 3), (5, 1, 1)):
        want = len([r for r in range(first, first + n) if r % every == 0])
        assert used(first, n, every) == want
        from pyhillfit_amd import marginal as mg
        assert mg.rows_used(first, n, every) == want
    assert used(-1, 1, 1) == -1 and used(0, -1, 1) == -1 and used(0, 1, 0) == -1

    # the accumulators' "given" likelihood: siblings of phf_waic_accumulate / phf_psis_accumulate, which refuse code 4 as before
    big = C.c_size_t(1 << 40)

    def wgiven(pts=None, x=fake, n=5, Q=3, stride=8, chains=64, first=0, total=20, ws=fake, wsb=big):
        return lib.phf_waic_accumulate_given(C.byref(pts or _points()), x, n, Q, stride, chains, first, total, ws, wsb, None)
    assert wgiven(stride=7) == -1 and b"row_stride_cols" in lib.phf_last_error() and b"phf_waic_accumulate_given" in lib.phf_last_error()
    assert wgiven(first=18) == -1 and b"total_rows" in lib.phf_last_error()
    assert wgiven(x=None) == -1 and b"null pointer" in lib.phf_last_error()
    assert wgiven(wsb=C.c_size_t(8)) == -1 and b"smaller" in lib.phf_last_error()
    assert wgiven(Q=2) == -1 and b"one row per problem" in lib.phf_last_error()
    assert wgiven(n=0) == 0
    assert lib.phf_waic_accumulate(C.byref(_points()), 4, 0, fake, 5, 3, 8, 64, 0, 20, fake, big, None) == -1
    assert b"likelihood must be 1, 2" in lib.phf_last_error()

    def pgiven(pts=None, x=fake, n=5, Q=3, stride=8, chains=64, first=0, total=20, ws=fake, wsb=big):
        return lib.phf_psis_accumulate_given(C.byref(pts or _points()), x, n, Q, stride, chains, first, total, 0, ws, wsb, None)
    assert pgiven(stride=7) == -1 and b"row_stride_cols" in lib.phf_last_error() and b"phf_psis_accumulate_given" in lib.phf_last_error()
    assert pgiven(first=18) == -1 and b"total_rows" in lib.phf_last_error()
    assert pgiven(x=None) == -1 and b"null pointer" in lib.phf_last_error()
    assert pgiven(wsb=C.c_size_t(8)) == -1 and b"smaller" in lib.phf_last_error()
    assert pgiven(n=0) == 0
    assert lib.phf_psis_accumulate(C.byref(_points()), 4, 0, fake, 5, 3, 8, 64, 0, 20, 0, fake, big, None) == -1
    assert b"likelihood must be 1, 2" in lib.phf_last_error()


def test_python_arguments():
    from pyhillfit_amd import marginal as mg
    from pyhillfit_amd import waic as wc
    expts = [[np.array([[0.1, 10.0], [1.0, 50.0]]), np.array([[0.3, 20.0]])]]
    hier = wc.Points.hierarchical(expts, [[3, 7]])
    single = wc.Points.single_level(expts)
    with pytest.raises(ValueError):
        mg.MarginalLogLik(single, 32, "cpu")
    with pytest.raises(ValueError):
        mg.MarginalLogLik(hier, 48, "cpu")
    with pytest.raises(ValueError):
        mg.MarginalRows(hier, 1, 4, 32, 0, "cpu")
    # more points in a pair than the kernel's LDS slices hold: refused when the object is made, before any sampling
    many = wc.Points.hierarchical([[np.column_stack([np.full(9, 1.0), np.full(9, 50.0)]) for _ in range(57)]])
    assert many.stride == 513 == mg.MAX_POINTS + 1
    for make in (lambda: mg.MarginalLogLik(many, 32, "cpu"), lambda: mg.MarginalRows(many, 1, 4, 32, 1, "cpu"),
                 lambda: mg.ExperimentLOO(many, 1, 4, 100, 32, 1, "cpu")):
        with pytest.raises(ValueError, match="at most 512 points"):
            make()
    ep = mg.experiment_points(hier)
    assert ep.num_expts is None and ep.count.tolist() == [2] and [i[0] for i in ep.info[0]] == [3, 7] and ep.stride == 2
    assert wc._likelihood("given", ep) == (4, 0) and wc.columns_read("given", ep) == 2
    with pytest.raises(ValueError):
        mg.workspace_bytes(1, 2, 1, 5, 7)                                 # one draw


# ---- 5. the flags ----------------------------------------------------------------------------------------------------------------
def test_parser_flags():
    from pyhillfit_amd import PyHillFit
    from pyhillfit_amd import marginal as mg
    p = PyHillFit.build_parser()
    a = p.parse_args(["--data-file", "x.csv", "-m", "2", "--hierarchical"])
    PyHillFit.check_args(p, a)
    assert a.leave_experiment_out is False and a.marginal_nodes is None and a.marginal_every is None
    a = p.parse_args(["--data-file", "x.csv", "-m", "2", "--hierarchical", "--leave-experiment-out"])
    PyHillFit.check_args(p, a)
    assert a.leave_experiment_out and a.marginal_nodes == mg.DEFAULT_NODES == 128 and a.marginal_every == mg.DEFAULT_EVERY
    a = p.parse_args(["--data-file", "x.csv", "-m", "2", "--hierarchical", "--leave-experiment-out", "--marginal-nodes", "32",
                      "--marginal-every", "5", "--fused-launch", "off", "-Ne", "1"])
    PyHillFit.check_args(p, a)
    assert (a.marginal_nodes, a.marginal_every, a.num_expts) == (32, 5, 1)


@pytest.mark.parametrize("extra,flag", [
    (["--leave-experiment-out"], "--leave-experiment-out"),
    (["--hierarchical", "--marginal-nodes", "64"], "--marginal-nodes"),
    (["--hierarchical", "--marginal-every", "3"], "--marginal-every"),
    (["--hierarchical", "--leave-experiment-out", "--marginal-nodes", "100"], "--marginal-nodes"),
    (["--hierarchical", "--leave-experiment-out", "--marginal-every", "0"], "--marginal-every"),
])
def test_flag_refusals(extra, flag, capsys):
    from pyhillfit_amd import PyHillFit
    with pytest.raises(SystemExit) as e:
        PyHillFit.main(["--data-file", "does-not-exist.csv", "-m", "2"] + extra)
    assert e.value.code == 2
    assert flag in capsys.readouterr().err


def test_chain_tool_refusals(capsys):
    from pyhillfit_amd import chain_loo
    for argv, flag in ((["x.txt", "--data-file", "d.csv", "--marginal-nodes", "64"], "--experiments"),
                       (["x.txt", "--data-file", "d.csv", "--marginal-every", "2"], "--experiments"),
                       (["x.txt", "--data-file", "d.csv", "--experiments", "--marginal-nodes", "65"], "--marginal-nodes"),
                       (["x.txt", "--data-file", "d.csv", "--experiments", "--marginal-every", "0"], "--marginal-every")):
        with pytest.raises(SystemExit) as e:
            chain_loo.main(argv)
        assert e.value.code == 2 and flag in capsys.readouterr().err


# ---- 6. the record ---------------------------------------------------------------------------------------------------------------
def _result(ne=3, S=6400, khat=(0.2, 0.9, 0.5), gap=(1e-6, 0.2, 0.004), det=(1, 1, 1)):
    from pyhillfit_amd import marginal as mg
    elpd = np.array([-13.5, -14.25, -9.0])[:ne]
    lppd = elpd + np.array([0.25, 0.5, 0.125])[:ne]
    lse = lppd + np.log(S) + 0.001
    return mg.finalize(elpd, lppd, np.array(khat)[:ne], np.array(det, dtype=float)[:ne], lse, np.array([0.3, 0.6, 0.1])[:ne],
                       np.array(gap)[:ne], [4, 4, 1][:ne], S)


def test_record_and_report_line():
    from pyhillfit_amd import marginal as mg
    res = _result()
    assert res["elpd_logo"] == -36.75 and res["p_logo"] == pytest.approx(0.875) and res["draws"] == 6400
    assert res["se_elpd_logo"] == pytest.approx(np.sqrt(3 * np.var([-13.5, -14.25, -9.0], ddof=1)))
    assert res["khat_threshold"] == 0.7 and res["n_khat_above_threshold"] == 1 and res["n_gap_above_0.01"] == 1
    rec = mg.json_record(res, [1, 2, 5], 128, 100)
    assert set(rec) == {"elpd_logo", "se_elpd_logo", "p_logo", "lppd", "elpd_waic", "n_experiments", "khat_threshold",
                        "n_khat_above_threshold", "n_gap_above_0.01", "max_khat", "n_undetermined", "draws", "nodes", "every",
                        "experiments", "method"}
    assert rec["nodes"] == 128 and rec["every"] == 100 and rec["n_experiments"] == 3 and len(rec["experiments"]) == 3
    for e, lab, n in zip(rec["experiments"], (1, 2, 5), (4, 4, 1)):
        assert set(e) == {"label", "n_i", "elpd_i", "lppd_i", "khat_i", "determined", "waic", "quadrature_gap_max"}
        assert e["label"] == lab and e["n_i"] == n and e["determined"] is True
        assert set(e["waic"]) == {"lppd_i", "p_waic_i", "elpd_waic_i"}
        assert e["waic"]["elpd_waic_i"] == pytest.approx(e["waic"]["lppd_i"] - e["waic"]["p_waic_i"])
    assert rec["experiments"][1]["quadrature_gap_max"] == 0.2 and rec["experiments"][1]["khat_i"] == 0.9
    assert "Merkle" in rec["method"] and "not renormalised" in rec["method"]
    json.dumps(rec, allow_nan=False)
    line = mg.report_line(0, ["Drug + Chan"], [res], [[1, 2, 5]])
    assert "1 with k-hat > threshold" in line and "Drug + Chan experiment 2" in line and "raise --marginal-nodes" in line
    quiet = mg.report_line(0, ["Drug + Chan"], [_result(gap=(1e-6, 1e-3, 0.004))], [[1, 2, 5]])
    assert "raise --marginal-nodes" not in quiet
    assert mg.report_line(2, [], []) == "loo-experiment [rank 2]: no problems"
    # an experiment PSIS could not determine: its fields and the totals are null
    und = mg.json_record(_result(det=(1, 0, 1)), [1, 2, 5], 32, 7)
    assert und["elpd_logo"] is None and und["se_elpd_logo"] is None and und["n_undetermined"] == 1
    # one experiment: leaving it out leaves the prior; reported, with no standard error
    one = mg.json_record(_result(ne=1), [4], 128, 100)
    assert one["n_experiments"] == 1 and one["elpd_logo"] == -13.5 and one["se_elpd_logo"] is None
    json.dumps(one, allow_nan=False)


# ---- 7. compare_models --criterion logo ---------------------------------------------------------------------------------------------
def _summary(path, drug, elpd, labels=(1, 2, 3), khat=(0.1, 0.2, 0.3), gap=(0.0, 0.0, 0.0), n=(4, 4, 1)):
    rec = {"khat_threshold": 0.7, "experiments": [{"label": l, "n_i": k, "elpd_i": e, "khat_i": h, "quadrature_gap_max": g}
                                                  for l, k, e, h, g in zip(labels, n, elpd, khat, gap)]}
    with open(path, "w") as f:
        json.dump({"drug": drug, "channel": "hERG", "num_expts": len(labels), "loo_experiment": rec}, f)
    return str(path)


def test_compare_models_logo(tmp_path, capsys):
    from pyhillfit_amd import compare_models as cm
    a = _summary(tmp_path / "a_summary.json", "Amiodarone", [-13.0, -14.0, -9.0], khat=(0.1, 0.9, 0.3))
    b = _summary(tmp_path / "b_summary.json", "Amiodarone", [-13.5, -14.25, -9.125], gap=(0.0, 0.5, 0.0))
    rows = cm.main([a, b, "--criterion", "logo"])
    assert json.loads(capsys.readouterr().out)["comparisons"] == rows
    assert len(rows) == 1
    r = rows[0]
    d = np.array([0.5, 0.25, 0.125])
    assert "error" not in r and r["n_points"] == 3 and r["elpd_diff"] == 0.875 and r["elpd_a"] == -36.0 and r["elpd_b"] == -36.875
    assert r["se_diff"] == pytest.approx(np.sqrt(3 * np.var(d, ddof=1))) and r["preferred"] == "A"
    assert (r["n_khat_a"], r["n_khat_b"], r["khat_flagged"]) == (1, 0, True)
    assert (r["n_gap_a"], r["n_gap_b"], r["gap_flagged"]) == (0, 1, True)
    # -Ne subsets: the experiments only one fit holds are refused unless the intersection is asked for
    c = _summary(tmp_path / "c_summary.json", "Amiodarone", [-13.25, -14.5], labels=(1, 2), khat=(0.1, 0.2), gap=(0.0, 0.0), n=(4, 4))
    r = cm.main([a, c, "--criterion", "logo"])[0]
    assert "experiment sets differ" in r["error"] and r["n_only_a"] == 1 and r["n_only_b"] == 0
    r = cm.main([a, c, "--criterion", "logo", "--intersection"])[0]
    assert "error" not in r and r["n_points"] == 2 and r["elpd_diff"] == 0.75
    # not the same data under one label
    e = _summary(tmp_path / "e_summary.json", "Amiodarone", [-13.0, -14.0, -9.0], n=(4, 5, 1))
    assert "different numbers of points" in cm.main([a, e, "--criterion", "logo"])[0]["error"]
    # an experiment without an elpd
    u = _summary(tmp_path / "u_summary.json", "Amiodarone", [-13.0, None, -9.0])
    assert "without an elpd_i" in cm.main([a, u, "--criterion", "logo"])[0]["error"]
    capsys.readouterr()
    # a single-level summary is refused, by name
    s = tmp_path / "s_summary.json"
    s.write_text(json.dumps({"drug": "Amiodarone", "channel": "hERG", "model": 2, "loo": {}}))
    with pytest.raises(SystemExit) as ex:
        cm.main([a, str(s), "--criterion", "logo"])
    assert "single-level" in str(ex.value) and "hierarchical" in str(ex.value)
    # a hierarchical summary written without the flag
    h = tmp_path / "h_summary.json"
    h.write_text(json.dumps({"drug": "Amiodarone", "channel": "hERG", "num_expts": 3}))
    with pytest.raises(SystemExit) as ex:
        cm.main([a, str(h), "--criterion", "logo"])
    assert "--leave-experiment-out" in str(ex.value)
