"""Differential-evolution moves without a GPU: the host build of phf_hier_de.h (the twin of the kernel) against an independent numpy
restatement bit for bit, the exact properties of the move (distinct donors of the other parity, a fair sign, reversibility, NaN and
-inf reject), the C ABI's argument validation and the command line's flags."""
import ctypes as C
import math
import shutil
import subprocess
import os

import numpy as np
import pytest

from conftest import REPO

CSRC = os.path.join(REPO, "pyhillfit_amd", "csrc")
DOMAIN = 0x20000000

SHIM = r"""
#include "phf_hier_de.h"
/* one full round (sub-round 0, then 1) on the C chains of ONE problem: theta [dim][..] with chain stride 1 and coordinate stride ts,
 * lt [C], work like theta, trace [C][6] as the kernel writes it, counts [2] = attempts, accepts */
void v_round(int ne, const int* es, const double* lc, const double* y, const phf_hier_prior* pr, int G, uint32_t cid0, uint32_t pid,
             uint32_t round, uint32_t seed_lo, uint32_t seed_hi, double gamma, int C, int ts, double* theta, double* lt, double* work,
             double* trace, int64_t* counts) {
  for (int h = 0; h < 2; ++h)
    for (int c = h; c < C; c += 2) {
      const int c_pop = c - c % G;
      const phf_de_outcome o = phf_de_move(ne, es, lc, y, pr, G, h, cid0 + (uint32_t)c, pid, round, seed_lo, seed_hi, gamma, theta + c,
                                           theta + c_pop, lt + c, work + c, ts, phf_k_exp, phf_k_log);
      double* tr = trace + 6 * c;
      tr[0] = c_pop + phf_de_donor_slot(o.a, h); tr[1] = c_pop + phf_de_donor_slot(o.b, h);
      tr[2] = o.sg; tr[3] = o.log_u; tr[4] = o.lt_star; tr[5] = o.accepted;
      counts[0] += 1; counts[1] += o.accepted;
    }
}
void v_pick(uint32_t w0, uint32_t w1, uint32_t w2, int n, int* a, int* b, double* sign) { phf_de_pick(w0, w1, w2, n, a, b, sign); }
int v_population_ok(int G) { return phf_de_population_ok(G); }
unsigned v_domain(void) { return PHF_DE_DOMAIN; }
"""


def build_shim(directory):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler for the host build of phf_hier_de.h")
    src, so = directory / "shim.c", directory / "libshim.so"
    src.write_text(SHIM)
    # the flags of oracle/Makefile: the host evaluates the operation sequence the kernels do
    subprocess.check_call([cc, "-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-shared",
                           "-I", CSRC, "-o", str(so), str(src), "-lm"])
    return C.CDLL(str(so))


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shim(tmp_path_factory.mktemp("hier_de"))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def experiments_of(ne, pair=0):
    """ne experiments from the synthetic set: 3 x 4 points of pair `pair`, then (ne == 4: the Crumb shape 4 + 4 + 4 + 1) one point,
    or further copies of the three"""
    from pyhillfit_amd import synthetic
    ex = synthetic.generate(pair + 1)[0][pair]
    if ne <= 3:
        return ex[:ne]
    if ne == 4:
        return ex + [ex[0][1:2]]
    return [ex[i % 3] for i in range(ne)]


def packed_pair(experiments):
    from oracle import c_oracle
    from pyhillfit_amd import hierarchical as H
    shapes, scales, locs = H.prior_params()
    return c_oracle.PackedHierPair(experiments, shapes, scales, locs)


def start_states(experiments, chains, seed, spread=0.03):
    """theta [dim][chains] scattered around the sampler's own start point, and the chains' log-targets"""
    from pyhillfit_amd import bestfit
    from pyhillfit_amd import hierarchical as H
    pair = packed_pair(experiments)
    th0 = np.asarray(bestfit.hierarchical_first_iteration(experiments, H.prior_params()[2]), dtype=np.float64)
    rng = np.random.default_rng(seed)
    theta = np.ascontiguousarray(th0[:, None] * (1.0 + spread * rng.standard_normal((th0.size, chains))))
    lt = np.array([pair.log_target(theta[:, c]) for c in range(chains)])
    assert np.all(np.isfinite(lt))
    return pair, theta, lt


def twin_round(lib, pair, G, cid0, pid, rnd, seed, gamma, theta, lt, ts=None, chains=None):
    """the host twin on one problem, in place: theta [dim][>= chains] (coordinate stride ts doubles), lt [chains]
    -> (trace [chains][6], attempts, accepts, work [dim][ts])"""
    chains = theta.shape[1] if chains is None else chains
    ts = theta.shape[1] if ts is None else ts
    assert theta.dtype == np.float64 and lt.dtype == np.float64
    work = np.full((pair.dim, ts), np.nan)
    trace = np.full((chains, 6), np.nan)
    counts = np.zeros(2, dtype=np.int64)
    lib.v_round(C.c_int(pair.n_expts), _p(pair.expt_start), _p(pair.ln_conc), _p(pair.response), C.byref(pair.pb.prior), C.c_int(G),
                C.c_uint32(cid0), C.c_uint32(pid), C.c_uint32(rnd), C.c_uint32(seed & 0xFFFFFFFF), C.c_uint32(seed >> 32),
                C.c_double(gamma), C.c_int(chains), C.c_int(ts), _p(theta), _p(lt), _p(work), _p(trace), _p(counts))
    return trace, int(counts[0]), int(counts[1]), work


def numpy_round(pair, G, cid0, pid, rnd, seed, gamma, theta, lt):
    """the restatement: Philox words from the oracle, log u from its logarithm, the target from its PackedHierPair; everything else
    numpy.  -> new theta, new lt, trace [chains][6], proposals [dim][chains]"""
    from oracle import c_oracle
    theta, lt = theta.copy(), lt.copy()
    dim, chains = theta.shape
    n = G // 2
    trace, star_all = np.full((chains, 6), np.nan), np.full((dim, chains), np.nan)
    for h in (0, 1):
        for c in range(h, chains, 2):
            w = [int(v) for v in c_oracle.philox([[cid0 + c, pid, rnd, DOMAIN | h, seed & 0xFFFFFFFF, seed >> 32]])[0]]
            a1 = (w[0] * n) >> 32
            b1 = (w[1] * (n - 1)) >> 32
            b1 += 1 if b1 >= a1 else 0
            a, b = min(a1, b1), max(a1, b1)
            sg = (-1.0 if w[2] >> 31 else 1.0) * gamma
            pop = c - c % G
            ca, cb = pop + 2 * a + (1 - h), pop + 2 * b + (1 - h)
            diff = theta[:, ca] - theta[:, cb]
            step = sg * diff
            star = theta[:, c] + step
            u = (w[3] + 0.5) * 2.0 ** -32
            log_u = float(c_oracle.vec("log_fast", [u])[0])
            lt_star = pair.log_target(star)
            acc = bool(log_u < lt_star - lt[c])
            trace[c] = [ca, cb, sg, log_u, lt_star, float(acc)]
            star_all[:, c] = star
            if acc:
                theta[:, c] = star
                lt[c] = lt_star
    return theta, lt, trace, star_all


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- 1. the twin against the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ne", [1, 3])
def test_twin_against_numpy(shim, ne):
    """a population of 8 chains; three rounds in a row (the third with gamma = 1) so that accepted moves feed later proposals"""
    from pyhillfit_amd import de_moves as de
    assert shim.v_domain() == DOMAIN == de.DOMAIN
    pair, theta, lt = start_states(experiments_of(ne), 8, seed=10 + ne)
    gamma = de.default_gamma(pair.dim)
    assert gamma == 2.38 / math.sqrt(2.0 * (5 + 2 * ne))
    seed, cid0, pid = 25 | (7 << 32), 64, 11
    want_theta, want_lt = theta.copy(), lt.copy()
    decisions = []
    for rnd, g in ((1, gamma), (2, gamma), (10, 1.0)):
        want_theta, want_lt, want_trace, want_star = numpy_round(pair, 8, cid0, pid, rnd, seed, g, want_theta, want_lt)
        trace, att, acc, work = twin_round(shim, pair, 8, cid0, pid, rnd, seed, g, theta, lt)
        assert _same_bits(trace, want_trace), (rnd, trace, want_trace)       # donors, sign gamma, log u, L(x'), decision
        assert _same_bits(work, want_star)                                   # the proposals
        assert _same_bits(theta, want_theta) and _same_bits(lt, want_lt)
        assert att == 8 and acc == int(want_trace[:, 5].sum())
        decisions += want_trace[:, 5].tolist()
    assert 0 < sum(decisions) < len(decisions)                               # both branches of the accept test ran


# ---- 2. exact properties ---------------------------------------------------------------------------------------------------------
def _pick(lib, w0, w1, w2, n):
    a, b, s = C.c_int(), C.c_int(), C.c_double()
    lib.v_pick(C.c_uint32(w0), C.c_uint32(w1), C.c_uint32(w2), C.c_int(n), C.byref(a), C.byref(b), C.byref(s))
    return a.value, b.value, s.value


def test_donor_pick_and_sign(shim):
    assert [g for g in range(0, 130) if shim.v_population_ok(g)] == [4, 8, 16, 32, 64]
    rng = np.random.default_rng(3)
    edge = [0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF]
    for n in (2, 4, 8, 16, 32):
        seen = set()
        words = [(a, b) for a in edge for b in edge] + [tuple(int(v) for v in rng.integers(0, 2 ** 32, 2)) for _ in range(4000)]
        for w0, w1 in words:
            a, b, _ = _pick(shim, w0, w1, 0, n)
            assert 0 <= a < b < n, (n, w0, w1, a, b)                         # distinct, ordered, among the n donors
            a1 = (w0 * n) >> 32
            b1 = (w1 * (n - 1)) >> 32
            b1 += b1 >= a1
            assert (a, b) == (min(a1, b1), max(a1, b1))
            seen.add((a, b))
        if n <= 8:
            assert len(seen) == n * (n - 1) // 2                             # every unordered pair can be drawn
    # the sign is the top bit of w2: the two branches, at their boundaries — half of the 2^32 words each, by construction
    for w2, want in ((0, 1.0), (0x7FFFFFFF, 1.0), (0x80000000, -1.0), (0xFFFFFFFF, -1.0)):
        assert _pick(shim, 5, 9, w2, 4)[2] == want


@pytest.mark.parametrize("G", [4, 8])
def test_donors_are_other_parity_of_same_population(shim, G):
    pair, theta, lt = start_states(experiments_of(1), 16, seed=5)
    trace = twin_round(shim, pair, G, 128, 3, 4, 25, 0.6, theta, lt)[0]
    for c in range(16):
        a, b = int(trace[c, 0]), int(trace[c, 1])
        assert a != b and a // G == b // G == c // G and a % 2 == b % 2 == 1 - c % 2, (c, a, b)
        assert abs(trace[c, 2]) == 0.6


def test_reverse_move_returns(shim):
    """from x' with the same donors and the opposite sign: x again, to within one rounding per coordinate"""
    pair, theta, lt = start_states(experiments_of(3), 8, seed=8)
    before = theta.copy()
    trace, _, _, work = twin_round(shim, pair, 8, 0, 0, 1, 25, 0.9, theta, lt)
    for c in range(0, 8, 2):                                                 # sub-round 0: the donors (odd chains) had not moved yet
        a, b, sg = int(trace[c, 0]), int(trace[c, 1]), trace[c, 2]
        star = work[:, c]
        back = star + (-sg) * (before[:, a] - before[:, b])
        assert np.all(np.abs(back - before[:, c]) <= np.spacing(np.maximum(np.abs(before[:, c]), np.abs(star))))
        assert not np.array_equal(star, before[:, c])


def test_nan_rejects(shim):
    pair, theta, lt = start_states(experiments_of(1), 4, seed=2)
    lt[0] = np.nan                                                           # the state's own log-target: the difference is NaN
    theta[2, 1] = np.nan                                                     # a donor of chain 2 (and of chain 0): the proposal is NaN
    before, lt_before = theta.copy(), lt.copy()
    trace, att, acc, _ = twin_round(shim, pair, 4, 0, 0, 1, 25, 0.7, theta, lt)
    assert att == 4 and trace[0, 5] == 0.0 and trace[2, 5] == 0.0
    assert not (trace[2, 4] > -np.inf)                                       # L(x') of a NaN proposal: NaN or -inf
    for c in (0, 2):
        assert _same_bits(theta[:, c], before[:, c]) and _same_bits(lt[c:c + 1], lt_before[c:c + 1])


def test_minus_infinity_rejects(shim):
    """either sign leaves the support (Hill_1 < 0 or pIC50_1 < -2): L(x') = -inf, never accepted"""
    pair, theta, lt = start_states(experiments_of(1), 4, seed=4)
    theta[5, 1], theta[5, 3] = theta[5, 0] + 50.0, theta[5, 0]               # Hill_1 of the two donors of chains 0 and 2: + 50
    theta[4, 1], theta[4, 3] = theta[4, 0], theta[4, 0] + 50.0               # pIC50_1: - 50
    for c in (1, 3):
        lt[c] = pair.log_target(theta[:, c])
    before = theta.copy()
    for rnd in range(1, 9):                                                  # both signs come up
        trace = twin_round(shim, pair, 4, 0, 0, rnd, 25, 1.0, theta, lt)[0]
        for c in (0, 2):
            assert trace[c, 4] == -np.inf and trace[c, 5] == 0.0 and _same_bits(theta[:, c], before[:, c])
        theta[:, 1], theta[:, 3] = before[:, 1], before[:, 3]                # the donors may have moved: put them back
        for c in (1, 3):
            lt[c] = pair.log_target(theta[:, c])


# ---- 3. the C ABI without a GPU --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from pyhillfit_amd import _lib
    return _lib.load()


def test_abi_validation(lib):
    from pyhillfit_amd import _lib
    from pyhillfit_amd import hierarchical as H
    fake = C.c_void_p(8)
    big = C.c_size_t(1 << 40)
    pr = H.make_prior()

    def call(ne=3, Q=2, chains=128, G=64, rnd=1, gamma=0.5, base=0, pts_null=None, prob_null=None, state=fake, work=fake, wb=big,
             stats=fake, sb=big, no_pts=False, no_prob=False, no_prior=False):
        hp = H.HierPoints(1, 16, ne, 0, 8, 8, 8)
        if pts_null:
            setattr(hp, pts_null, None)
        prob = _lib.Problems(Q, chains, 8, 8, 8, base, 0, None, None)
        if prob_null:
            setattr(prob, prob_null, None)
        return lib.phf_hier_de_round(None if no_pts else C.byref(hp), None if no_prob else C.byref(prob), None if no_prior else C.byref(pr),
                                     rnd, 25, G, gamma, state, work, wb, stats, sb, None, None)

    for kw in ({"no_pts": True}, {"no_prob": True}, {"no_prior": True}):
        assert call(**kw) == -1 and b"null points, problems or prior" in lib.phf_last_error()
    for ne in (0, 65):
        assert call(ne=ne) == -3 and b"n_expts" in lib.phf_last_error()
    for f in ("ln_conc", "response", "expt_start"):
        assert call(pts_null=f) == -1 and b"incomplete" in lib.phf_last_error()
    for f in ("pair_index", "problem_id"):
        assert call(prob_null=f) == -1 and b"null pair_index or problem ids" in lib.phf_last_error()
    assert call(Q=0) == -1 and call(chains=0) == -1 and b"positive" in lib.phf_last_error()
    for G in (0, 1, 2, 3, 6, 12, 48, 128, -4):
        assert call(G=G) == -1 and b"population must be 4, 8, 16, 32 or 64" in lib.phf_last_error(), G
    assert call(chains=96, G=64) == -1 and b"multiples of the population" in lib.phf_last_error()
    assert call(chains=100, G=8) == -1 and b"multiples of the population" in lib.phf_last_error()
    assert call(base=32, G=64) == -1 and b"multiples of the population" in lib.phf_last_error()
    for rnd in (0, -1, 1 << 32):
        assert call(rnd=rnd) == -1 and b"round must lie in [1, 2^32)" in lib.phf_last_error()
    for gamma in (0.0, -1.0, float("inf"), float("nan")):
        assert call(gamma=gamma) == -1 and b"gamma" in lib.phf_last_error()
    for kw in ({"state": None}, {"work": None}, {"stats": None}):
        assert call(**kw) == -1 and b"null pointer" in lib.phf_last_error()
    need_w, need_s = 11 * 2 * 128 * 8, 4 * 2 * 2 * 8
    assert lib.phf_hier_de_workspace_bytes(3, 2, 128) == need_w and lib.phf_hier_de_stats_bytes(2, 128) == need_s
    assert call(wb=C.c_size_t(need_w - 1)) == -1 and b"workspace smaller" in lib.phf_last_error()
    assert call(sb=C.c_size_t(need_s - 1)) == -1 and b"stats smaller" in lib.phf_last_error()
    assert call(ne=64, Q=1 << 14, chains=1 << 10) == -1 and b"int32" in lib.phf_last_error()
    # byte counts: 4 int64 counters per (problem, 64-chain block); (5 + 2 Ne) doubles per chain
    for Q, chains in ((1, 4), (1, 64), (3, 65), (210, 1024)):
        assert lib.phf_hier_de_stats_bytes(Q, chains) == 4 * Q * -(-chains // 64) * 8
        assert lib.phf_hier_de_workspace_bytes(9, Q, chains) == 23 * Q * chains * 8
    assert lib.phf_hier_de_stats_bytes(0, 64) == 0 and b"positive" in lib.phf_last_error()
    assert lib.phf_hier_de_workspace_bytes(0, 1, 64) == 0 and lib.phf_hier_de_workspace_bytes(65, 1, 64) == 0
    assert lib.phf_hier_de_stats_init(1, 64, None, big, None) == -1 and b"null stats" in lib.phf_last_error()
    assert lib.phf_hier_de_stats_init(1, 64, fake, C.c_size_t(8), None) == -1 and b"smaller" in lib.phf_last_error()
    assert lib.phf_hier_de_stats_read(1, 64, None, big, fake, None) == -1 and lib.phf_hier_de_stats_read(1, 64, fake, big, None, None) == -1
    assert lib.phf_hier_de_stats_read(1, 64, fake, C.c_size_t(8), fake, None) == -1 and b"smaller" in lib.phf_last_error()


def test_python_settings():
    from pyhillfit_amd import de_moves as de
    de.check_settings(100, 5, 64, 128)
    for kw in (dict(every=0), dict(every=7), dict(population=12), dict(chains=96), dict(gamma=0.0), dict(gamma=float("nan")),
               dict(jump_every=-1)):
        args = dict(every=100, thinning=5, population=64, chains=128, gamma=None, jump_every=10)
        args.update(kw)
        with pytest.raises(ValueError):
            de.check_settings(**args)
    assert de.cut_points(0, 250, 100) == [100, 200, 250] and de.cut_points(250, 400, 100) == [300, 400] and de.cut_points(5, 5, 10) == []
    rec = de.json_record(100, 64, 0.5, 10, 20, 1000, 250, 100, 3)
    assert rec["accept_rate"] == 0.25 and rec["jump_accept_rate"] == 0.03 and rec["rounds"] == 20 and rec["every"] == 100
    assert de.json_record(100, 64, 0.5, 0, 0, 0, 0, 0, 0)["jump_accept_rate"] is None
    line = de.report_line(1, ["A + x", "B + y"], [rec, de.json_record(100, 64, 0.5, 10, 20, 1000, 100, 100, 50)])
    assert "rank 1" in line and "0.1000 (B + y)" in line and "0.0300" in line
    assert "64" in de.COUPLING_NOTE.format(G=64) and "optimistic" in de.COUPLING_NOTE


# ---- 4. the flags ----------------------------------------------------------------------------------------------------------------
def test_parser_flags():
    from pyhillfit_amd import PyHillFit
    p = PyHillFit.build_parser()
    a = p.parse_args(["--data-file", "x.csv", "-m", "2", "--hierarchical"])
    PyHillFit.check_args(p, a)
    assert a.de_every == 0 and a.de_population is None and a.de_gamma is None and a.de_jump_every is None
    a = p.parse_args(["--data-file", "x.csv", "-m", "2", "--hierarchical", "--de-every", "100"])
    PyHillFit.check_args(p, a)
    assert (a.de_every, a.de_population, a.de_gamma, a.de_jump_every) == (100, 64, None, 10)
    a = p.parse_args(["--data-file", "x.csv", "-m", "2", "--hierarchical", "--de-every", "1000", "--de-population", "8", "--de-gamma", "0.4",
                      "--de-jump-every", "0", "--num-chains", "72", "-t", "10"])
    PyHillFit.check_args(p, a)
    assert (a.de_every, a.de_population, a.de_gamma, a.de_jump_every) == (1000, 8, 0.4, 0)


@pytest.mark.parametrize("extra,flag", [
    (["--de-every", "100"], "--hierarchical"),                                            # single-level: refused
    (["--hierarchical", "--de-every", "-5"], "--de-every"),
    (["--hierarchical", "--de-every", "102"], "multiple of the thinning"),                # default thinning 5
    (["--hierarchical", "--de-every", "100", "-t", "3"], "multiple of the thinning"),
    (["--hierarchical", "--de-every", "100", "--de-population", "12"], "--de-population"),
    (["--hierarchical", "--de-every", "100", "--num-chains", "96"], "multiple of the population"),
    (["--hierarchical", "--de-every", "100", "--de-gamma", "0"], "gamma"),
    (["--hierarchical", "--de-every", "100", "--de-jump-every", "-1"], "--de-jump-every"),
    (["--hierarchical", "--de-population", "8"], "--de-every"),
    (["--hierarchical", "--de-gamma", "0.5"], "--de-every"),
])
def test_flag_refusals(extra, flag, capsys):
    from pyhillfit_amd import PyHillFit
    with pytest.raises(SystemExit) as e:
        PyHillFit.main(["--data-file", "does-not-exist.csv", "-m", "2"] + extra)
    assert e.value.code == 2
    assert flag in capsys.readouterr().err
