"""Edge states of the hierarchical sampler: the scenario table of tests/test_gpu_isa_edges.py (the kernels against each other and the twin)
and tests/test_hier_edges_host.py (the twin alone: the conditions that keep the GPU comparison from being vacuous).

A scenario is a list of RUNS on one group of pairs; a run is one launch shape — problems (a pair and a start each), proposal scale, start of
the adaptation.  Every run has C = 130 chains (two full wavefronts and a ragged one), thinning 5, 300 iterations cut as (7, 6, 1, 286)
around adapt_start = 10, moments from iteration 5.  Odd chains take the problem's EDGE start, even chains its HEALTHY one — one wavefront
holds both kinds of lane — except where a run says all chains.  Inputs are tuned against the twin (oracle/c_oracle.PackedHierPair), never
against a kernel; the shares below are the twin's — mean over the seven Crumb shapes (min .. max), each over the eight checked chains of
every problem (tests/test_hier_edges_host.py prints them; per shape: profiles/hier_edges/results.txt).  No proposal of any run has a NaN
log-target: NaN arises as the accept ratio -inf - (-inf) only.

   scenario, run                           accepted               proposals at -inf      proposals outside      saved rows at -inf
   a  on every bound, cov_scale 1          0.233 (0.229..0.237)   0.289 (0.273..0.332)   0.180 (0.166..0.224)   0.169 (0.168..0.169)
   b  outside the support, cov_scale 1     0.247 (0.235..0.262)   0.244 (0.212..0.289)   0.244 (0.212..0.289)   0.104 (0.098..0.133)
   b  outside the support, cov_scale 0.01  0.158 (0.147..0.167)   0.462 (0.429..0.520)   0.462 (0.429..0.520)   0.375 (0.375..0.376)
   c  frozen at -inf                       0.138 (0.129..0.145)   0.540 (0.516..0.598)   0.540 (0.516..0.598)   0.500
   d  zero-variance directions             0.279 (0.271..0.290)   0.093 (0.054..0.178)   0.093 (0.054..0.178)   0
   e  zero covariance                      1                      0                      0                      0
   f  cov_scale 1, no adaptation           0.026 (0.018..0.046)   0.667 (0.606..0.751)   0.667 (0.606..0.751)   0
   f  cov_scale 1e8, no adaptation         0                      1                      1.000 (0.999..1.000)   0
   f  cov_scale 1/8, no adaptation         0.049 (0.035..0.097)   0.250 (0.150..0.314)   0.250 (0.150..0.314)   0
   g  edited data, cov_scale 0.01          0.278 (0.273..0.282)   0.104 (0.084..0.155)   0.104 (0.084..0.155)   0
   g  edited data, cov_scale 1             0.288 (0.283..0.294)   0.132 (0.101..0.149)   0.132 (0.101..0.149)   0
"""
import collections

import numpy as np

from test_gpu_isa import NE4, NE5, NE6, OTHER_SHAPES, THETA0, THETA0_4, THETA0_5, THETA0_6, UNIFORM4

C, THIN, T, ADAPT, CUTS, MOMENTS_AFTER, SEED = 130, 5, 300, 10, (7, 6, 1, 286), 5, 20261019
NO_ADAPT = 10 ** 6                                          # "the adaptation never starts": adapt_start beyond the run
FUSED_CUTS = (5, 10, 285)                                   # the fused grid takes launches that start on a saved row: before, across, after adapt_start
CHECKED = [0, 1, 62, 63, 64, 65, C - 2, C - 1]              # the chains compared with the twin: both kinds of lane, the wavefronts' ends
PROBLEM_ID0, PROBLEM_ID_STEP, CHAIN_ID_BASE = 7, 3, 9       # as test_gpu_isa._setup numbers problems and chains

# one shape for each way the kernels keep their state: (names of three Crumb pairs, their healthy starts)
SHAPES = collections.OrderedDict([
    ("4 + 4 + 4", (UNIFORM4, THETA0)), ("2 + 2 + 2", (OTHER_SHAPES["2 + 2 + 2"], THETA0)), ("5 + 5 + 4", (OTHER_SHAPES["5 + 5 + 4"], THETA0)),
    ("4 + 4 + 4 + 1", (NE4["4 + 4 + 4 + 1"], THETA0_4)), ("5 + 5 + 5 + 1", (NE4["5 + 5 + 5 + 1"], THETA0_4)),
    ("4 + 4 + 4 + 4 + 4", (NE5["4 + 4 + 4 + 4 + 4"], THETA0_5)), ("4 + 4 + 4 + 4 + 2 + 1", (NE6["4 + 4 + 4 + 4 + 2 + 1"], THETA0_6))])
# the code object has the iteration of all fourteen shapes as a BODY of the fused grid, and a kernel of its own (a plain launch,
# phf_hierarchical_last_kernel 4) for these; the other shapes reach the assembly as a fused grid of one group (last kernel 6), which takes
# launches that start on a saved row: FUSED_CUTS
PLAIN_ASSEMBLY = ("4 + 4 + 4", "2 + 2 + 2", "5 + 5 + 4", "4 + 4 + 4 + 1")
# all fourteen launch groups of the fused grid, in the order test_fused_launch_of_fourteen_groups... builds them
FOURTEEN = ([(UNIFORM4, THETA0), (OTHER_SHAPES["2 + 2 + 2"], THETA0), (OTHER_SHAPES["5 + 5 + 4"], THETA0)]
            + [(NE4[k], THETA0_4) for k in ("4 + 4 + 4 + 1", "4 + 4 + 4 + 2", "4 + 4 + 4 + 3", "2 + 2 + 2 + 1", "5 + 5 + 5 + 1")]
            + [(NE5[k], THETA0_5) for k in sorted(NE5)] + [(NE6[k], THETA0_6) for k in sorted(NE6)])
# experiment counts without an assembly kernel (hipcc only): points per experiment of the synthetic pairs.  Ne = 9 runs the
# wavefront-per-chain kernel and, in the twin, phf_hier_log_target_by_experiment
SYNTHETIC = collections.OrderedDict([("ne1", [5]), ("ne2", [4, 3]), ("ne9", [3, 4, 1, 2, 5, 4, 4, 2, 1])])

SCENARIOS = ("a", "b", "c", "d", "e", "f", "g")
FUSED_SCENARIOS = ("a", "c", "d", "g")
SYNTHETIC_SCENARIOS = ("a", "b", "c", "d", "e")

# key: what the run is; pair[q]: which of the group's pairs problem q fits; healthy / edge [Q][dim]; all_chains: every chain takes `edge`;
# edited: the pairs are the group's with values overwritten (edited_experiments)
Run = collections.namedtuple("Run", "key pair healthy edge all_chains cov_scale adapt edited")


def _run(key, pair, healthy, edge, cov_scale, adapt=ADAPT, all_chains=False, edited=False):
    return Run(key, list(pair), np.array(healthy, dtype=np.float64), np.array(edge, dtype=np.float64), all_chains, float(cov_scale), int(adapt), edited)


def _with(theta, index, value):
    th = np.array(theta, dtype=np.float64)
    th[index] = value
    return th


def runs_of(scenario, theta0, locs):
    """the runs of a scenario on a group of three pairs whose healthy starts are theta0[0..2] ([alpha, beta, mu, s, (pIC50_i, Hill_i) x Ne, sigma])"""
    theta0 = [np.asarray(t, dtype=np.float64) for t in theta0]
    dim = theta0[0].size
    ne = (dim - 5) // 2
    pic50 = lambda i: 4 + 2 * i
    hill = lambda i: 5 + 2 * i
    ends = sorted({0, ne - 1})                              # the first and the last experiment (one and the same at Ne = 1)
    three = [0, 1, 2]

    def per_edge(key, edges, cov_scale):                    # one problem per (index, value): pair q % 3
        pair = [q % 3 for q in range(len(edges))]
        return _run(key, pair, [theta0[p] for p in pair], [_with(theta0[p], i, v) for p, (i, v) in zip(pair, edges)], cov_scale)
    if scenario == "a":
        # ON every bound, unit proposal scale.  alpha, beta, mu, s, sigma AT loc_k are outside (<=); Hill_i = 0 and pIC50_i = -2 are inside (<),
        # Hill_i = 0 has log-target -inf all the same (ln Hill_i).  alpha = 0 and Hill_i = 0 also have variance cov_scale |theta_i| = 0: frozen
        edges = [(k, locs[k]) for k in range(4)] + [(dim - 1, locs[4])] + [(hill(i), 0.0) for i in ends] + [(pic50(i), -2.0) for i in ends]
        return [per_edge("on every bound, cov_scale 1", edges, 1.0)]
    if scenario == "b":
        # OUTSIDE the support: the log-target starts at -inf, and some chains step inside
        edges = [(hill(0), -1.0), (pic50(0), -2.5), (dim - 1, 5e-4), (1, 1.5)]
        return [per_edge("outside the support, cov_scale %g" % cs, edges, cs) for cs in (1.0, 0.01)]
    if scenario == "c":
        # alpha = 0: outside, and the variance of alpha is 0 — the odd lanes never leave, every accept ratio is -inf - (-inf) = NaN
        return [_run("frozen at -inf", three, theta0, [_with(t, 0, 0.0) for t in theta0], 0.01)]
    if scenario == "d":
        # a component exactly 0 INSIDE the support: d_k = 0 in the factors, dn = 0 in the update of column k, finite log-targets
        idx = [2, pic50(0), pic50(ne - 1)]
        return [_run("zero-variance directions", three, theta0, [_with(t, i, 0.0) for t, i in zip(theta0, idx)], 0.01)]
    if scenario == "e":
        # cov_scale = 0 from powers of two: the running mean reproduces the state exactly, the covariance stays 0, every pivot is non-positive
        # on every iteration, the proposal is the state and is accepted.  Problems 0 and 1 sit ON pIC50_i = -2 (first / last experiment)
        # with it: every proposal has pIC50_i == -2 exactly, which is inside (<) — a kernel that compared <= would reject all 300
        p2 = [np.concatenate([[1.0, 4.0, 4.0, 0.25], np.tile([4.0, 1.0], ne), [8.0]]), np.concatenate([[2.0, 4.0, 8.0, 0.5], np.tile([8.0, 0.5], ne), [4.0]]),
              np.concatenate([[0.5, 8.0, 4.0, 0.125], np.tile([4.0, 2.0], ne), [16.0]])]
        p2[0][pic50(0)] = -2.0
        p2[1][pic50(ne - 1)] = -2.0
        return [_run("zero covariance", three, p2, p2, 0.0, all_chains=True)]
    if scenario == "f":
        # proposals as wide as the start, and 1e4 times wider, never adapted: exp overflow and underflow, NaN inside the target, the
        # mass-underflow -inf of the truncation term.  At cov_scale 1 a problem whose healthy start sits at its pair's mode accepts NOTHING
        # (4 + 4 + 4 and 5 + 5 + 4, problem 0: 0 of 39 000 proposals over all 130 chains of the twin; 4 + 4 + 4 + 4 + 4, problem 1: 2), so
        # the run at 1/8 stands beside it: the widest power of two at which every problem of every shape has both outcomes on its eight
        # checked chains (4 of 2 400 at the least) with 15 % to 31 % of the proposals still at -inf
        return [_run("cov_scale %g, no adaptation" % cs, three, theta0, theta0, cs, adapt=NO_ADAPT, all_chains=True) for cs in (1.0, 1e8, 0.125)]
    if scenario == "g":
        return [_run("edited data, cov_scale %g" % cs, three, theta0, theta0, cs, all_chains=True, edited=True) for cs in (0.01, 1.0)]
    raise ValueError(scenario)


def starts(run, chains=C):
    """[Q][chains][dim]: odd chains the edge start, even chains the healthy one"""
    th = np.repeat(run.healthy[:, None, :], chains, axis=1)
    th[:, (slice(None) if run.all_chains else slice(1, None, 2)), :] = run.edge[:, None, :]
    return np.ascontiguousarray(th)


def edited_experiments(experiments):
    """a copy of a pair's experiments with one dose 0, one dose 1e-30 and responses of exactly 0, exactly 100, -2.6 and 104 — six different
    points, taken from both ends of the pair so that both halves of the target and the first and last experiment get some; the shape stays"""
    out = [np.array(e, dtype=np.float64) for e in experiments]
    where = [(i, j) for i, e in enumerate(out) for j in range(len(e))]
    n = len(where)
    assert n >= 6
    for (i, j), (col, value) in zip([where[k] for k in (0, n - 1, 1, n - 2, 2, n - 3)],
                                    [(0, 0.0), (0, 1e-30), (1, 0.0), (1, 100.0), (1, -2.6), (1, 104.0)]):
        out[i][j, col] = value
    return out


def experiments_of(run, group_experiments):
    """the experiments of every PROBLEM of a run"""
    return [edited_experiments(group_experiments[p]) if run.edited else group_experiments[p] for p in run.pair]


def synthetic_group(name):
    """three generated pairs with SYNTHETIC[name] points per experiment, and healthy starts near the generating values"""
    from test_gpu_waic import synthetic_pair
    sizes = SYNTHETIC[name]
    rng = np.random.default_rng([20261019, list(SYNTHETIC).index(name)])
    pairs, theta0 = [], []
    for _ in range(3):
        ex, (pic50, hill, sigma) = synthetic_pair(rng, sizes)
        pairs.append(ex)
        theta0.append(np.concatenate([[1.1, 4.5, pic50 + 0.1, 0.3], np.tile([pic50 - 0.1, 1.1 * hill], len(sizes)), [1.2 * sigma]]))
    return pairs, theta0


def twin_run(run, experiments, chains=CHECKED, trace=False, problem_id0=PROBLEM_ID0):
    """the twin on the checked chains of every problem of a run: {(q, c): (rows, final state[, trace])}"""
    from oracle import c_oracle as co
    from pyhillfit_amd import hierarchical as H
    from pyhillfit_amd.sampler import gamma_table
    shapes, scales, locs = H.prior_params()
    gam = gamma_table(T)
    th = starts(run)
    out = {}
    for q, ex in enumerate(experiments):
        pk = co.PackedHierPair(ex, shapes, scales, locs)
        for c in chains:
            st = pk.init_state(th[q, c], run.cov_scale)
            got = pk.advance(st, 0, T, THIN, run.adapt, gam, seed=SEED, chain_id=CHAIN_ID_BASE + c, problem_id=problem_id0 + PROBLEM_ID_STEP * q, trace=trace)
            out[(q, c)] = (got[0], st, got[1]) if trace else (got, st)
    return out
