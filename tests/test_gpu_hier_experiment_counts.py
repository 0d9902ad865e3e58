"""The hierarchical sampler at experiment counts outside the Crumb set's 3..6 (-m gpu): 1 <= Ne <= PHF_HIER_MAX_EXPTS = 64.

The case table (CASES) reaches what no Crumb pair and not the one synthetic Ne = 50 pair launches: hier_*_kernel<1>, <2>, <7>, <8> with their
straight-line (four points in every experiment) and run-time-loop bodies — the instantiations where the register/LDS split of the proposal
factor sits at its ends —, and the wavefront-per-chain kernel at its ends (Ne = 9, 33, 64; experiments of a single point).

  1. the sampler kernels against the CPU twin, bit for bit (launch order, chain offsets, chain-id base, ragged wavefronts, uneven launches);
  2. the same kernels against arithmetic that shares no source with them: the numpy oracle and a 50-digit mpmath restatement of the target;
  3. ChainDiagnostics and PosteriorQuantiles at 8 and 134 columns (the other statistics kernels: test_gpu_waic / _psis / _ppc parameters);
  4. the command lines with -Ne;
  5. golden G11: the reference's own loop on pairs cut to their first 1 and first 2 experiments.

The synthetic pairs come from a seeded numpy generator (Hill curve plus Gaussian noise clipped to [0, 100], doses around the IC50, as
pyhillfit_amd/synthetic.py makes its pairs), so parts 1 to 3 need no fixture."""
import filecmp
import json
import os
import time

import numpy as np
import pytest

from conftest import GOLDEN, REPO
from test_gpu_hierarchical import _hier_posteriors_against_reference_loop, dr_setup, gpu  # noqa: F401
from test_gpu_waic import synthetic_pair

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ONE_LANE, WAVE = 1, 3                     # PHF_HIER_KERNEL_ONE_LANE, PHF_HIER_KERNEL_WAVE (include/pyhillfit_amd.h)

# id -> points per experiment
CASES = {
    "ne1_4": [4],                                  # hier_*_kernel<1>, straight-line body; shape_code has no code for one experiment
    "ne1_1": [1],                                  # <1>, loop body, a single point
    "ne1_7": [7],
    "ne2_4+4": [4, 4],                             # <2> straight-line: what `-Ne 2` runs for most Crumb pairs
    "ne2_4+1": [4, 1],
    "ne2_17+3": [17, 3],                           # an experiment with more than 15 points: no shape code
    "ne7_4each": [4] * 7,
    "ne7_4+4+4+2+2+1+1": [4, 4, 4, 2, 2, 1, 1],    # the list-form shape code at its 7-experiment limit
    "ne8_4each": [4] * 8,                          # the last compiled instantiation: the largest LDS request of the one-lane kernel
    "ne8_5+4+3+2+1+1+2+3": [5, 4, 3, 2, 1, 1, 2, 3],
    "ne9_4each": [4] * 9,                          # the first Ne of the wavefront-per-chain kernel
    "ne33_2,5": [2, 5] * 16 + [2],                 # more experiments than half a wavefront, dim 71: a second factor row for some lanes only
    "ne64_4each": [4] * 64,                        # PHF_HIER_MAX_EXPTS: every lane an experiment, dim 133, the largest LDS request
    "ne64_1each": [1] * 64,
}
CASE_IDS = list(CASES)
T, ADAPT = 420, 150
CUTS = (ADAPT - 3, 4, 101, T - ADAPT - 102)       # uneven launches, the second one straddles adapt_start
SEED, CHAIN_ID_BASE, PROBLEM_IDS, CHAIN_OFFSETS = 20261016, 5, [11, 12, 40], [0, 128, 64]
LAUNCH_ORDER = [2, 0, 1]


def case_pairs(case):
    """the two pairs of a case and their start points (near, not at, the generating values)"""
    rng = np.random.default_rng([2026, CASE_IDS.index(case)])
    sizes = CASES[case]
    pairs, theta0 = [], []
    for _ in range(2):
        ex, (pic50, hill, sigma) = synthetic_pair(rng, sizes)
        pairs.append(ex)
        theta0.append(np.concatenate([[1.1, 4.5, pic50 + 0.1, 0.3], np.tile([pic50 - 0.1, 1.1 * hill], len(sizes)), [1.2 * sigma]]))
    return pairs, theta0


def oracle_tolerance(expts, th, want):
    """the tolerance of test_gpu_full_configs.test_hierarchical_sampled_rows_recomputed_by_the_numpy_oracle, as it stands there:
    1e-12 (|want| + 1) + 4 * 2^-53 * cond, cond the conditioning of SSE / (2 sigma^2) against a relative error in a prediction"""
    from oracle import pyhillfit_oracle as orc
    with np.errstate(all="ignore"):
        cond = sum(np.sum(np.abs(e[:, 1] - orc.hill_curve(e[:, 0], th[5 + 2 * i], orc.ic50_of(th[4 + 2 * i]))) * 100.0) for i, e in enumerate(expts)) / th[-1] ** 2
    return 1e-12 * (abs(want) + 1.0) + 4 * 2.0 ** -53 * cond


def mp_log_target(expts, th, shapes, scales, locs):
    """PyHillFit.py:173-193 written out at 50 digits: the Gaussian truncated to [0, 100] per point (:113-132), the log-logistic level of
    Hill_i (:134-142), the logistic level of pIC50_i (:144-154), the shifted-Gamma hyper-priors of (alpha, beta, mu, s, sigma)"""
    import mpmath as mp
    with mp.workdps(50):
        t = [mp.mpf(float(v)) for v in th]
        alpha, beta, mu, s, sigma = t[0], t[1], t[2], t[3], t[-1]
        total = mp.mpf(0)
        for i, e in enumerate(expts):
            p_i, h_i = t[4 + 2 * i], t[5 + 2 * i]
            ic50 = mp.mpf(10) ** (6 - p_i)
            for dose, y in e:
                pred = 100 * (1 - 1 / (1 + (mp.mpf(float(dose)) / ic50) ** h_i))
                total -= mp.log(sigma) + (mp.mpf(float(y)) - pred) ** 2 / (2 * sigma ** 2) + mp.log(mp.ncdf((100 - pred) / sigma) - mp.ncdf(-pred / sigma))
            total += mp.log(beta) - beta * mp.log(alpha) + (beta - 1) * mp.log(h_i) - 2 * mp.log(1 + (h_i / alpha) ** beta)
            z = (p_i - mu) / s
            total += -z - mp.log(s) - 2 * mp.log(1 + mp.exp(-z))
        for x, k in zip((alpha, beta, mu, s, sigma), range(5)):
            total += (mp.mpf(float(shapes[k])) - 1) * mp.log(x - mp.mpf(float(locs[k]))) - (x - mp.mpf(float(locs[k]))) / mp.mpf(float(scales[k]))
        return float(total)


def random_thetas(rng, ne, m, locs):
    """m parameter vectors: inside the support over the ranges the chains visit and beyond (sigma down to 0.02), and — every eighth vector, in
    turn — alpha, beta, s, sigma AT and BELOW their prior bounds, a Hill_i below 0, a pIC50_i below -2"""
    th = np.column_stack([rng.uniform(0.3, 2.5, m), rng.uniform(2.1, 6.0, m), rng.uniform(3.0, 8.0, m), rng.uniform(0.02, 1.0, m)]
                         + [c for _ in range(ne) for c in (rng.uniform(3.0, 8.0, m), rng.uniform(0.2, 3.0, m))]
                         + [np.exp(rng.uniform(np.log(0.02), np.log(40.0), m))])
    outside = np.zeros(m, dtype=bool)
    for n, i in enumerate(range(0, m, 8)):
        kind = n % 10
        if kind < 8:
            col = (0, 1, 3, -1)[kind // 2]
            bound = locs[(0, 1, 3, 4)[kind // 2]]
            th[i, col] = bound if kind % 2 == 0 else bound - rng.uniform(1e-3, 0.5)
        elif kind == 8:
            th[i, 5 + 2 * rng.integers(ne)] = -rng.uniform(1e-6, 0.5)
        else:
            th[i, 4 + 2 * rng.integers(ne)] = -2.0 - rng.uniform(1e-6, 0.5)
        outside[i] = True
    return th, outside


_KEPT = {}                                 # the runs parts 2 and 3 look at again: (case, 70 chains, thinning) of the configurations in KEEP
KEEP = {(70, 5): CASE_IDS, (70, 1): ["ne1_4", "ne64_4each"]}


def run_case(device, case, C, thin, lanes=0):
    """one sampler run of a case: problems (pair A, pair B, pair A again under another problem id), a launch order that is not the identity,
    chain offsets, a chain-id base, moments from adapt_start on, the advance cut into CUTS.  Returns host arrays."""
    key = (case, C, thin)
    if lanes == 0 and key in _KEPT:
        return _KEPT[key]
    got = _run_case(device, case, C, thin, lanes)
    if lanes == 0 and case in KEEP.get((C, thin), ()):
        _KEPT[key] = got
    return got


def _run_case(device, case, C, thin, lanes):
    from pyhillfit_amd import hierarchical as H
    pairs, theta0 = case_pairs(case)
    packed = H.PackedHierPoints(pairs)
    H.set_kernel_policy(lanes=lanes)
    try:
        s = H.HierarchicalSampler(packed, [0, 1, 0], C, thinning=thin, seed=SEED, adapt_start=ADAPT, problem_ids=PROBLEM_IDS,
                                  chain_id_base=CHAIN_ID_BASE, chain_offsets=CHAIN_OFFSETS, device=device)
        s.launch_order.copy_(torch.tensor(LAUNCH_ORDER, dtype=torch.int32))          # a permutation of its own, in place: prob holds the pointer
        s.init(np.array([theta0[0], theta0[1], theta0[0]]), cov_scale=0.01)
        s.enable_moments(after_iteration=ADAPT)
        row0 = s.row0.cpu().numpy()
        kernels, parts = [], []
        for k in CUTS:
            parts.append(s.advance(k).cpu().numpy())
            kernels.append(H.last_kernel())
        assert s.t == T
        mean, var, n = s.posterior_moments()
        return dict(row0=row0, chain=np.concatenate(parts), state=s.state.cpu().numpy().reshape(s.S, 3, C), kernels=kernels,
                    mean=mean.cpu().numpy(), var=var.cpu().numpy(), n=n, acceptance=s.acceptance().cpu().numpy())
    finally:
        H.set_kernel_policy(0, 0)


# ---- 1. bit identity with the twin ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,thin", [(70, 5), (70, 1), (1, 5), (1, 1)])
@pytest.mark.parametrize("case", CASE_IDS)
def test_chains_bit_identical_to_cpu_twin(case, C, thin, gpu):
    """row 0, every saved row and the final state of chain 0, the last chain and two random ones of every problem == the twin; the kernel the
    case means ran; forcing two lanes per chain changes neither the kernel nor a bit where no two-lane kernel exists (Ne = 1, 2, 7, 8); the
    device moments are the sums of the saved rows; the chains moved"""
    from oracle import c_oracle as co
    from pyhillfit_amd import hierarchical as H
    from pyhillfit_amd.sampler import gamma_table
    shapes, scales, locs = H.prior_params()
    pairs, theta0 = case_pairs(case)
    ne = len(CASES[case])
    d = 5 + 2 * ne
    got = run_case(gpu, case, C, thin)
    chain, state, row0 = got["chain"], got["state"], got["row0"]
    assert chain.shape == (T // thin, 3, d + 1, C) and np.isfinite(chain).all()
    assert got["kernels"] == [ONE_LANE if ne <= 8 else WAVE] * len(CUTS), got["kernels"]
    if ne <= 8:
        forced = run_case(gpu, case, C, thin, 2)
        assert forced["kernels"] == [ONE_LANE] * len(CUTS), forced["kernels"]
        for k in ("row0", "chain", "state", "mean", "var"):
            assert np.array_equal(forced[k], got[k]), k
    gam = gamma_table(T)
    rng = np.random.default_rng([7, CASE_IDS.index(case)])
    picks = sorted({0, C - 1} | set(rng.integers(0, C, 2).tolist()))
    for q, p in enumerate([0, 1, 0]):
        pk = co.PackedHierPair(pairs[p], shapes, scales, locs)
        for c in picks:
            st = pk.init_state(theta0[p], 0.01)
            assert np.array_equal(row0[q, :, c], np.concatenate([theta0[p], [st[d]]])), (q, c)
            rows = pk.advance(st, 0, T, thin, ADAPT, gam, seed=SEED, chain_id=CHAIN_ID_BASE + CHAIN_OFFSETS[q] + c, problem_id=PROBLEM_IDS[q])
            assert np.array_equal(chain[:, q, :, c], rows), (q, c)
            assert np.array_equal(state[:, q, c], st), (q, c)
    assert not np.array_equal(chain[:, 0], chain[:, 2])                      # one pair under two problem ids: two streams
    keep = chain[(ADAPT // thin):]                                            # rows saved at t > adapt_start
    assert got["n"] == keep.shape[0]
    np.testing.assert_allclose(got["mean"], keep.mean(axis=0).transpose(1, 0, 2), rtol=1e-12, atol=1e-12)       # [d+1][Q][C]
    np.testing.assert_allclose(got["var"], keep.var(axis=0, ddof=1).transpose(1, 0, 2), rtol=1e-7, atol=1e-12)
    assert 0.01 < float(got["acceptance"].mean()) < 0.95, got["acceptance"].mean()      # (C = 1: the mean of the three problems' single chains)


# ---- 2. against arithmetic that shares no source with the kernels ----------------------------------------------------------------------
@pytest.mark.parametrize("case", CASE_IDS)
def test_sampled_rows_recomputed_by_the_numpy_oracle(case, gpu):
    """the log-target column of rows the kernels sampled: three (row, chain) picks per problem"""
    from oracle import pyhillfit_oracle as orc
    from pyhillfit_amd import hierarchical as H
    shapes, scales, locs = H.prior_params()
    pairs, _ = case_pairs(case)
    d = 5 + 2 * len(CASES[case])
    chain = run_case(gpu, case, 70, 5)["chain"]
    rng = np.random.default_rng([8, CASE_IDS.index(case)])
    worst = 0.0
    for q, p in enumerate([0, 1, 0]):
        for r, c in zip(rng.integers(0, chain.shape[0], 3), rng.integers(0, 70, 3)):
            th = chain[r, q, :d, c]
            want = orc.hier_log_target(pairs[p], th, shapes, scales, locs)
            worst = max(worst, abs(chain[r, q, d, c] - want) / oracle_tolerance(pairs[p], th, want))
    print("%s: sampled rows against the numpy oracle, worst ratio to the tolerance %.2e" % (case, worst))
    assert worst <= 1.0, worst


@pytest.mark.parametrize("case", CASE_IDS)
def test_log_target_against_twin_numpy_oracle_and_mpmath(case, gpu):
    """phf_hierarchical_log_target at 2 000 random parameter vectors of both pairs of the case, vectors outside the support among them: the
    twin's bits, the numpy oracle's value under the tolerance of the sampled-rows test where finite, -inf exactly where the oracle says so;
    five vectors against the 50-digit restatement (which also checks the oracle)"""
    from oracle import c_oracle as co
    from oracle import pyhillfit_oracle as orc
    from pyhillfit_amd import hierarchical as H
    shapes, scales, locs = H.prior_params()
    pairs, _ = case_pairs(case)
    ne = len(CASES[case])
    rng = np.random.default_rng([9, CASE_IDS.index(case)])
    m = 2000
    th, outside = random_thetas(rng, ne, m, locs)
    pi = rng.integers(0, 2, m).astype(np.int32)
    got = H.log_target_batch(H.PackedHierPoints(pairs), pi, th, device=gpu)
    pks = [co.PackedHierPair(p, shapes, scales, locs) for p in pairs]
    twin = np.array([pks[pi[i]].log_target(th[i]) for i in range(m)])
    assert np.array_equal(got, twin, equal_nan=True)
    want = np.array([orc.hier_log_target(pairs[pi[i]], th[i], shapes, scales, locs) for i in range(m)])
    assert not np.isnan(want).any()
    assert np.all(want[outside] == -np.inf) and np.isfinite(want[~outside]).all()
    assert np.array_equal(got == -np.inf, want == -np.inf) and not np.isnan(got).any()
    fin = np.flatnonzero(np.isfinite(want))
    ratio = np.array([abs(got[i] - want[i]) / oracle_tolerance(pairs[pi[i]], th[i], want[i]) for i in fin])
    print("%s: log_target_batch against the numpy oracle, worst ratio to the tolerance %.2e" % (case, ratio.max()))
    assert ratio.max() <= 1.0, (ratio.max(), th[fin[int(ratio.argmax())]])
    worst_mp, worst_orc = 0.0, 0.0
    for i in fin[rng.choice(len(fin), 5, replace=False)]:
        exact = mp_log_target(pairs[pi[i]], th[i], shapes, scales, locs)
        tol = oracle_tolerance(pairs[pi[i]], th[i], exact)
        worst_mp, worst_orc = max(worst_mp, abs(got[i] - exact) / tol), max(worst_orc, abs(want[i] - exact) / tol)
    print("%s: against mpmath at 50 digits, worst ratio to the tolerance: kernel %.2e, numpy oracle %.2e" % (case, worst_mp, worst_orc))
    assert worst_mp <= 1.0 and worst_orc <= 1.0, (worst_mp, worst_orc)


# ---- 3. diagnostics and quantiles at 8 and 134 columns ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["ne1_4", "ne64_4each"])
def test_diagnostics_and_quantiles_on_sampled_rows(case, gpu):
    """ChainDiagnostics and PosteriorQuantiles (row stride 5 + 2 Ne + 1) on the rows part 1 produced, against the numpy restatements of
    test_gpu_diagnostics and test_gpu_quantiles"""
    from pyhillfit_amd.diagnostics import ChainDiagnostics
    from pyhillfit_amd.quantiles import PosteriorQuantiles
    from test_gpu_diagnostics import compare
    from test_gpu_quantiles import PROBS, check_brackets
    chain = run_case(gpu, case, 70, 1)["chain"][ADAPT:]                      # [270][3][d + 1][70]
    rows, Q, cols, C = chain.shape
    assert cols == 6 + 2 * len(CASES[case])
    t = torch.from_numpy(np.ascontiguousarray(chain)).to(gpu)
    dg = ChainDiagnostics(Q, C, cols, rows, 64, gpu)
    qn = PosteriorQuantiles(Q, C, cols, rows, PROBS, 16384, gpu)
    for a, b in ((0, 77), (77, 78), (78, rows)):
        dg.accumulate(t[a:b].contiguous())
        qn.accumulate(t[a:b].contiguous())
    compare(dg.result(), chain, cols, 64)
    check_brackets(qn.result(), chain)


# ---- 4. the command lines with -Ne -----------------------------------------------------------------------------------------------------
CLI_DRUGS, CLI_CHANNELS = "Amiodarone,Verapamil,Amitriptyline", "hERG,Kv4.3"


def _chain_path(out, drug, channel, ne):
    return os.path.join(out, "crumb_data", "hierarchical", drug, channel, "%d_expts" % ne, "chain", "crumb_data_%s_%s_hierarchical_chain.txt" % (drug, channel))


@pytest.mark.parametrize("num_expts", [1, 2, 7])
def test_cli_num_expts_chain_files_equal_the_twin(num_expts, gpu, tmp_path):
    """PyHillFit --hierarchical -Ne 1 / 2 keeps the first experiments of every pair (4 + 4 + 4, 5 + 5 + 4 and pairs of four to six experiments
    among the six): files under N_expts, the summary says so, chain 0 through the text file == the twin on the cut pair; --fused-launch on
    declines (no cut shape has a gfx950 kernel) and writes the same bytes as off.  -Ne 7, more than any of them has: all are fitted."""
    from oracle import c_oracle as co
    from pyhillfit_amd import PyHillFit
    from pyhillfit_amd import doseresponse as dr
    from pyhillfit_amd import hierarchical as H
    from pyhillfit_amd.sampler import gamma_table
    dr.setup(os.path.join(REPO, "data", "crumb_dataset.json"))
    csv = str(tmp_path / "crumb_data.csv")
    dr.table.to_csv(csv)
    T_cli = 3000
    shapes, scales, locs = H.prior_params()
    all_pairs = [(a, b) for a in dr.drugs for b in dr.channels]
    sizes = {(d, c): [len(x) for x in dr.load_crumb_data(d, c)[2]] for d in CLI_DRUGS.split(",") for c in CLI_CHANNELS.split(",")}
    assert sizes[("Amiodarone", "hERG")] == [4, 4, 4] and sizes[("Verapamil", "hERG")] == [5, 5, 4] and len(sizes[("Amitriptyline", "Kv4.3")]) == 6
    res = {}
    for mode in ("on", "off"):
        out = str(tmp_path / ("output_" + mode))
        res[mode] = (out, PyHillFit.main(["--data-file", csv, "-m", "2", "--hierarchical", "-Ne", str(num_expts), "-i", str(T_cli), "-t", "5",
                                          "--drugs", CLI_DRUGS, "--channels", CLI_CHANNELS, "--num-chains", "64", "--output-root", out,
                                          "--num-APs", "50", "--segment", "1000", "--fused-launch", mode]))
        if num_expts < 3:
            assert H.last_kernel() == ONE_LANE                               # neither the fused grid nor a two-lane kernel exists for Ne = 1, 2
    out, summ = res["off"]
    assert len(summ) == len(res["on"][1]) == 6
    for sm in summ:
        drug, c = sm["drug"], sm["channel"]
        ne = min(num_expts, len(sizes[(drug, c)]))
        assert sm["num_expts"] == ne and len(sm["first_iteration"]) == 5 + 2 * ne
        f = _chain_path(out, drug, c, ne)
        with open(f[:-4] + "_summary.json") as fh:
            assert json.load(fh)["num_expts"] == ne
        assert filecmp.cmp(f, _chain_path(res["on"][0], drug, c, ne), shallow=False), (drug, c)
        chain = np.loadtxt(f)
        assert chain.shape == (T_cli // 5 + 1, 5 + 2 * ne + 1)
        ex = dr.load_crumb_data(drug, c)[2][:ne]
        pk = co.PackedHierPair(ex, shapes, scales, locs)
        st = pk.init_state(np.array(sm["first_iteration"]), 0.01)
        rows = pk.advance(st, 0, T_cli, 5, 100 * (5 + 2 * ne), gamma_table(T_cli), seed=25, chain_id=0, problem_id=all_pairs.index((drug, c)))
        assert np.array_equal(chain[0, :-1], np.array(sm["first_iteration"])) and np.array_equal(chain[1:], rows), (drug, c)
    on = {(b["drug"], b["channel"]): b for b in res["on"][1]}
    for a in summ:
        b = on[(a["drug"], a["channel"])]
        assert a["pooled_mean"] == b["pooled_mean"] and a["pooled_sd"] == b["pooled_sd"] and a["acceptance"] == b["acceptance"]


@pytest.mark.parametrize("num_expts", [1, 2])
def test_cli_num_expts_statistics_and_cdfs(num_expts, gpu, tmp_path):
    """-Ne with --diagnostics --waic --loo --quantiles --ppc: the summary's five blocks are there and finite — ESS and MCSE may be null exactly in the
    columns the diagnostics flag lag_limit_reached, nothing else anywhere —, WAIC's pointwise list has one entry per point of the CUT pair; construct_hierarchical_cdfs -Ne reads the chain file of that run and writes the reference's two CDF files for it"""
    from oracle import pyhillfit_oracle as orc
    from pyhillfit_amd import PyHillFit, construct_hierarchical_cdfs
    from pyhillfit_amd import doseresponse as dr
    dr.setup(os.path.join(REPO, "data", "crumb_dataset.json"))
    csv = str(tmp_path / "crumb_data.csv")
    dr.table.to_csv(csv)
    out = str(tmp_path / "output")
    summ = PyHillFit.main(["--data-file", csv, "-m", "2", "--hierarchical", "-Ne", str(num_expts), "-i", "60000", "-t", "5", "--drugs", CLI_DRUGS,
                           "--channels", CLI_CHANNELS, "--num-chains", "64", "--output-root", out, "--num-APs", "50", "--segment", "10000",
                           "--diagnostics", "--diagnostic-lags", "1024", "--waic", "--loo", "--quantiles", "--ppc"])
    assert len(summ) == 6

    def leaves(x):
        if isinstance(x, dict):
            return [v for y in x.values() for v in leaves(y)]
        if isinstance(x, (list, tuple)):
            return [v for y in x for v in leaves(y)]
        return [x]
    for sm in summ:
        n_points = sum(len(x) for x in dr.load_crumb_data(sm["drug"], sm["channel"])[2][:num_expts])
        assert sm["num_expts"] == num_expts
        for block in ("diagnostics", "waic", "loo", "quantiles", "ppc"):
            assert block in sm, block
        assert len(sm["waic"]["pointwise"]["elpd"]) == n_points == sm["waic"]["n_points"] == sm["loo"]["n_points"] == sm["ppc"]["n_points"]
        assert len(sm["loo"]["pointwise"]["elpd_loo"]) == n_points and len(sm["ppc"]["points"]["pit"]) == n_points
        # the summaries write NaN and infinities as null.  None anywhere in the five blocks, with ONE exception that is the kernel's contract, not a
        # gap: where a column's autocorrelation sum has not turned negative within --diagnostic-lags lags, lag_limit_reached is true and ess /
        # mcse_mean are NaN by design (pyhillfit_amd/diagnostics.py; test_gpu_diagnostics.compare holds the kernel to exactly that).  The run is long
        # enough to mix (60 000 iterations: R-hat below 1.02) and the lag limit raised to 1 024, so that the command-line path does produce ESS
        # and MCSE: on the twin's chains of this very run 0 to 1 column per pair stays flagged, 6 of 10 for Verapamil-Kv4.3 at Ne = 2; at 4 000
        # iterations and the default 256 lags EVERY column is flagged (profiles/few_experiments/results.txt).  So: ess and mcse_mean null exactly in
        # the flagged columns, finite in every other, and at least one column per pair determined.
        dgn = sm["diagnostics"]
        nulls = [(name, k) for name in ("diagnostics", "waic", "loo", "quantiles", "ppc") for k, v in sorted(sm[name].items()) if None in leaves(v)]
        print("-Ne %d %s-%s: null entries %s; lag limit reached in %d of %d columns, k-hat undetermined %d, max k-hat %s, max R-hat %s"
              % (num_expts, sm["drug"], sm["channel"], nulls, sum(dgn["lag_limit_reached"]), len(dgn["rhat"]), sm["loo"]["n_undetermined"],
                 sm["loo"]["max_khat"], max(dgn["rhat"])))
        assert set(nulls) <= {("diagnostics", "ess"), ("diagnostics", "mcse_mean")}, (sm["drug"], sm["channel"], nulls)
        for k in ("ess", "mcse_mean"):
            assert [v is None for v in dgn[k]] == dgn["lag_limit_reached"], (sm["drug"], sm["channel"], k)
        assert None not in dgn["rhat"] and max(dgn["rhat"]) < 1.05 and not all(dgn["lag_limit_reached"]) and dgn["lags"] == 1024
        for name in ("diagnostics", "waic", "loo", "quantiles", "ppc"):
            vals = [v for v in leaves(sm[name]) if isinstance(v, float)]
            assert len(vals) > 0 and np.isfinite(vals).all(), (sm["drug"], sm["channel"], name)
        cols = 6 + 2 * num_expts
        assert all(len(sm["diagnostics"][k]) == cols for k in ("rhat", "ess", "mcse_mean", "lag_limit_reached"))
        assert sm["loo"]["n_undetermined"] == 0 and all(sm["loo"]["pointwise"]["determined"])
        assert sm["ppc"]["invalid"] == 0
    done = construct_hierarchical_cdfs.main(["--data-file", csv, "-a", "-s", "50", "-Ne", str(num_expts), "--output-root", out, "--device", gpu])
    assert sorted(done) == sorted((sm["drug"], sm["channel"]) for sm in summ)
    for sm in summ:
        drug, c = sm["drug"], sm["channel"]
        base = os.path.join(out, "crumb_data", "hierarchical", drug, c, "%d_expts" % num_expts)
        hill = np.loadtxt(os.path.join(base, "cdfs", "crumb_data_%s_%s_posterior_predictive_hill_cdf.txt" % (drug, c)))
        pic50 = np.loadtxt(os.path.join(base, "cdfs", "crumb_data_%s_%s_posterior_predictive_pic50_cdf.txt" % (drug, c)))
        assert hill.shape == (501, 2) and pic50.shape == (501, 2)
        chain = np.loadtxt(_chain_path(out, drug, c, num_expts), usecols=range(4))
        chain = chain[chain.shape[0] // 4:]
        _, hc, _, pc, _, _ = orc.predictive_cdfs(chain[:, 0], chain[:, 1], chain[:, 2], chain[:, 3])
        assert np.allclose(hill[:, 1], hc, rtol=1e-11, atol=1e-70) and np.allclose(pic50[:, 1], pc, rtol=1e-11, atol=1e-70)
    # a cut fit is not what the action-potential step reads: no (Hill, pIC50) sample file (construct_hierarchical_cdfs.py:67-69,139)
    assert not os.path.exists(os.path.join(out, "crumb_data", "hierarchical", "posterior_predictive_hill_pic50_samples"))


# ---- 5. golden G11 ----------------------------------------------------------------------------------------------------------------------
def test_g11_few_experiments_match_the_reference_loop(gpu, dr_setup):
    """Golden G11 (tests/golden/make_golden_posteriors_hier.py --few-experiments; the rule stands in its docstring): the reference's own
    hierarchical loop on the first four G10 pairs cut to their first 1 and first 2 experiments, 8 seeds each at the reference's length.  Here
    512 chains per case from the fixture's start point, a seed not used before, the helper's bar exactly as G10..G10e have it: every column's
    pooled mean within 1 % + 4 standard errors, every pooled sd within 20 % + 4 standard errors of the reference's pooled sd, acceptance
    within 0.02.  No case, no column excepted."""
    with open(os.path.join(GOLDEN, "g11_hier_posteriors_few_experiments.json")) as f:
        g11 = json.load(f)
    assert [(e["drug"], e["channel"], e["Ne"]) for e in g11] == [(d, c, ne) for d, c in (("Amiodarone", "hERG"), ("Amiodarone", "Kv4.3"), ("Dofetilide", "hERG"),
                                                                                       ("Amitriptyline", "Kv4.3")) for ne in (1, 2)]
    t0 = time.time()
    failures = []
    _hier_posteriors_against_reference_loop(gpu, dr_setup, g11, 512, 2028, "g11", failures=failures, first_experiments=True)
    print("g11: %.0f s" % (time.time() - t0))
    assert not failures, failures
