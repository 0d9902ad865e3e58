"""CPU precheck of golden G11 (tests/golden/g11_hier_posteriors_few_experiments.json), to be run BEFORE the GPU test
test_gpu_hier_experiment_counts.py::test_g11_few_experiments_match_the_reference_loop:

  1. the CPU twin (oracle/c_oracle.py: the kernels' arithmetic bit for bit) — 32 chains per case at the reference's length, seeds of its
     own — against the fixture under the bar of tests/test_gpu_hierarchical.py::_hier_posteriors_against_reference_loop, restated here:
     every column's pooled mean within 1 % + 4 standard errors of the reference's (the larger of batch means and between-seed scatter),
     every pooled sd within [0.8 - 4 r, 1.2 + 4 r] (clamped to [0.5, 3.0]; r the reference's own relative standard error of its pooled
     sd), acceptance within 0.02 (the bar is restated, not shared: the helper is tied to the GPU sampler — keep the two in step by hand; the
     helper's fixture-level clause, at most 3 % of the entries outside the plain [0.8, 1.2] band, is not restated: see the sd ratios printed);
  2. the reference against itself: the first half of a case's seeds as the fixture, the second half as the run under test, the same bar —
     which says whether the reference's seeds determine a column at all.

    python tests/golden/precheck_few_experiments.py [--workers 7] [--chains 32] > profiles/few_experiments/cpu_precheck.txt
"""
import argparse
import json
import multiprocessing as mp
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
TWIN_SEED = 3028                                   # used by no test and no fixture


def COLUMNS(ne):
    return ["alpha", "beta", "mu", "s"] + [n for e in range(1, ne + 1) for n in ("pic50_%d" % e, "hill_%d" % e)] + ["sigma", "log-target"]


def _twin_chain(job):
    """one twin chain of a case: (case index, per-column mean, per-column variance (ddof 1), acceptance) after the burn-in"""
    from oracle import c_oracle as co
    from pyhillfit_amd import doseresponse as dr
    from pyhillfit_amd import hierarchical as H
    from pyhillfit_amd.sampler import gamma_table
    k, drug, channel, ne, theta0, T, thin, chain_id = job
    dr.setup(os.path.join(REPO, "data", "crumb_dataset.json"))
    shapes, scales, locs = H.prior_params()
    ex = dr.load_crumb_data(drug, channel)[2][:ne]
    pk = co.PackedHierPair(ex, shapes, scales, locs)
    d = 5 + 2 * ne
    st = pk.init_state(np.array(theta0), 0.01)
    rows = pk.advance(st, 0, T, thin, 100 * d, gamma_table(T), seed=TWIN_SEED, chain_id=chain_id, problem_id=k)
    burn_rows = (T // thin + 1) // 4               # saved row 0 is the start point: saved row i >= 1 is rows[i - 1]
    keep = rows[burn_rows - 1:]
    return k, keep.mean(axis=0), keep.var(axis=0, ddof=1), st[-1] / T


def pooled_of_runs(runs):
    means = np.array([r["mean"] for r in runs]); sds = np.array([r["sd"] for r in runs]); ses = np.array([r["batch_means_se"] for r in runs])
    n = len(runs)
    return {"mean": means.mean(axis=0), "sd": np.sqrt((sds ** 2).mean(axis=0) + means.var(axis=0)),
            "se_batch_means": np.sqrt((ses ** 2).sum(axis=0)) / n, "se_between_seeds": means.std(axis=0, ddof=1) / np.sqrt(n)}


def against_the_bar(ref_runs, got_mean, got_sd, got_acc):
    """the helper's comparison: (mean ratio to the bar, sd ratio, sd_lo, sd_hi, acceptance difference) per column"""
    p = pooled_of_runs(ref_runs)
    se = np.maximum(p["se_batch_means"], p["se_between_seeds"])
    ratio = np.abs(got_mean - p["mean"]) / (0.01 * np.abs(p["mean"]) + 4 * se)
    sd_ratio = got_sd / p["sd"]
    run_means = np.array([r["mean"] for r in ref_runs]); run_sds = np.array([r["sd"] for r in ref_runs])
    v_seed = run_sds ** 2 + (run_means - run_means.mean(axis=0)) ** 2
    rel = v_seed.std(axis=0, ddof=1) / np.sqrt(len(ref_runs)) / (2.0 * np.maximum(v_seed.mean(axis=0), 1e-300))
    lo, hi = np.maximum(0.5, 0.8 - 4 * rel), np.minimum(3.0, 1.2 + 4 * rel)
    return ratio, sd_ratio, lo, hi, got_acc - float(np.mean([r["acceptance"] for r in ref_runs]))


def table(title, name, ne, res):
    ratio, sd_ratio, lo, hi, dacc = res
    sd_bar = np.where(sd_ratio >= 1.0, (sd_ratio - 1.0) / (hi - 1.0), (1.0 - sd_ratio) / (1.0 - lo))       # 1 = at the edge of the band
    outside = []
    for c, col in enumerate(COLUMNS(ne)):
        flag = "" if (ratio[c] < 1.0 and lo[c] < sd_ratio[c] < hi[c]) else "   <-- OUTSIDE"
        print("%-34s %-11s mean %6.3f   sd ratio %6.3f in (%.3f, %.3f): %6.3f of the band%s" % (title + " " + name, col, ratio[c], sd_ratio[c], lo[c], hi[c], sd_bar[c], flag))
        if flag:
            outside.append(col)
    flag = "" if abs(dacc) < 0.02 else "   <-- OUTSIDE"
    print("%-34s %-11s difference %+.4f (bar 0.02)%s" % (title + " " + name, "acceptance", dacc, flag))
    return outside + (["acceptance"] if flag else [])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workers", type=int, default=7)
    ap.add_argument("--chains", type=int, default=32)
    ap.add_argument("--fixture", default=os.path.join(REPO, "tests", "golden", "g11_hier_posteriors_few_experiments.json"))
    a = ap.parse_args()
    with open(a.fixture) as f:
        g11 = json.load(f)
    jobs = [(k, e["drug"], e["channel"], e["Ne"], e["first_iteration"], e["iterations"], e["thinning"], c) for k, e in enumerate(g11) for c in range(a.chains)]
    with mp.get_context("fork").Pool(a.workers) as pool:
        done = pool.map(_twin_chain, jobs, chunksize=1)
    print("# G11 CPU precheck: %d twin chains per case (seed %d, chain ids 0..%d, problem id = case index), %d iterations, thinning %d,"
          % (a.chains, TWIN_SEED, a.chains - 1, g11[0]["iterations"], g11[0]["thinning"]))
    print("# against %s; columns: ratio of |mean difference| to 1 %% + 4 s.e.; pooled sd ratio, its band, and where in the band it lies" % os.path.basename(a.fixture))
    bad_twin, bad_ref = {}, {}
    for k, e in enumerate(g11):
        mine = [r for r in done if r[0] == k]
        means = np.array([r[1] for r in mine]); variances = np.array([r[2] for r in mine])
        got_sd = np.sqrt(variances.mean(axis=0) + means.var(axis=0, ddof=1))
        name = "%s-%s Ne=%d" % (e["drug"], e["channel"], e["Ne"])
        out = table("twin", name, e["Ne"], against_the_bar(e["runs"], means.mean(axis=0), got_sd, float(np.mean([r[3] for r in mine]))))
        if out:
            bad_twin[name] = out
    print("#\n# the reference against itself: the second half of each case's seeds under the bar set by the first half")
    for e in g11:
        h = len(e["runs"]) // 2
        a_runs, b_runs = e["runs"][:h], e["runs"][h:]
        b = pooled_of_runs(b_runs)
        name = "%s-%s Ne=%d" % (e["drug"], e["channel"], e["Ne"])
        out = table("seeds %d.. vs %d.." % (b_runs[0]["seed"], a_runs[0]["seed"]), name, e["Ne"],
                    against_the_bar(a_runs, b["mean"], b["sd"], float(np.mean([r["acceptance"] for r in b_runs]))))
        if out:
            bad_ref[name] = out
    print("#\n# twin outside the bar: %s" % (bad_twin or "nothing"))
    print("# reference halves outside each other's bar: %s" % (bad_ref or "nothing"))


if __name__ == "__main__":
    main()
