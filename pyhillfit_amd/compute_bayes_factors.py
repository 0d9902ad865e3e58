"""Drop-in for the reference's python/compute_bayes_factors.py (thermodynamic integration -> Bayes factor B12).

    python -m pyhillfit_amd.compute_bayes_factors --data-file ../data/crumb_data.csv -d 0 -c 0 [--from-files]

The reference re-reads every rung's chain file and calls dr.log_data_likelihood(..., t=1) once per saved sample in a
Python loop (compute_bayes_factors.py:11-27; 41 rungs x 75 001 samples x 2 models per pair).  Here that expectation
is accumulated inside the tempered sampler kernel itself (the untempered log-likelihood is a by-product of the
tempered one), so normally this script only reads `thermodynamic_integration.json` written by PyHillTemp, applies
the trapezium rule over the ladder (:83, doseresponse.py:192-193) and writes BFs/<drug>_<channel>_B12.txt (:86-100).
With --from-files (or when the JSON is missing) it does what the reference does — sweeps the chain files — but
with the HIP batch evaluator (phf_single_level_log_target) instead of the Python loop.

--estimator stepping-stone takes log Z and its standard error from the "stepping_stone" object PyHillTemp --stepping-stone wrote
(pyhillfit_amd/stepping_stone.py) and prints log B12 +- se; with --from-files it computes chain 0's stepping-stone estimate from the
rung chain files (no standard error: one chain).  The se is the between-chain Monte Carlo error of the runs: it cannot see a bias
that all chains of a rung share, and on the G6 setup the estimate's real error is far larger ("phf_stepping_stone.hip").

--estimator savage-dickey needs no ladder: it reads the "bayes_factor" object PyHillFit -m 2 --savage-dickey wrote into the pair's
model-2 summary (pyhillfit_amd/savage_dickey.py) and prints log B12 +- se."""
import argparse
import json
import os
import sys

import numpy as np

from . import doseresponse as dr
from .PyHillTemp import thermodynamic_integration_file


def log_py_from_chain_files(model, drug, channel, temperatures, concs, responses, device):
    """compute_log_py_approxn (:11-27) for every rung: mean of log L(theta; t=1) over the rows of the rung's chain file"""
    from .sampler import log_target_batch
    packed = dr.PackedPoints([(concs, responses)])
    out = []
    for temp in temperatures:
        _, _, chain_file, _ = dr.nonhierarchical_chain_file_and_figs_dir(model, drug, channel, temp)
        chain = np.loadtxt(chain_file, usecols=range(dr.num_params))                       # :14
        chain = np.atleast_2d(chain)
        lik, _ = log_target_batch(packed, model, np.zeros(len(chain), dtype=np.int32), np.ones(len(chain)), chain, device)
        out.append(float(np.sum(lik) / len(chain)))                                         # :16-24
    return out


def log_z_stepping_stone_from_chain_files(model, drug, channel, temperatures, concs, responses, device):
    """stepping stone of chain 0 (the one chain a rung's file holds): sum over rungs k < R - 1 of LSE_j(Delta_k l_j) - ln n, with
    l = log L(theta; t=1) of every row of the rung's chain file, evaluated by the HIP batch evaluator"""
    from . import stepping_stone as ss
    from .sampler import log_target_batch
    packed = dr.PackedPoints([(concs, responses)])
    delta = ss.deltas(temperatures)
    total = 0.0
    for temp, dk in zip(temperatures[:-1], delta[:-1]):
        _, _, chain_file, _ = dr.nonhierarchical_chain_file_and_figs_dir(model, drug, channel, temp)
        chain = np.atleast_2d(np.loadtxt(chain_file, usecols=range(dr.num_params)))
        lik, _ = log_target_batch(packed, model, np.zeros(len(chain), dtype=np.int32), np.ones(len(chain)), chain, device)
        total += ss.finalize(ss.chain_accumulators(lik[None, :], float(dk)))["log_r"]
    return total


def stepping_stone_main(args, top_drug, top_channel, concs, responses, temps):
    """--estimator stepping-stone: log B12 = log Z_1 - log Z_2 with se = sqrt(se_1^2 + se_2^2)"""
    log_z, se, sources, methods = {}, {}, {}, {}
    for m in (1, 2):
        dr.define_model(m)
        ti_file = thermodynamic_integration_file(m, top_drug, top_channel)
        if args.from_files:
            log_z[m], se[m], sources[m] = log_z_stepping_stone_from_chain_files(m, top_drug, top_channel, temps, concs, responses,
                                                                                args.device), None, "chain files"
            continue
        if not os.path.exists(ti_file):
            raise SystemExit("%s is missing: run PyHillTemp -m %d --stepping-stone first (or use --from-files)" % (ti_file, m))
        with open(ti_file) as f:
            ti = json.load(f)
        if "stepping_stone" not in ti:
            raise SystemExit("%s has no stepping-stone estimate: run PyHillTemp -m %d --stepping-stone" % (ti_file, m))
        if not np.allclose(ti["temperatures"], temps):
            raise SystemExit("ladder in %s does not match --rungs" % ti_file)
        rec = ti["stepping_stone"]
        log_z[m] = float(rec["log_z"]) if rec["log_z"] is not None else float("nan")
        se[m], sources[m] = rec["se"], "stepping stone"
        methods[m] = rec.get("se_method", "independent_rungs")     # "replica_sets": PyHillTemp --swap-every
    log_b12 = log_z[1] - log_z[2]
    log_b12_se = None if se[1] is None or se[2] is None else float(np.sqrt(se[1] ** 2 + se[2] ** 2))
    print(log_z)
    over = " over replica sets" if methods and all(v == "replica_sets" for v in methods.values()) else ""
    print("log B12 = {:.6g} +- {}".format(log_b12, "n/a (one chain)" if log_b12_se is None else
                                          "{:.3g} (between-chain Monte Carlo error{} only, blind to a bias the chains share)".format(log_b12_se, over)))
    drug, channel, _, _ = dr.nonhierarchical_chain_file_and_figs_dir(1, top_drug, top_channel, 1)
    if not os.path.exists(args.bf_dir):
        os.makedirs(args.bf_dir)
    bf_file = args.bf_dir + "{}_{}_B12.txt".format(drug, channel)
    B12 = np.exp(log_b12)
    np.savetxt(bf_file, [B12])
    return {"B12": float(B12), "expectations": log_z, "sources": sources, "file": bf_file, "log_B12": float(log_b12),
            "log_B12_se": log_b12_se, "estimator": "stepping-stone", "se_methods": methods}


def savage_dickey_main(args, top_drug, top_channel):
    """--estimator savage-dickey: log B12 and its se from the "bayes_factor" object PyHillFit -m 2 --savage-dickey wrote into the
    pair's model-2 summary; no ladder and no model-1 fit"""
    dr.define_model(2)
    drug, channel, chain_file, _ = dr.nonhierarchical_chain_file_and_figs_dir(2, top_drug, top_channel, 1)
    summary = chain_file[:-4] + "_summary.json"
    run = "run PyHillFit -m 2 --savage-dickey --drugs {} --channels {} first".format(top_drug, top_channel)
    if not os.path.exists(summary):
        raise SystemExit("%s is missing: %s" % (summary, run))
    with open(summary) as f:
        rec = json.load(f).get("bayes_factor")
    if rec is None:
        raise SystemExit("%s has no Savage-Dickey Bayes factor: %s" % (summary, run))
    if rec["log_b12"] is None:
        raise SystemExit("%s: the Bayes factor is not finite (%s)" % (summary, rec.get("reason")))
    log_b12, se = float(rec["log_b12"]), rec["log_b12_se"]
    print("log B12 = {:.6g} +- {}".format(log_b12, "n/a (one chain)" if se is None else
                                          "{:.3g} (between-chain Monte Carlo error only)".format(se)))
    if not rec["reliable"]:
        print("not reliable: {}".format(rec.get("reason")))
    if not os.path.exists(args.bf_dir):
        os.makedirs(args.bf_dir)
    bf_file = args.bf_dir + "{}_{}_B12.txt".format(drug, channel)
    B12 = np.exp(log_b12)
    np.savetxt(bf_file, [B12])
    return {"B12": float(B12), "sources": {2: "savage-dickey"}, "file": bf_file, "log_B12": log_b12, "log_B12_se": se,
            "estimator": "savage-dickey", "reliable": bool(rec["reliable"])}


def main(argv=None):
    parser = argparse.ArgumentParser(prog="compute_bayes_factors.py")
    parser.add_argument("-nc", "--num-cores", type=int, default=1, help="accepted for compatibility")
    req = parser.add_argument_group('required arguments')
    req.add_argument("-d", "--drug", type=int, help="drug index", required=True)
    req.add_argument("-c", "--channel", type=int, help="channel index", required=True)
    req.add_argument("--data-file", type=str, required=True)
    new = parser.add_argument_group('MI355X options')
    new.add_argument("--from-files", action="store_true", help="sweep the chain files (reference method) instead of the fused sums")
    new.add_argument("--rungs", type=int, default=None)
    new.add_argument("--device", type=str, default="cuda:0")
    new.add_argument("--output-root", type=str, default="output")
    new.add_argument("--bf-dir", type=str, default="BFs/")
    new.add_argument("--estimator", choices=("ti", "stepping-stone", "savage-dickey"), default="ti",
                     help="ti: thermodynamic integration (the reference's); stepping-stone: PyHillTemp --stepping-stone's log Z with its se; "
                          "savage-dickey: the \"bayes_factor\" PyHillFit -m 2 --savage-dickey wrote (no ladder)")
    if argv is None and len(sys.argv) == 1:
        parser.print_help(); sys.exit(1)
    args = parser.parse_args(argv)
    dr.setup(args.data_file)
    dr.output_root = args.output_root
    top_drug, top_channel = dr.drugs[args.drug], dr.channels[args.channel]                 # :50-51
    if args.estimator == "savage-dickey":
        return savage_dickey_main(args, top_drug, top_channel)
    num_expts, _, experiments = dr.load_crumb_data(top_drug, top_channel)
    concs, responses = dr.concatenate_experiments(num_expts, experiments)                  # :55-59
    temps = dr.temperature_ladder(args.rungs)                                              # :70
    if args.estimator == "stepping-stone":
        return stepping_stone_main(args, top_drug, top_channel, concs, responses, temps)
    expectations, sources = {}, {}
    for m in (1, 2):                                                                       # :67
        dr.define_model(m)
        ti_file = thermodynamic_integration_file(m, top_drug, top_channel)
        if os.path.exists(ti_file) and not args.from_files:
            with open(ti_file) as f:
                ti = json.load(f)
            if not np.allclose(ti["temperatures"], temps):
                raise SystemExit("ladder in %s does not match --rungs" % ti_file)
            log_p_ys, sources[m] = np.array(ti["log_py_pooled"]), "fused"
        else:
            log_p_ys, sources[m] = np.array(log_py_from_chain_files(m, top_drug, top_channel, temps, concs, responses, args.device)), "chain files"
        print(log_p_ys)
        expectations[m] = dr.trapezium_rule(temps, log_p_ys)                               # :83
    print(expectations)
    drug, channel, _, _ = dr.nonhierarchical_chain_file_and_figs_dir(1, top_drug, top_channel, 1)
    if not os.path.exists(args.bf_dir):
        os.makedirs(args.bf_dir)
    bf_file = args.bf_dir + "{}_{}_B12.txt".format(drug, channel)                          # :90
    B12 = np.exp(expectations[1] - expectations[2])                                        # :94
    np.savetxt(bf_file, [B12])                                                             # :100
    return {"B12": float(B12), "expectations": expectations, "sources": sources, "file": bf_file}


if __name__ == "__main__":
    main()
