"""Drop-in for the sampling step of the reference's python/PyHillFit.py, on MI355X.

    python -m pyhillfit_amd.PyHillFit --data-file ../data/crumb_data.csv -m 2 -a [--hierarchical]
           [-i 500000] [-t 5] [-b 4] [-c N] [-Ne 0] [--num-APs 500] [-bfo]
           [--num-chains 64 | 128 with --hierarchical] [--seed 25] [--device cuda:0] [--save-all-chains] [--segment 20000]
           [--diagnostics [--diagnostic-lags 256] [--diagnostic-batch-means]] [--waic] [--loo [--loo-tail-per-chain 0]]
           [--quantiles [--quantile-probs 0.025,...,0.975] [--quantile-bins 16384] [--curve-bands G]] [--ppc]
           [--hierarchical --quantiles --predictive-bands G [--band-concs c1,c2,...]]
           [--hierarchical --leave-experiment-out [--marginal-nodes 128] [--marginal-every T]]
           [--sensitivity [--sensitivity-delta 0.01] [--sensitivity-bins 4096] [--sensitivity-threshold 0.05]]
           [--hierarchical --de-every K [--de-population 64] [--de-gamma GAMMA] [--de-jump-every 10]]
           [--next-dose G [--next-dose-concs c1,c2,...] [--next-dose-bins 256] [--next-dose-every 17]] [--correlations]
           [-m 2 --savage-dickey [--savage-dickey-panels 32] [--savage-dickey-every 11]]
           [--drug-profile-concs c1,c2,... | --drug-profile-cmax FILE [--drug-profile-multiples 1,3,10]] [--drug-profile-weights name=w,...]
           [--drug-profile-bins 4096]

Same command-line flags, same output files in the same places (python/PyHillFit.py:33-65,645-971; chain-file
contract: doseresponse.py:70-82,115-128), but every selected (drug, channel) pair is sampled AT ONCE by the HIP
kernels, `--num-chains` independent chains per pair.  What lands in the reference's chain file is chain 0 of the
pair (burn-in removed exactly like PyHillFit.py:861-864); with --save-all-chains every chain is also written to
`<chain file minus .txt>_all_chains.npy` ([rows][d+1][chains]); posterior moments of all chains, accumulated on the
device, go to `<...>_summary.json`; with --diagnostics, also split-R-hat / ESS / MCSE of every column over all chains
(pyhillfit_amd/diagnostics.py), accumulated on the device segment by segment; with --waic, WAIC and the pointwise predictive
accuracy of every data point over all chains (pyhillfit_amd/waic.py), accumulated the same way; with --loo, PSIS-LOO and the Pareto
k-hat of every data point (pyhillfit_amd/loo.py), accumulated the same way; with --quantiles, posterior quantiles and 90 / 95 %
credible intervals of every column over all chains (pyhillfit_amd/quantiles.py), and with --curve-bands G the same of the
dose-response curve at G doses, accumulated the same way; with --ppc, posterior predictive checks (test quantities of replicated
data against the data, and the predictive PIT of every data point; pyhillfit_amd/ppc.py), accumulated the same way; with
--hierarchical --quantiles --predictive-bands G, the quantiles of the dose-response curve of the inferred underlying effect and of a
predicted future experiment at G doses (and at the named --band-concs), accumulated the same way; with --hierarchical
--leave-experiment-out, the integrated leave-one-experiment-out cross-validation of every pair (pyhillfit_amd/marginal.py: each experiment's
(Hill_i, pIC50_i) integrated out on the GPU, PSIS and WAIC over the experiments), written to the summary JSON as "loo_experiment"; with
--sensitivity, the power-scaling sensitivity of every parameter column to the prior and to the likelihood (pyhillfit_amd/sensitivity.py),
accumulated the same way and written to the summary JSON as "sensitivity"; with --next-dose G (single-level), the expected information
gain of one further measurement at G candidate doses (pyhillfit_amd/design.py), accumulated the same way and written as "next_dose"; with --correlations, the posterior and within-chain correlation matrices of the
parameter columns and the multivariate R-hat with the direction along which the chains sit apart (pyhillfit_amd/correlations.py),
accumulated the same way and written as "correlations"; with -m 2 --savage-dickey, the Bayes factor B12 of Hill = 1 against Hill free by
the Savage-Dickey density ratio from this run's draws alone (pyhillfit_amd/savage_dickey.py), accumulated the same way and written as
"bayes_factor"; with --drug-profile-concs or --drug-profile-cmax (single-level), the joint multi-channel block of every drug at the given
concentrations — per channel and as a weighted net block, with the probability that the net block is positive and of each channel being
the most blocked one (pyhillfit_amd/drug_profile.py) — accumulated the same way and written to one
`<drug>/drug_profiles/<drug>_drug_profile.json` per drug.  The CMA-ES start point is replaced by a deterministic least-squares fit
(bestfit.py); figures are not produced (plotting is outside the sampling step).

Multi-GPU: `-c/--num-cores N` — the reference's pool size (python/PyHillFit.py:40,997-1003) — starts min(N, visible GPUs) ranks,
one per GPU (this process runs `torch.distributed.run` as a child before it touches a GPU and passes the exit code on); or
launch under torchrun yourself.  Pairs are partitioned over the ranks by cost, each rank writes the files of its pairs, rank 0
reads the data file and broadcasts it first and gathers the summaries at the end (RCCL)."""
import argparse
import itertools as it
import json
import sys
import time

import numpy as np

from . import bestfit, chainio
from . import distributed as phfdist
from . import doseresponse as dr


QUANTILE_PROBS = (0.025, 0.05, 0.25, 0.5, 0.75, 0.95, 0.975)


def _probs(text):
    from .quantiles import parse_probs
    try:
        return parse_probs(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def _bins(text):
    b = int(text)
    if b < 64 or b > 32768 or b & (b - 1):
        raise argparse.ArgumentTypeError("must be a power of two in [64, 32768], got %d" % b)
    return b


def check_args(parser, args):
    """refusals that need no GPU"""
    if isinstance(args.quantile_probs, str):
        args.quantile_probs = _probs(args.quantile_probs)
    if args.curve_bands < 0:
        parser.error("--curve-bands must be >= 0")
    if args.curve_bands and args.hierarchical:
        parser.error("--curve-bands is single-level only (no bands for the hierarchical model)")
    if args.curve_bands and not args.quantiles:
        parser.error("--curve-bands needs --quantiles")
    if args.predictive_bands < 0:
        parser.error("--predictive-bands must be >= 1")
    if args.predictive_bands and not args.hierarchical:
        parser.error("--predictive-bands needs --hierarchical (single-level: --curve-bands)")
    if args.predictive_bands and not args.quantiles:
        parser.error("--predictive-bands needs --quantiles")
    if args.band_concs is not None:
        from .quantiles import parse_band_concs
        if isinstance(args.band_concs, str):
            try:
                args.band_concs = parse_band_concs(args.band_concs)
            except ValueError as e:
                parser.error(str(e))
        if not args.predictive_bands:
            parser.error("--band-concs needs --predictive-bands")
    if getattr(args, "diagnostic_batch_means", False) and not args.diagnostics:
        parser.error("--diagnostic-batch-means needs --diagnostics")
    sens_given = [n for n in ("sensitivity_delta", "sensitivity_bins", "sensitivity_threshold") if getattr(args, n, None) is not None]
    if sens_given and not getattr(args, "sensitivity", False):
        parser.error("--%s needs --sensitivity" % sens_given[0].replace("_", "-"))
    if getattr(args, "sensitivity", False):
        from . import sensitivity as sn
        try:
            args.sensitivity_delta = sn.check_delta(sn.DEFAULT_DELTA if args.sensitivity_delta is None else args.sensitivity_delta)
            args.sensitivity_bins = sn.check_bins(sn.DEFAULT_BINS if args.sensitivity_bins is None else args.sensitivity_bins)
            args.sensitivity_threshold = sn.check_threshold(sn.DEFAULT_THRESHOLD if args.sensitivity_threshold is None
                                                            else args.sensitivity_threshold)
        except ValueError as e:
            parser.error(str(e))
    if args.leave_experiment_out and not args.hierarchical:
        parser.error("--leave-experiment-out needs --hierarchical (there are no experiment-level parameters to integrate out otherwise)")
    if (args.marginal_nodes is not None or args.marginal_every is not None) and not args.leave_experiment_out:
        parser.error("--marginal-nodes and --marginal-every need --leave-experiment-out")
    if args.leave_experiment_out:
        from .marginal import DEFAULT_EVERY, DEFAULT_NODES, NODE_CHOICES
        args.marginal_nodes = DEFAULT_NODES if args.marginal_nodes is None else args.marginal_nodes
        args.marginal_every = DEFAULT_EVERY if args.marginal_every is None else args.marginal_every
        if args.marginal_nodes not in NODE_CHOICES:
            parser.error("--marginal-nodes must be one of %s" % ", ".join(str(q) for q in NODE_CHOICES))
        if args.marginal_every < 1:
            parser.error("--marginal-every must be >= 1")
    if args.next_dose < 0:
        parser.error("--next-dose must be >= 1 (0 = off)")
    nd_given = [n for n in ("next_dose_concs", "next_dose_bins", "next_dose_every") if getattr(args, n, None) is not None]
    if nd_given and not args.next_dose:
        parser.error("--%s needs --next-dose" % nd_given[0].replace("_", "-"))
    if args.next_dose and args.hierarchical:
        parser.error("--next-dose is single-level only: the information of a new experiment under the population model of --hierarchical "
                     "is a different integral")
    if args.next_dose:
        from . import design as ds
        try:
            if isinstance(args.next_dose_concs, str):
                args.next_dose_concs = ds.parse_concs(args.next_dose_concs)
            args.next_dose_bins = ds.check_bins(ds.DEFAULT_BINS if args.next_dose_bins is None else args.next_dose_bins)
        except ValueError as e:
            parser.error(str(e))
        args.next_dose_every = ds.DEFAULT_EVERY if args.next_dose_every is None else args.next_dose_every
        if args.next_dose_every < 1:
            parser.error("--next-dose-every must be >= 1")
    sd_given = [n for n in ("savage_dickey_panels", "savage_dickey_every") if getattr(args, n, None) is not None]
    if sd_given and not args.savage_dickey:
        parser.error("--%s needs --savage-dickey" % sd_given[0].replace("_", "-"))
    if args.savage_dickey:
        if args.hierarchical:
            parser.error("--savage-dickey is single-level only: the hierarchical model has no Hill = 1 sub-model with nested priors")
        if args.model != 2:
            parser.error("--savage-dickey needs -m 2: B12 is read off the Hill-free fit (model 1 is model 2 at Hill = 1)")
        from . import savage_dickey as sd
        try:
            args.savage_dickey_panels = sd.check_panels(sd.DEFAULT_PANELS if args.savage_dickey_panels is None else args.savage_dickey_panels)
        except ValueError as e:
            parser.error(str(e))
        args.savage_dickey_every = sd.DEFAULT_EVERY if args.savage_dickey_every is None else args.savage_dickey_every
        if args.savage_dickey_every < 1:
            parser.error("--savage-dickey-every must be >= 1")
    check_drug_profile_args(parser, args)
    de_given = [n for n in ("de_population", "de_gamma", "de_jump_every") if getattr(args, n, None) is not None]
    if args.de_every < 0:
        parser.error("--de-every must be >= 0 (0 = no differential-evolution moves)")
    if args.de_every and not args.hierarchical:
        parser.error("--de-every needs --hierarchical (the moves are between the chains of the hierarchical sampler; PyHillTemp has --swap-every)")
    if de_given and not args.de_every:
        parser.error("--%s needs --de-every" % de_given[0].replace("_", "-"))
    if args.de_every:
        from . import de_moves as de
        args.de_population = de.DEFAULT_POPULATION if args.de_population is None else args.de_population
        args.de_jump_every = de.DEFAULT_JUMP_EVERY if args.de_jump_every is None else args.de_jump_every
        chains = DEFAULT_CHAINS_HIERARCHICAL if args.num_chains is None else args.num_chains
        try:
            de.check_settings(args.de_every, args.thinning, args.de_population, chains, args.de_gamma, args.de_jump_every)
        except ValueError as e:
            parser.error("--de-every / --de-population / --de-gamma / --de-jump-every: " + str(e))


def check_drug_profile_args(parser, args):
    """the --drug-profile-* flags: args.drug_profile says whether the analysis is on; the values are parsed in place"""
    from . import drug_profile as dp
    args.drug_profile = args.drug_profile_concs is not None or args.drug_profile_cmax is not None
    given = [n for n in ("drug_profile_multiples", "drug_profile_weights", "drug_profile_bins") if getattr(args, n) is not None]
    if given and not args.drug_profile:
        parser.error("--%s needs --drug-profile-concs or --drug-profile-cmax" % given[0].replace("_", "-"))
    if not args.drug_profile:
        return
    if args.hierarchical:
        parser.error("--drug-profile-concs / --drug-profile-cmax are single-level only: a drug's pairs fall into different launch groups of "
                     "the hierarchical sampler; profile hierarchical chain files with `python -m pyhillfit_amd.drug_profile --hierarchical`")
    if args.drug_profile_multiples is not None and args.drug_profile_cmax is None:
        parser.error("--drug-profile-multiples needs --drug-profile-cmax (the multiples are of Cmax)")
    try:
        if isinstance(args.drug_profile_concs, str):
            args.drug_profile_concs = dp.parse_concs(args.drug_profile_concs)
        args.drug_profile_multiples = (dp.DEFAULT_MULTIPLES if args.drug_profile_multiples is None else
                                       dp.parse_multiples(args.drug_profile_multiples))
        if isinstance(args.drug_profile_cmax, str):
            args.drug_profile_cmax = dp.read_cmax(args.drug_profile_cmax)
        if isinstance(args.drug_profile_weights, str):
            args.drug_profile_weights = dp.parse_weights(args.drug_profile_weights)
        args.drug_profile_bins = dp.check_bins(dp.DEFAULT_BINS if args.drug_profile_bins is None else args.drug_profile_bins)
        doses = len(args.drug_profile_concs or ()) + (len(args.drug_profile_multiples) if args.drug_profile_cmax is not None else 0)
        if doses > dp.MAX_DOSES:
            raise ValueError("at most %d doses per drug (--drug-profile-concs and --drug-profile-multiples together), got %d"
                             % (dp.MAX_DOSES, doses))
    except (ValueError, OSError) as e:
        parser.error(str(e))


def build_parser():
    parser = argparse.ArgumentParser(prog="PyHillFit.py")
    # flags of the reference, python/PyHillFit.py:35-48
    parser.add_argument("-i", "--iterations", type=int, help="number of MCMC iterations", default=500000)
    parser.add_argument("-t", "--thinning", type=int, help="how often to thin the MCMC, i.e. save every t-th iteration", default=5)
    parser.add_argument("-b", "--burn-in-fraction", type=int, help="given N saved MCMC iterations, discard the first N/b as burn-in", default=4)
    parser.add_argument("-a", "--all", action='store_true', help='run MCMC on all drugs and channels', default=False)
    parser.add_argument('-ppp', '--plot-parameter-paths', action='store_true', help='accepted, ignored (no figures)', default=False)
    parser.add_argument("-c", "--num-cores", type=int, help="number of cores to parallelise drug/channel combinations: here GPUs — N > 1 starts min(N, visible GPUs) ranks, one per GPU", default=1)
    parser.add_argument("-Ne", "--num-expts", type=int, help="how many experiments to fit to", default=0)
    parser.add_argument("--num-APs", type=int, help="how many (alpha,mu) samples to take for AP simulations", default=500)
    parser.add_argument("--hierarchical", action='store_true', help="run hierarchical MCMC algorithm", default=False)
    parser.add_argument("-bfo", "--best-fit-only", action='store_true', help="only do the best fit, then quit", default=False)
    req = parser.add_argument_group('required arguments')
    req.add_argument("--data-file", type=str, help="csv file in the format of crumb_data.csv", required=True)
    req.add_argument("-m", "--model", type=int, help="For non-hierarchical: 1. fix Hill=1; 2. vary Hill", required=True)
    # new, GPU-side options (defaults keep old command lines working)
    new = parser.add_argument_group('MI355X options')
    new.add_argument("--num-chains", type=int, default=None, help="independent chains per (drug, channel) pair (default: 64; --hierarchical: 128 — "
                     "measured on the full Crumb set, 128 chains per pair take the wall time of 64: 6.24 s against 6.21, the run being the latency of "
                     "one wavefront-iteration on a chip the 420 wavefronts of 64 chains leave 59 %% idle; profiles/r05/cli_host_profile_hierarchical.txt)")
    new.add_argument("--seed", type=int, default=25, help="Philox seed (the reference seeds numpy with 25)")
    new.add_argument("--device", type=str, default=None, help="HIP device, default cuda:<LOCAL_RANK>")
    new.add_argument("--predictive-cdfs", action='store_true', default=False, help="hierarchical: also write the posterior-predictive CDFs and (Hill,pIC50) samples of construct_hierarchical_cdfs.py, accumulated on the GPU during sampling")
    new.add_argument("--cdf-chains", type=int, default=0, help="chains per pair feeding --predictive-cdfs (0 = all; 1 = chain 0 only, what the reference's script computes from the chain file)")
    new.add_argument("--write-workers", type=int, default=None, help="processes formatting the chain text files (default: this rank's host cores - 1, at most 16; 0 = write in the main process)")
    new.add_argument("--save-all-chains", action='store_true', default=False, help="also write every chain to a .npy next to the chain file")
    new.add_argument("--segment", type=int, default=20000, help="MH iterations per kernel launch")
    new.add_argument("--diagnostics", action='store_true', default=False, help="split-R-hat, multi-chain ESS and MCSE of every column over all chains, "
                     "accumulated on the GPU while the rows stream past; written to the summary JSON as \"diagnostics\"")
    new.add_argument("--diagnostic-lags", type=int, default=256, help="lag limit K of the autocorrelation sums of --diagnostics")
    new.add_argument("--diagnostic-batch-means", action='store_true', default=False, help="--diagnostics: also ESS and MCSE by batch means on a "
                     "dyadic ladder of batch sizes, for columns whose autocorrelation time exceeds --diagnostic-lags; written to the summary "
                     "JSON as \"batch_means\" inside \"diagnostics\"")
    new.add_argument("--waic", action='store_true', default=False, help="WAIC, p_waic and the pointwise elpd of every data point over all "
                     "chains' post-burn-in draws, accumulated on the GPU while the rows stream past; written to the summary JSON as \"waic\"")
    new.add_argument("--loo", action='store_true', default=False, help="PSIS-LOO: elpd_loo, p_loo and the Pareto k-hat of every data point over "
                     "all chains' post-burn-in draws, accumulated on the GPU while the rows stream past; written to the summary JSON as \"loo\"")
    new.add_argument("--loo-tail-per-chain", type=int, default=0, help="--loo: smallest log-likelihoods kept per (point, chain); 0: "
                     "M + 1 for the tail length M (every point exact) while the workspace fits 32 GiB, else 2 ceil((M + 1)/chains) + 32.  "
                     "Raise it if points are reported undetermined")
    new.add_argument("--quantiles", action='store_true', default=False, help="posterior quantiles of every column over all chains' "
                     "post-burn-in draws (each reported with the bracket that holds the exact sample quantile) and the central 90 %% and "
                     "95 %% credible intervals, from histograms accumulated on the GPU while the rows stream past; written to the summary "
                     "JSON as \"quantiles\"")
    new.add_argument("--quantile-probs", type=_probs, default=",".join(str(p) for p in QUANTILE_PROBS),
                     help="--quantiles: the probabilities, comma-separated")
    new.add_argument("--quantile-bins", type=_bins, default=16384, help="--quantiles: histogram bins per column, a power of two")
    new.add_argument("--curve-bands", type=int, default=0, metavar="G", help="--quantiles, single-level only: also the quantiles of the "
                     "dose-response curve at G doses log-spaced from the pair's smallest dose / 10 to its largest x 10; written to the "
                     "summary JSON as \"curve_band\"")
    new.add_argument("--predictive-bands", type=int, default=0, metavar="G", help="--hierarchical --quantiles: the quantiles of the "
                     "dose-response curve of the inferred underlying effect (Hill = alpha, pIC50 = mu) and of a predicted future experiment "
                     "(Hill ~ log-logistic(alpha, beta), pIC50 ~ logistic(mu, s), one replicate per draw) at G doses log-spaced from the "
                     "pair's smallest dose / 10 to its largest x 10; written to the summary JSON as \"hierarchical_bands\"")
    new.add_argument("--band-concs", type=str, default=None, metavar="c1,c2,...", help="--predictive-bands: named concentrations (uM, "
                     "all > 0, at most 64) appended after the grid (the reference's -c/--concs)")
    new.add_argument("--leave-experiment-out", action='store_true', default=False, help="--hierarchical: integrated leave-one-experiment-out "
                     "cross-validation: every experiment's (Hill_i, pIC50_i) integrated out against the population distribution of each "
                     "draw on the GPU, then PSIS and WAIC over the experiments; written to the summary JSON as \"loo_experiment\"")
    new.add_argument("--marginal-nodes", type=int, default=None, metavar="Q", help="--leave-experiment-out: nodes a side of the Q x Q rule, "
                     "32, 64, 128 (default) or 256; raise it when the report names experiments with a quadrature gap above 0.01")
    new.add_argument("--marginal-every", type=int, default=None, metavar="T", help="--leave-experiment-out: every T-th post-burn-in row "
                     "of every chain is used (default 178: on the whole Crumb set at the default chains and Q = 128 the flag then adds no more than "
                     "the sampling time; the cost is proportional to Q^2 / T)")
    new.add_argument("--ppc", action='store_true', default=False, help="posterior predictive checks: mid-p values of the deviance, mean, sd "
                     "and counts of 0 and 100 of data replicated from every post-burn-in draw of every chain against the data's, and the "
                     "predictive PIT of every data point, accumulated on the GPU while the rows stream past; written to the summary JSON as \"ppc\"")
    new.add_argument("--sensitivity", action='store_true', default=False, help="power-scaling sensitivity (Kallioinen et al. 2023): how far every "
                     "parameter's posterior moves when the prior, or the likelihood, is raised to a power a little off 1, from re-weighted "
                     "histograms accumulated on the GPU while the rows stream past; written to the summary JSON as \"sensitivity\"")
    new.add_argument("--sensitivity-delta", type=float, default=None, metavar="DELTA", help="--sensitivity: the powers are 1/(1 + DELTA) and "
                     "1 + DELTA; 0 < DELTA <= 0.25 (default 0.01)")
    new.add_argument("--sensitivity-bins", type=int, default=None, metavar="B", help="--sensitivity: histogram bins per column, a power of two "
                     "in [64, 4096] (default 4096)")
    new.add_argument("--sensitivity-threshold", type=float, default=None, metavar="TAU", help="--sensitivity: a column is flagged when its "
                     "sensitivity D exceeds TAU (default 0.05)")
    new.add_argument("--next-dose", type=int, default=0, metavar="G", help="single-level: at which concentration should the next measurement be "
                     "taken?  The expected information gain (nats) of ONE further measurement, recorded to 100/K %% block, at G doses "
                     "log-spaced from the pair's smallest dose / 10 to its largest x 10 (and at the named --next-dose-concs), accumulated on "
                     "the GPU while the rows stream past; a lower bound of the continuous value that rises with K; written to the summary "
                     "JSON as \"next_dose\"")
    new.add_argument("--next-dose-concs", type=str, default=None, metavar="C1,C2,...", help="--next-dose: further candidate doses in uM")
    new.add_argument("--next-dose-bins", type=int, default=None, metavar="K", help="--next-dose: bins of (0, 100) the new response is recorded "
                     "to, 128, 256 (default), 512 or 1024")
    new.add_argument("--next-dose-every", type=int, default=None, metavar="T", help="--next-dose: every T-th post-burn-in row of every chain is "
                     "used (default 17: on the whole Crumb set at the default chains, G = 16 and K = 256 the flag then adds no more than the "
                     "sampling time; the cost is proportional to G K / T)")
    new.add_argument("--correlations", action='store_true', default=False, help="the posterior correlation matrix of the parameter columns "
                     "over all chains, the within-chain correlation matrix and its principal axes, and the multivariate R-hat (Brooks & Gelman "
                     "1998, in the convention of the split-R-hat) with the linear combination of the parameters along which the chains "
                     "disagree most, from co-moments accumulated on the GPU while the rows stream past; written to the summary JSON as "
                     "\"correlations\"")
    new.add_argument("--savage-dickey", action='store_true', default=False, help="-m 2 only: the Bayes factor B12 of Hill = 1 (model 1) against "
                     "Hill free (model 2) by the Savage-Dickey density ratio, from this run's draws alone (no tempered ladder, no model-1 "
                     "fit): the mean over the draws of L(Hill = 1) / mean over Hill's prior of L, the latter by Gauss-Kronrod quadrature "
                     "on the GPU while the rows stream past; valid for the nested priors of models 1 and 2 only; written to the summary "
                     "JSON as \"bayes_factor\"")
    new.add_argument("--savage-dickey-panels", type=int, default=None, metavar="P", help="--savage-dickey: equal panels of [0, 10], each with "
                     "the 15-point Gauss-Kronrod rule: 16, 32 (default) or 64; raise it when pairs are reported with a quadrature gap")
    new.add_argument("--savage-dickey-every", type=int, default=None, metavar="T", help="--savage-dickey: every T-th post-burn-in row of every "
                     "chain is used (default 11: on the whole Crumb set at the default chains and P = 32 the flag then adds no more than the "
                     "sampling time; the cost grows with P / T)")
    new.add_argument("--drug-profile-concs", type=str, default=None, metavar="c1,c2,...", help="single-level: the drug profile at these "
                     "concentrations (uM, the same for every drug): per post-burn-in draw of all the channels of a drug side by side, the "
                     "percent block of every channel, their weighted net block and the most blocked channel; quantiles at the "
                     "--quantile-probs, the probability of a positive net block and of each channel being the most blocked, from "
                     "histograms and integer counts accumulated on the GPU while the rows stream past; written to one "
                     "<drug>/drug_profiles/<drug>_drug_profile.json per drug.  Not an action-potential prediction, not a risk category")
    new.add_argument("--drug-profile-cmax", type=str, default=None, metavar="FILE", help="single-level: the drug profile at multiples of "
                     "each drug's clinical concentration; FILE as the reference's chaste/drug_list.txt: a header line, then `Drug "
                     "EFTPCmax(nM) [anything]`; a drug the file does not name is skipped unless --drug-profile-concs is given too")
    new.add_argument("--drug-profile-multiples", type=str, default=None, metavar="m1,...", help="--drug-profile-cmax: the multiples of "
                     "Cmax (default 1,3,10: a convention)")
    new.add_argument("--drug-profile-weights", type=str, default=None, metavar="name=w,...", help="the drug profile's weights of the net "
                     "block by channel name, overriding the defaults: +1 hERG, KvLQT1_mink, Kv4.3, Kir2.1, -1 Nav1.5-peak, Nav1.5-late, "
                     "Cav1.2, 0 any other name — a convention (repolarising minus depolarising block), not a measurement")
    new.add_argument("--drug-profile-bins", type=int, default=None, metavar="B", help="the drug profile's histogram bins per channel and "
                     "dose, a power of two in [64, 32768] (default 4096)")
    new.add_argument("--de-every", type=int, default=0, metavar="K", help="--hierarchical: differential-evolution moves between the chains of "
                     "each pair (ter Braak 2006) after every K iterations, K a multiple of the thinning (default 0 = off: every output as "
                     "without the flag); the chains of one population are then coupled; written to the summary JSON as \"de_moves\"")
    new.add_argument("--de-population", type=int, default=None, metavar="G", help="--de-every: chains per population, 4, 8, 16, 32 or 64 "
                     "(default 64); must divide --num-chains")
    new.add_argument("--de-gamma", type=float, default=None, metavar="GAMMA", help="--de-every: the step factor (default 2.38 / sqrt(2 dim), "
                     "dim = 5 + 2 experiments)")
    new.add_argument("--de-jump-every", type=int, default=None, metavar="J", help="--de-every: every J-th round uses gamma = 1, a jump "
                     "between modes (default 10; 0 = never)")
    new.add_argument("--fused-launch", choices=["auto", "on", "off"], default="auto",
                     help="--hierarchical: the launch groups the gfx950 code object has kernels for (Ne = 3; Ne = 4 with 4 + 4 + 4 + 1 / 2 / 3 points) through "
                          "ONE persistent grid per segment instead of a launch each (auto: when the run's chains give every SIMD a wavefront); same numbers")
    new.add_argument("--output-root", type=str, default="output", help="root of the output tree (reference: ./output)")
    new.add_argument("--drugs", type=str, default=None, help="comma-separated drug names instead of -a / the menu")
    new.add_argument("--channels", type=str, default=None, help="comma-separated channel names instead of -a / the menu")
    return parser


def select_pairs(args):
    if args.drugs or args.channels:
        drugs = args.drugs.split(",") if args.drugs else list(dr.drugs)
        channels = args.channels.split(",") if args.channels else list(dr.channels)
    else:
        drugs, channels = dr.list_drug_channel_options(args.all)      # PyHillFit.py:65
    return list(it.product(drugs, channels))                          # PyHillFit.py:978


def load_single_level_pairs(pairs):
    """PyHillFit.py:653-669: skip pairs without data or with missing responses."""
    out = []
    for drug, channel in pairs:
        try:
            num_expts, _, experiments = dr.load_crumb_data(drug, channel)
            concs, responses = dr.concatenate_experiments(num_expts, experiments)
        except Exception:
            print("Problem loading data, guessing there are no entries for {} + {} --- skipping".format(drug, channel))
            continue
        if np.any(np.isnan(responses)):
            print("Skipping {} because of empty responses / missing data".format((drug, channel)))
            continue
        out.append((drug, channel, concs, responses))
    return out


def run_single_level(pairs, args, device, rank=0, world=1):
    """All pairs of this rank at once — replaces python/PyHillFit.py:645-971 run per pair."""
    import torch
    from . import analyses as an
    from .sampler import SingleLevelSampler
    from .waic import Points
    model, temperature = args.model, 1                                 # PyHillFit.py:57
    t_begin = time.time()
    loaded = load_single_level_pairs(pairs)
    if not loaded:
        return []
    # ---- start points + best-fit files (PyHillFit.py:699-746) ----
    writers = chainio.WriterPool(args.write_workers)                   # one pool for the start-point fits and the file formatting
    fit_theta, fit_ss = bestfit.best_fit_batch([(concs, responses) for _, _, concs, responses in loaded], model)   # all pairs at once
    theta0, files = [], []
    for (drug, channel, concs, responses), th0, ss in zip(loaded, fit_theta, fit_ss):
        d_clean, c_clean, chain_file, images_dir = dr.nonhierarchical_chain_file_and_figs_dir(model, drug, channel, temperature)
        chainio.save_best_fit_params(images_dir + "{}_{}_best_fit_params.txt".format(d_clean, c_clean), th0, model)
        start0 = bestfit.chain_start(th0, model)                       # the fit, with a Hill coefficient above the prior's bound moved onto it
        if not np.array_equal(start0, th0):
            print("{} + {}: least-squares Hill {:.3g} is outside the prior's support; chains start at Hill = {:g}".format(drug, channel, th0[1], start0[1]))
        theta0.append(start0); files.append((d_clean, c_clean, chain_file))
    if args.best_fit_only:
        writers.close()
        return []
    total_iterations, thinning = args.iterations, args.thinning
    assert total_iterations % thinning == 0                            # PyHillFit.py:805
    packed = dr.PackedPoints([(c, y) for _, _, c, y in loaded])
    Q, C = len(loaded), args.num_chains
    problem_ids = [p[4] for p in pairs_with_ids(pairs, loaded)]
    s = SingleLevelSampler(packed, model, list(range(Q)), [1.0] * Q, C, thinning=thinning, seed=args.seed,
                           adapt_start=1000 * dr.num_params, problem_ids=problem_ids, device=device)
    s.init(np.array(theta0), cov_identity=False, cov_scale=0.05)       # PyHillFit.py:748-751
    saved_iterations = total_iterations // thinning + 1                # :810
    burn = saved_iterations // args.burn_in_fraction                   # :862
    s.enable_moments(after_iteration=max(burn * thinning - 1, 0))      # moments over exactly the rows that are written
    s.reserve(total_iterations)
    keep_all = args.save_all_chains
    if keep_all:                                                       # every saved row of every chain stays in HBM until it is written
        need = saved_iterations * Q * (s.d + 1) * C * 8
        free = torch.cuda.mem_get_info(device)[0]
        if need > 0.8 * free:
            raise SystemExit("--save-all-chains needs {:.1f} GB of device memory for {} pairs x {} chains x {} saved rows, {:.1f} GB are free: "
                             "select fewer pairs (--drugs/--channels), fewer chains or a larger thinning".format(need / 1e9, Q, C, saved_iterations, free / 1e9))
    d = s.d
    columns = dr.file_labels + ["log-target"]
    kinds = an.fit_analyses(args)
    aset = an.AnalysisSet(kinds, an.Run(
        args=args, kind=model, Q=Q, C=C, cols=d + 1, columns=columns, saved=saved_iterations, burn=burn, device=device,
        sampler_points=s.points, concs=[concs for _, _, concs, _ in loaded], seed=args.seed, problem_ids=problem_ids, prior=None, de=None,
        pairs=[(drug, channel) for drug, channel, _, _ in loaded],
        make_points=lambda: Points.single_level(*zip(*[experiments_and_labels(drug, channel) for drug, channel, _, _ in loaded]))))
    aset.feed_start(s.row0)
    kept = (torch.empty((saved_iterations, Q, d + 1, C), dtype=torch.float64, device=device) if keep_all else
            chainio.host_buffer((saved_iterations, Q, d + 1, 1)))   # pinned: chain 0 leaves the GPU asynchronously
    kept[0] = s.row0 if keep_all else s.row0[:, :, :1].cpu()
    seg = max(thinning, args.segment - args.segment % thinning)
    buf = torch.empty((seg // thinning, Q, d + 1, C), dtype=torch.float64, device=device)
    done, r = 0, 1
    torch.cuda.synchronize(device)
    start = time.time()
    while done < total_iterations:
        k = min(seg, total_iterations - done)
        nr = k // thinning
        rows = s.advance(k, out=buf[:nr])
        aset.feed(rows, r, nr)                                         # saved rows before `burn` are the burn-in
        # stream-ordered and asynchronous: the next segment is queued behind this copy while the host moves on (a blocking copy
        # here left the GPU idle for the gather + transfer + launch latency of every segment)
        kept[r:r + nr].copy_(rows if keep_all else rows[:, :, :, :1], non_blocking=True)
        done += k; r += nr
    torch.cuda.synchronize(device)
    elapsed = time.time() - start
    mean, var, n_mom = s.posterior_moments()
    mean, var = mean.cpu().numpy(), var.cpu().numpy()
    acc = s.acceptance().cpu().numpy()
    aset.finish()
    summaries = []
    for q, (d_clean, c_clean, chain_file) in enumerate(files):
        chain0 = kept[:, q, :, 0].cpu().numpy()
        writers.submit(chainio.save_single_level_chain, chain_file, chainio.drop_burn_in(chain0, args.burn_in_fraction), d_clean, c_clean, model)
        if keep_all:
            np.save(chain_file[:-4] + "_all_chains.npy", chainio.drop_burn_in(kept[:, q].cpu().numpy(), args.burn_in_fraction))   # binary: no formatting to spread
        pooled_mean = mean[:, q].mean(axis=1)
        pooled_sd = np.sqrt(var[:, q].mean(axis=1) + mean[:, q].var(axis=1))
        summ = {"drug": d_clean, "channel": c_clean, "model": model, "chains": C, "iterations": total_iterations,
                "thinning": thinning, "saved_rows_after_burn_in": int(saved_iterations - burn),
                "columns": columns, "pooled_mean": pooled_mean.tolist(), "pooled_sd": pooled_sd.tolist(),
                "per_chain_mean_sd": mean[:, q].std(axis=1).tolist(), "acceptance": float(acc[q].mean()),
                "start_point": np.asarray(theta0[q]).tolist(), "seed": args.seed,
                "mh_samples_per_second": Q * C * total_iterations / elapsed}
        aset.record(summ, q)
        with open(chain_file[:-4] + "_summary.json", "w") as f:
            json.dump(summ, f, indent=1)
        summaries.append(summ)
        print("\n\n{} + {} complete!\n\n".format(d_clean, c_clean))      # PyHillFit.py:970
    writers.close()
    for line in an.report(kinds, [aset], rank, ["{} + {}".format(f[0], f[1]) for f in files], args):
        print(line)
    print("timing [rank {}]: data + start points {:.1f} s, sampling {:.1f} s ({} chains x {} iterations), chain files {:.1f} s".format(
        rank, start - t_begin, elapsed, Q * C, total_iterations, time.time() - start - elapsed))
    return summaries


def experiments_and_labels(drug, channel, num_expts=None):
    """the experiments the sampler concatenates for a pair (PyHillFit.py:661-665; the first num_expts of them if given) and their
    labels in the data file"""
    n, numbers, experiments = dr.load_crumb_data(drug, channel)
    n = n if num_expts is None else num_expts
    return list(experiments[:n]), [int(e) + 1 for e in numbers[:n]]


def pairs_with_ids(all_pairs, loaded):
    """global problem number of every loaded pair = its index in the full drug x channel product of the data file
    (so a pair's Philox streams do not depend on which other pairs were selected or on the rank layout)"""
    index = {(d, c): i for i, (d, c) in enumerate(it.product(dr.drugs, dr.channels))}
    return [(d, c, cc, y, index.get((d, c), 0)) for d, c, cc, y in loaded]


def main(argv=None):
    parser = build_parser()
    if argv is None and len(sys.argv) == 1:
        parser.print_help()
        sys.exit(1)
    args = parser.parse_args(argv)
    check_args(parser, args)
    n = phfdist.ranks_for_cores(args.num_cores)                        # -c N: the reference's pool (PyHillFit.py:997-1003) -> N ranks
    if n:
        sys.exit(phfdist.spawn_ranks("pyhillfit_amd.PyHillFit", sys.argv[1:] if argv is None else argv, n))
    rank, local_rank, world = phfdist.init()
    try:
        return _run(args, rank, local_rank, world)
    finally:
        phfdist.finalize()       # also on an error or SystemExit of this rank: the others' next collective fails instead of hanging


DEFAULT_CHAINS, DEFAULT_CHAINS_HIERARCHICAL = 64, 128


def _run(args, rank, local_rank, world):
    device = args.device or "cuda:%d" % local_rank
    if args.num_chains is None:
        args.num_chains = DEFAULT_CHAINS_HIERARCHICAL if args.hierarchical else DEFAULT_CHAINS
    if args.write_workers is None:
        args.write_workers = chainio.default_write_workers(world)
    dr.define_model(args.model)                                        # PyHillFit.py:56
    phfdist.setup_data_file(args.data_file)                            # :61 (rank 0 reads, broadcast to the other GPUs' ranks)
    dr.output_root = args.output_root
    pairs = select_pairs(args)
    if world > 1:                                                      # partition pairs over the GPUs of the node
        costs = []
        for d, c in pairs:
            try:
                costs.append(sum(len(e) for e in dr.load_crumb_data(d, c)[2]))
            except Exception:
                costs.append(0)
        if getattr(args, "drug_profile", False):                       # a drug's channels are paired row by row: whole drugs to a rank
            mine = phfdist.shard_drugs(costs, [d for d, _ in pairs], world)[rank]
        else:
            mine = phfdist.shard_problems(costs, world)[rank]
        pairs = [pairs[i] for i in mine]
    if args.hierarchical:
        from .hierarchical import run_hierarchical
        summaries = run_hierarchical(pairs, args, device, rank, world)
    else:
        summaries = run_single_level(pairs, args, device, rank, world)
    if world > 1:
        import torch
        # gather a compact numeric summary on rank 0 (pooled means of the first 3 columns + acceptance)
        rows = torch.tensor([[s_["pooled_mean"][0], s_["pooled_mean"][-1], s_["acceptance"]] for s_ in summaries] or
                            np.zeros((0, 3)), dtype=torch.float64, device=phfdist.collective_device(device)).reshape(-1, 3)
        allrows = phfdist.gather_rows(rows, dst=0)
        if rank == 0:
            print("gathered summaries from %d ranks: %d pairs" % (world, sum(len(a) for a in allrows)))
    return summaries


if __name__ == "__main__":
    main()
