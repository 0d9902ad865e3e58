"""The on-device analyses of a run's rows, and the one life cycle the command lines drive them through.

Every analysis keeps an accumulator on the GPU that is fed the post-burn-in rows of every segment, reduced once, freed, written into
every pair's summary and reported in a line per rank.  An adapter per analysis (below, around the accumulator class of its module) says
how it is sized, checked against the free memory and built from the run's facts (`Run`), what it adds to a pair's summary and what it
reports; `AnalysisSet` holds the analyses of one sampler in a fixed order and is all a driver calls:

    kinds = fit_analyses(args)                       # the ordered list of the run: its flags, in the order below
    aset = AnalysisSet(kinds, Run(...))              # memory check + construction, in that order
    aset.feed_start(s.row0)                          # the start point is a saved row when there is no burn-in
    aset.feed(rows, r, nr)                           # per segment: saved rows r .. r + nr - 1, on the sampler's stream
    aset.finish()                                    # result() then free(), once each
    aset.record(summ, q)                             # per pair, in the same order: the summary's keys
    report(kinds, [aset, ...], rank, names, args)    # the report lines, over the sets of all launch groups

A new row analysis is one adapter and one entry in fit_analyses() or tempered_analyses()."""
import functools
import json

import numpy as np
import torch

from . import batch_means as bm
from . import correlations as cr
from . import de_moves as de
from . import design as ds
from . import diagnostics as dg
from . import doseresponse as dr
from . import drug_profile as dp
from . import loo as lo
from . import marginal as mg
from . import ppc as pp
from . import predictive
from . import quantiles as qn
from . import replica_exchange as rx
from . import savage_dickey as sd
from . import sensitivity as sn
from . import stepping_stone as ss
from . import waic as wc

WORKSPACE = "workspace, {:.1f} GB are free: select fewer pairs, fewer chains or a smaller --diagnostic-lags"


def check_memory(nbytes, device, what, hint=WORKSPACE):
    """refuse to start when the workspace of flag `what` would take more than 80 % of the free device memory (as --save-all-chains
    does); hint: the rest of the message from what the memory holds on"""
    free = torch.cuda.mem_get_info(device)[0]
    if nbytes > 0.8 * free:
        raise SystemExit(("{} needs {:.1f} GB of device memory for its " + hint).format(what, nbytes / 1e9, free / 1e9))


class Run(object):
    """The facts of one sampler's run that its analyses are built from, as keywords.  All runs: args, kind (model 1 | 2 or
    "hierarchical"), Q, C, cols (columns of a row, the log-target included) and their names `columns`, saved, burn (saved rows, and
    how many of them are burn-in), device, sampler_points.  The fits also: make_points (-> waic.Points of the problems, built once,
    when an analysis first asks for `points`), concs (per problem, its concentrations), seed, problem_ids, prior, de (the sampler's
    DEMoves or None).  Hierarchical also: seg_rows, cdf_chains, writers, rng_pred, fitted_all (per problem).  Tempered also:
    pair_index, rung_index (per problem), temperatures, num_pairs, swap.  Single-level fits also: pairs (per problem, its (drug,
    channel))."""

    def __init__(self, **facts):
        self.__dict__.update(facts)

    @property
    def rows(self):
        return self.saved - self.burn

    @functools.cached_property
    def points(self):
        return self.make_points()


class Analysis(object):
    """One analysis of one sampler's rows.  make(run) checks the memory and returns the accumulator; `first` is the first saved row
    it takes: the first after the burn-in, and with skips_row0 never row 0; `res` is its result once finish() has run (what the
    accumulator's attributes still say after free() stays readable); `module`: where the plain report line is, if it has one."""
    what, hint, skips_row0, module = None, WORKSPACE, False, None

    def __init__(self, run):
        self.run, self.first = run, max(run.burn, 1) if self.skips_row0 else run.burn
        self.acc = self.make(run)

    def check(self, nbytes):
        check_memory(nbytes, self.run.device, self.what, self.hint)

    def accumulate(self, rows):
        self.acc.accumulate(rows)

    def finish(self):
        self.res = self.acc.result()
        self.acc.free()

    def per_problem(self):
        return [self.res[q] for q in range(self.run.Q)]

    def record(self, summ, q):
        """add this analysis' keys to the summary of problem q"""

    @classmethod
    def report(cls, rank, names, group, args):
        """the report lines over `group`, this analysis of every set; names: the problems of all sets, in order"""
        return [cls.module.report_line(rank, names, [r for a in group for r in a.per_problem()])] if cls.module else []


class PredictiveCdfs(Analysis):
    """--predictive-cdfs: construct_hierarchical_cdfs.py fused into the run; files of its own instead of summary keys"""

    def make(self, run):
        return predictive.PredictiveCurves(run.Q, run.device)

    def accumulate(self, rows):
        self.acc.accumulate(rows, self.run.cdf_chains)

    def finish(self):
        self.res = [self.acc.result(q) for q in range(self.run.Q)]
        self.acc.free()

    def record(self, summ, q):
        run = self.run
        predictive.save_cdfs_and_samples(run.writers, summ["drug"], summ["channel"], summ["num_expts"], self.res[q], run.args.num_APs,
                                         run.rng_pred, run.fitted_all[q])


class Diagnostics(Analysis):
    what = "--diagnostics"

    def make(self, run):
        lags, run.diagnostics = run.args.diagnostic_lags, self            # (the batch means are reported against this ESS)
        self.check(dg.workspace_bytes(run.Q, run.cols, run.C, run.rows, lags))
        return dg.ChainDiagnostics(run.Q, run.C, run.cols, run.rows, lags, run.device)

    def record(self, summ, q):
        run = self.run
        summ["diagnostics"] = dg.json_record(self.res, q, run.args.diagnostic_lags, run.rows, run.C,
                                             columns=run.columns if run.kind == "hierarchical" else None)
        if run.de is not None:
            summ["diagnostics"]["chains_coupled_within_populations_of"] = run.de.G
            summ["diagnostics"]["note"] = de.COUPLING_NOTE.format(G=run.de.G)

    @classmethod
    def report(cls, rank, names, group, args):
        lines = [dg.report_line(rank, names, [v for a in group for v in a.res["rhat"]], [v for a in group for v in a.res["ess"]])]
        if args.de_every:
            lines.append("diagnostics [rank {}]: {}".format(rank, de.COUPLING_NOTE.format(G=args.de_population)))
        return lines


class BatchMeans(Analysis):
    """--diagnostic-batch-means: inside the diagnostics' record, and reported against their ESS (the flag needs --diagnostics)"""
    what = "--diagnostic-batch-means"

    def make(self, run):
        self.check(bm.workspace_bytes(run.Q, run.cols, run.C, run.rows))
        return bm.BatchMeans(run.Q, run.C, run.cols, run.rows, run.device)

    def record(self, summ, q):
        summ["diagnostics"]["batch_means"] = bm.json_record(self.res, q, de_coupled=self.run.de is not None)

    @classmethod
    def report(cls, rank, names, group, args):
        lines = [bm.report_line(rank, names, [v for a in group for v in a.run.diagnostics.res["ess"]],
                                [v for a in group for v in a.res["ess"]], [v for a in group for v in a.res["tau"]], args.thinning)]
        if args.de_every:
            lines.append("batch means [rank {}]: {}".format(rank, bm.DE_NOTE))
        return lines


class DeMoves(Analysis):
    """--de-every: the records of the differential-evolution moves.  No row analysis (the sampler counts them), but their key and
    their line stand between those of the row analyses."""
    module = de

    def make(self, run):
        return run.de

    def accumulate(self, rows):
        pass

    def finish(self):
        self.res = self.acc.records()

    def record(self, summ, q):
        summ["de_moves"] = self.res[q]


class Waic(Analysis):
    what, module = "--waic", wc

    def make(self, run):
        self.check(wc.workspace_bytes(run.Q, run.points.stride, run.C, run.rows))
        return wc.PointwiseWAIC(run.points, run.kind, run.Q, run.C, run.rows, run.device)

    def record(self, summ, q):
        summ["waic"] = wc.json_record(self.res[q], self.run.points, q)


class Loo(Analysis):
    what, module, hint = "--loo", lo, "workspace, {:.1f} GB are free: select fewer pairs, fewer chains or a smaller --loo-tail-per-chain"

    def make(self, run):
        tail = run.args.loo_tail_per_chain
        self.check(lo.workspace_bytes(run.Q, run.points.stride, run.C, run.rows, tail))
        return lo.PointwiseLOO(run.points, run.kind, run.Q, run.C, run.rows, run.device, tail)

    def record(self, summ, q):
        summ["loo"] = lo.json_record(self.res[q], self.run.points, q, self.acc.M, self.acc.k)


class ExperimentLoo(Analysis):
    what = "--leave-experiment-out"

    def make(self, run):
        a = run.args
        self.check(mg.workspace_bytes(run.Q, run.points.num_expts, run.C, run.rows, a.marginal_every, run.seg_rows))
        return mg.ExperimentLOO(run.points, run.Q, run.C, run.rows, a.marginal_nodes, a.marginal_every, run.device)

    def labels(self, q):
        return [e[0] for e in self.acc.epoints.info[q]]

    def record(self, summ, q):
        summ["loo_experiment"] = mg.json_record(self.res[q], self.labels(q), self.acc.nodes, self.acc.every)

    @classmethod
    def report(cls, rank, names, group, args):
        return [mg.report_line(rank, names, [r for a in group for r in a.per_problem()],
                               [a.labels(q) for a in group for q in range(a.run.Q)])]


class Quantiles(Analysis):
    """--quantiles, with the single-level --curve-bands or the hierarchical --predictive-bands riding on its histograms; `doses`:
    per problem, the doses of its band, or None without one"""
    what, hint = "--quantiles", "histograms, {:.1f} GB are free: select fewer pairs, fewer curve points or a smaller --quantile-bins"

    def make(self, run):
        a = run.args
        if run.kind == "hierarchical":
            # the doses of the bands: G over the concentrations of the pair's fitted experiments, then the named ones
            G, named = a.predictive_bands, tuple(a.band_concs or ())
            self.doses = [qn.band_doses(c, G, named) for c in run.concs] if G else None
            slots = 2 * (G + len(named)) if G else 0
            bands = dict(band_ln_doses=np.log(np.array(self.doses)) if G else None, seed=run.seed, problem_ids=run.problem_ids,
                         chain_id_base=0)
        else:
            slots = G = a.curve_bands
            self.doses = [qn.curve_doses(c, G) for c in run.concs] if G else None
            bands = dict(curve_ln_doses=np.log(np.array(self.doses)) if G else None, model=run.kind)
        self.check(qn.workspace_bytes(run.Q, run.cols, slots, a.quantile_bins))
        return qn.PosteriorQuantiles(run.Q, run.C, run.cols, run.rows, a.quantile_probs, a.quantile_bins, run.device, **bands)

    def record(self, summ, q):
        run = self.run
        summ["quantiles"] = qn.json_record(self.res, q, run.columns, run.args.quantile_bins)
        if self.doses is not None and run.kind == "hierarchical":
            summ["hierarchical_bands"] = qn.hier_band_record(self.res, q, self.doses[q], run.args.predictive_bands)
        elif self.doses is not None:
            summ["curve_band"] = qn.curve_band_record(self.res, q, self.doses[q])

    @classmethod
    def report(cls, rank, names, group, args):
        parts, band_nf = [], 0
        for a in group:
            res, nc = a.res, int(a.res["columns"])                  # the band slots follow the columns
            parts += [(res["bin_width"][q, :nc], res["min"][q, :nc], res["max"][q, :nc], res["non_finite"][q, :nc])
                      for q in range(a.run.Q)]
            band_nf += int(np.sum(res["non_finite"][:, nc:]))
        return [qn.report_line(rank, names, parts, band_nf if args.predictive_bands else None)]


class Ppc(Analysis):
    what, module = "--ppc", pp

    def make(self, run):
        self.check(pp.workspace_bytes(run.Q, run.points.stride, run.C, run.rows))
        return pp.PosteriorPredictiveCheck(run.points, run.kind, run.Q, run.C, run.rows, run.seed, run.problem_ids, 0, run.device)

    def record(self, summ, q):
        summ["ppc"] = pp.json_record(self.res[q], self.run.points, q)


class Sensitivity(Analysis):
    what, hint = "--sensitivity", "histograms, {:.1f} GB are free: select fewer pairs or a smaller --sensitivity-bins"

    def make(self, run):
        a, d = run.args, run.cols - 1
        self.check(sn.workspace_bytes(run.Q, d, run.C, run.rows, a.sensitivity_bins))
        return sn.PowerScaling(run.sampler_points, run.kind, run.Q, run.C, d, run.rows, a.sensitivity_delta, a.sensitivity_bins,
                               run.device, prior=run.prior, threshold=a.sensitivity_threshold)

    def record(self, summ, q):
        summ["sensitivity"] = sn.json_record(self.res, q, self.run.columns[:-1])

    @classmethod
    def report(cls, rank, names, group, args):
        return [sn.report_line(rank, names, [sn.part_of(a.res, q) for a in group for q in range(a.run.Q)])]


class SteppingStone(Analysis):
    """--stepping-stone of the tempered run: the rows the fused <log L(t=1)> counts, saved rows with t > moments_after, i.e. from row
    max(burn, 1) on.  `res`: the reduced unit columns; `se_joint`: under replica exchange, the se over the replica sets, which has to
    be taken from the workspace before it is freed."""
    what, skips_row0 = "--stepping-stone", True

    def make(self, run):
        self.check(ss.workspace_bytes(run.Q, run.C, run.saved - self.first))
        delta = ss.deltas(run.temperatures)
        return ss.SteppingStone(run.sampler_points, run.kind, run.pair_index, [float(delta[r]) for r in run.rung_index], run.C,
                                run.saved - self.first, run.device)

    def finish(self):
        run = self.run
        self.res = self.acc.reduced()
        self.se_joint = rx.joint_se(self.acc, run.num_pairs, len(run.temperatures)) if run.swap > 0 else None
        self.acc.free()


class Design(Analysis):
    """--next-dose: the expected information gain of one further measurement at candidate doses (single-level only)"""
    what, module = "--next-dose", ds
    hint = "accumulators, {:.1f} GB are free: select fewer pairs, fewer candidate doses or a smaller --next-dose-bins"

    def make(self, run):
        a = run.args
        doses = [ds.candidate_doses(c, a.next_dose, a.next_dose_concs) for c in run.concs]
        self.check(ds.workspace_bytes(run.Q, len(doses[0]), a.next_dose_bins, run.C))
        return ds.NextDose(run.kind, run.Q, run.C, doses, run.concs, a.next_dose_bins, a.next_dose_every, run.device)

    def record(self, summ, q):
        summ["next_dose"] = ds.json_record(self.res[q])

    @classmethod
    def report(cls, rank, names, group, args):
        return [ds.report_line(rank, names, [r for a in group for r in a.per_problem()], args.next_dose)]


class Correlations(Analysis):
    """--correlations: the posterior and within-chain correlation matrices of the parameter columns (the log-target is left out, as
    --sensitivity leaves it out) and the multivariate R-hat"""
    what, module, hint = "--correlations", cr, "co-moments, {:.1f} GB are free: select fewer pairs or fewer chains"

    def make(self, run):
        self.check(cr.workspace_bytes(run.Q, run.cols - 1, run.C, run.rows))
        return cr.PosteriorCorrelations(run.Q, run.C, run.columns[:-1], run.rows, run.device)

    def record(self, summ, q):
        run = self.run
        summ["correlations"] = cr.json_record(self.res[q])
        if run.de is not None:                                            # B is then taken over dependent chains
            summ["correlations"]["chains_coupled_within_populations_of"] = run.de.G
            summ["correlations"]["note"] = de.COUPLING_NOTE.format(G=run.de.G)


class SavageDickeyBF(Analysis):
    """--savage-dickey: the Bayes factor B12 of Hill = 1 against Hill free from the model-2 draws alone (single-level, -m 2 only)"""
    what, module = "--savage-dickey", sd
    hint = "accumulators, {:.1f} GB are free: select fewer pairs or fewer chains"

    def make(self, run):
        a = run.args
        self.check(sd.workspace_bytes(run.Q, run.C, a.savage_dickey_panels))
        return sd.SavageDickey(run.sampler_points, run.Q, run.C, a.savage_dickey_panels, a.savage_dickey_every, run.device)

    def record(self, summ, q):
        summ["bayes_factor"] = sd.json_record(self.res[q])


class DrugProfile(Analysis):
    """--drug-profile-concs / --drug-profile-cmax: the joint multi-channel block of every drug at its doses (single-level only); a
    file of its own per drug instead of summary keys, written when the drug's first pair is recorded.  `records`: per profiled drug"""
    what = "--drug-profile-concs / --drug-profile-cmax"
    hint = "histograms, {:.1f} GB are free: select fewer drugs, fewer doses or a smaller --drug-profile-bins"

    def make(self, run):
        a = run.args
        clean = dr._clean                                                 # the names the files carry: KvLQT1/mink -> KvLQT1_mink
        try:
            self.plan = p = dp.Plan([(clean(d), clean(c)) for d, c in run.pairs], [clean(c) for c in dr.channels],
                                    a.drug_profile_concs, a.drug_profile_cmax, a.drug_profile_multiples, a.drug_profile_weights)
        except ValueError as e:
            raise SystemExit(str(e))
        self.records = []
        if not p.drugs:
            return None
        shape = (len(p.drugs), len(p.channels), p.doses.shape[1], a.drug_profile_bins)
        self.check(dp.workspace_bytes(*shape))
        return dp.DrugProfile(run.kind, run.Q, run.C, p.map, p.weights, p.doses, run.rows, a.quantile_probs, a.drug_profile_bins, run.device)

    def accumulate(self, rows):
        if self.acc is not None:
            self.acc.accumulate(rows)

    def finish(self):
        if self.acc is None:
            return
        res, p = self.acc.result(), self.plan
        self.acc.free()
        self.records = [dp.json_record(res, d, drug, p.channels, p.cmax[d], p.multiples) for d, drug in enumerate(p.drugs)]
        self.writes_at = {p.first_problem(d): d for d in range(len(p.drugs))}

    def record(self, summ, q):
        d = self.writes_at.get(q) if self.records else None
        if d is not None:
            with open(dr.drug_profile_file(self.plan.drugs[d]), "w") as f:
                json.dump(self.records[d], f, indent=1)

    @classmethod
    def report(cls, rank, names, group, args):
        return [dp.report_line(rank, [r for a in group for r in a.records], [d for a in group for d in a.plan.skipped])]


def fit_analyses(args):
    """the analyses of a PyHillFit run, single-level or hierarchical, in the order they are built, fed, recorded and reported"""
    table = [(args.hierarchical and args.predictive_cdfs, PredictiveCdfs), (args.diagnostics, Diagnostics),
             (args.diagnostic_batch_means, BatchMeans), (args.de_every, DeMoves), (args.waic, Waic), (args.loo, Loo),
             (args.leave_experiment_out, ExperimentLoo), (args.quantiles, Quantiles), (args.ppc, Ppc), (args.sensitivity, Sensitivity),
             (args.next_dose and not args.hierarchical, Design), (args.correlations, Correlations),
             (args.savage_dickey and not args.hierarchical, SavageDickeyBF),
             (getattr(args, "drug_profile", False) and not args.hierarchical, DrugProfile)]   # (set by check_args)
    return [kind for on, kind in table if on]


def tempered_analyses(args):
    """the analyses of a PyHillTemp run, in the order they are built and fed (their results ride on the run's one gather)"""
    table = [(args.diagnostics, Diagnostics), (args.diagnostic_batch_means, BatchMeans), (args.stepping_stone, SteppingStone)]
    return [kind for on, kind in table if on]


class AnalysisSet(object):
    """the analyses of one sampler's run, each built from `run` in the order of `kinds` and driven in that order"""

    def __init__(self, kinds, run):
        self.items = [kind(run) for kind in kinds]

    def of(self, kind):
        """the set's analysis of this kind, or None"""
        return next((a for a in self.items if isinstance(a, kind)), None)

    def feed_start(self, row0):
        """row0 [Q][cols][C]: saved row 0, the start point; a row like the others for an analysis whose first row it is"""
        for a in self.items:
            if a.first == 0:
                a.accumulate(row0.unsqueeze(0).contiguous())

    def feed(self, rows, r, nr):
        """rows: saved rows r .. r + nr - 1; every analysis takes those from its first row on (saved rows before it are the burn-in)"""
        for a in self.items:
            first = max(0, a.first - r)
            if first < nr:
                a.accumulate(rows[first:])

    def finish(self):
        for a in self.items:
            a.finish()

    def record(self, summ, q):
        for a in self.items:
            a.record(summ, q)


def report(kinds, sets, rank, names, args):
    """the report lines of a rank, in the order of `kinds`: one analysis over all sets (none, when no pair was loaded) at a time"""
    return [line for kind in kinds for line in kind.report(rank, names, [s.of(kind) for s in sets], args)]
