"""The life cycle of the run analyses (pyhillfit_amd/analyses.py) without a GPU: the burn-in gate, the fixed orders, result-then-free,
and the memory refusals' texts.  The adapters under test are the real ones with make() (and, for the orders, record() and report())
replaced by loggers, so the lists, the first rows and the feed / finish plumbing are the shipped ones."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from pyhillfit_amd import PyHillFit, PyHillTemp  # noqa: E402
from pyhillfit_amd import analyses as an  # noqa: E402
from pyhillfit_amd import waic as wc  # noqa: E402


class Acc(object):
    """stands in for an accumulator class: logs what the adapter calls"""

    def __init__(self, name, log):
        self.name, self.log, self.got = name, log, []

    def accumulate(self, rows, chains_used=None):
        self.log.append(("accumulate", self.name))
        self.got.append(rows)

    def result(self, q=None):
        if not q:                                                     # (the predictive curves' result is taken per problem)
            self.log.append(("result", self.name))
        return {}

    reduced = records = result

    def free(self):
        self.log.append(("free", self.name))


def stub(kind, log):
    def make(self, run):
        log.append(("make", kind.__name__))
        return Acc(kind.__name__, log)

    def record(self, summ, q):
        summ[kind.__name__] = q

    def report(cls, rank, names, group, args):
        assert len(group) == len(names)                               # (the tests below: one problem per set)
        return [kind.__name__]
    return type(kind.__name__, (kind,), {"make": make, "record": record, "report": classmethod(report)})


def fit_args(*flags):
    parser = PyHillFit.build_parser()
    args = parser.parse_args(["--data-file", "x.csv", "-m", "2"] + list(flags))
    PyHillFit.check_args(parser, args)
    return args


def tempered_args(*flags):
    return PyHillTemp.build_parser().parse_args(["--data-file", "x.csv", "-m", "2", "-d", "0", "-c", "0"] + list(flags))


# ---- the burn-in gate ---------------------------------------------------------------------------------------------------------
ROWS, SEG, Q, COLS, C = 11, 4, 2, 3, 5                                # row 0 and segments of 4, 4 and 2 rows


@pytest.mark.parametrize("burn", [0, 1, 3, 5, 50])                     # none, row 0 only, mid-segment, a segment boundary, everything
def test_burn_in_gate(burn):
    saved = torch.arange(ROWS * Q * COLS * C, dtype=torch.float64).reshape(ROWS, Q, COLS, C)
    row0 = saved[0].transpose(0, 1).contiguous().transpose(0, 1)      # the same numbers, not contiguous
    assert not row0.is_contiguous()
    log = []
    aset = an.AnalysisSet([stub(an.Diagnostics, log), stub(an.SteppingStone, log)], an.Run(saved=ROWS, burn=burn))
    aset.feed_start(row0)
    r = 1
    while r < ROWS:
        nr = min(SEG, ROWS - r)
        aset.feed(saved[r:r + nr], r, nr)
        r += nr
    for a, first in zip(aset.items, (burn, max(burn, 1))):
        assert a.first == first
        got = a.acc.got
        assert all(g.shape[0] > 0 for g in got)                       # never called with nothing
        if first >= ROWS:
            assert got == []
            continue
        assert torch.equal(torch.cat(got), saved[first:])
        starts_with_row0 = tuple(got[0].shape) == (1, Q, COLS, C) and torch.equal(got[0][0], saved[0])
        assert starts_with_row0 == (first == 0)
        if first == 0:
            assert got[0].is_contiguous() and not any(torch.equal(g[0], saved[0]) for g in got[1:])


# ---- the orders ---------------------------------------------------------------------------------------------------------------
SINGLE_LEVEL = ["Diagnostics", "BatchMeans", "Waic", "Loo", "Quantiles", "Ppc", "Sensitivity"]
HIERARCHICAL = ["PredictiveCdfs", "Diagnostics", "BatchMeans", "Waic", "Loo", "ExperimentLoo", "Quantiles", "Ppc", "Sensitivity"]
HIERARCHICAL_DE = ["PredictiveCdfs", "Diagnostics", "BatchMeans", "DeMoves", "Waic", "Loo", "ExperimentLoo", "Quantiles", "Ppc",
                   "Sensitivity"]
TEMPERED = ["Diagnostics", "BatchMeans", "SteppingStone"]
SL_FLAGS = ["--diagnostics", "--diagnostic-batch-means", "--waic", "--loo", "--quantiles", "--curve-bands", "8", "--ppc", "--sensitivity"]
HIER_FLAGS = ["--hierarchical", "--predictive-cdfs", "--diagnostics", "--diagnostic-batch-means", "--waic", "--loo",
              "--leave-experiment-out", "--quantiles", "--predictive-bands", "4", "--ppc", "--sensitivity"]
DE_FLAGS = ["--de-every", "100", "--num-chains", "64"]
TEMPERED_FLAGS = ["--diagnostics", "--diagnostic-batch-means", "--stepping-stone"]


def _life_cycle(kinds, args):
    """one set of stubs through a run of row 0 and one segment, no burn-in -> the log, the summary's keys, the report"""
    log = []
    stubs = [stub(k, log) for k in kinds]
    aset = an.AnalysisSet(stubs, an.Run(saved=3, burn=0, Q=1, cdf_chains=1, swap=0))
    rows = torch.zeros((3, 1, 2, 2), dtype=torch.float64)
    aset.feed_start(rows[0])
    aset.feed(rows[1:], 1, 2)
    aset.finish()
    summ = {}
    aset.record(summ, 0)
    return log, list(summ), an.report(stubs, [aset], 0, ["a pair"], args)


@pytest.mark.parametrize("kinds_of, args, want", [
    (an.fit_analyses, fit_args(*SL_FLAGS), SINGLE_LEVEL),
    (an.fit_analyses, fit_args(*HIER_FLAGS), HIERARCHICAL),
    (an.fit_analyses, fit_args(*(HIER_FLAGS + DE_FLAGS)), HIERARCHICAL_DE),
    (an.tempered_analyses, tempered_args(*TEMPERED_FLAGS), TEMPERED)], ids=["single-level", "hierarchical", "hierarchical-de", "tempered"])
def test_orders_and_finish(kinds_of, args, want):
    kinds = kinds_of(args)
    assert [k.__name__ for k in kinds] == want
    log, keys, lines = _life_cycle(kinds, args)
    fed = [n for n in want if n != "DeMoves"]                         # the moves are counted by the sampler, not fed
    start = [n for n in fed if n != "SteppingStone"]                  # the stepping-stone never takes row 0
    assert [n for e, n in log if e == "make"] == want
    assert [n for e, n in log if e == "accumulate"] == start + fed    # row 0, then the segment, each in the construction order
    assert [n for e, n in log if e == "result"] == want
    assert keys == want and lines == want
    for n in fed:                                                     # result once, then free once
        events = [e for e, name in log if name == n and e in ("result", "free")]
        assert events == ["result", "free"]
    assert ("free", "DeMoves") not in log                             # (the sampler's own object: nothing of the analyses' to free)


def test_single_level_run_ignores_the_hierarchical_only_flag():
    assert an.fit_analyses(fit_args("--predictive-cdfs")) == []


@pytest.mark.parametrize("flags, want", [
    (["--diagnostics"], ["Diagnostics"]), (["--diagnostics", "--diagnostic-batch-means"], ["Diagnostics", "BatchMeans"]),
    (["--waic"], ["Waic"]), (["--loo"], ["Loo"]), (["--quantiles"], ["Quantiles"]), (["--quantiles", "--curve-bands", "8"], ["Quantiles"]),
    (["--ppc"], ["Ppc"]), (["--sensitivity"], ["Sensitivity"]), (["--hierarchical", "--predictive-cdfs"], ["PredictiveCdfs"]),
    (["--hierarchical", "--leave-experiment-out"], ["ExperimentLoo"]),
    (["--hierarchical", "--quantiles", "--predictive-bands", "4"], ["Quantiles"]), (["--hierarchical"] + DE_FLAGS, ["DeMoves"]), ([], [])])
def test_one_flag_one_adapter(flags, want):
    assert [k.__name__ for k in an.fit_analyses(fit_args(*flags))] == want


@pytest.mark.parametrize("flags, want", [(["--diagnostics"], ["Diagnostics"]), (["--stepping-stone"], ["SteppingStone"]), ([], [])])
def test_one_flag_one_adapter_tempered(flags, want):
    assert [k.__name__ for k in an.tempered_analyses(tempered_args(*flags))] == want


# ---- the memory refusals ------------------------------------------------------------------------------------------------------
# a run of the default length (100001 saved rows, 25000 of them burn-in) of 2000 problems x 4096 chains against 0.1 GB of free memory:
# the texts as the command lines printed them before the check was one function
NQ, NC, SAVED, BURN = 2000, 4096, 100001, 25000
TAIL = "0.1 GB are free: select fewer pairs, fewer chains or a smaller "
REFUSALS = {
    "--diagnostics": "--diagnostics needs 270.0 GB of device memory for its workspace, " + TAIL + "--diagnostic-lags",
    "--diagnostic-batch-means": "--diagnostic-batch-means needs 21.5 GB of device memory for its workspace, " + TAIL + "--diagnostic-lags",
    "--waic": "--waic needs 2.0 GB of device memory for its workspace, " + TAIL + "--diagnostic-lags",
    "--loo": "--loo needs 25.4 GB of device memory for its workspace, " + TAIL + "--loo-tail-per-chain",
    "--quantiles": "--quantiles needs 17.8 GB of device memory for its histograms, 0.1 GB are free: select fewer pairs, fewer curve "
                   "points or a smaller --quantile-bins",
    "--ppc": "--ppc needs 1.8 GB of device memory for its workspace, " + TAIL + "--diagnostic-lags",
    "--sensitivity": "--sensitivity needs 11.3 GB of device memory for its histograms, 0.1 GB are free: select fewer pairs or a smaller "
                     "--sensitivity-bins",
    "--leave-experiment-out": "--leave-experiment-out needs 1587.3 GB of device memory for its workspace, " + TAIL + "--diagnostic-lags",
    "--predictive-bands": "--quantiles needs 37.8 GB of device memory for its histograms, 0.1 GB are free: select fewer pairs, fewer "
                          "curve points or a smaller --quantile-bins",
    "--stepping-stone": "--stepping-stone needs 0.3 GB of device memory for its workspace, " + TAIL + "--diagnostic-lags",
}
EXPERIMENT = np.array([[0.1, 10.0], [1.0, 50.0], [10.0, 90.0]])
CONCS = [np.array([0.1, 1.0, 10.0])] * NQ


@pytest.fixture
def little_memory(monkeypatch):
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (100_000_000, 10 ** 12))


def _refusal(kind, run):
    with pytest.raises(SystemExit) as e:
        kind(run)
    return str(e.value)


@pytest.mark.parametrize("flags, kind", [
    (["--diagnostics"], an.Diagnostics), (["--diagnostics", "--diagnostic-batch-means"], an.BatchMeans), (["--waic"], an.Waic),
    (["--loo"], an.Loo), (["--quantiles", "--curve-bands", "64"], an.Quantiles), (["--ppc"], an.Ppc), (["--sensitivity"], an.Sensitivity)])
def test_single_level_refusals(little_memory, flags, kind):
    run = an.Run(args=fit_args(*flags), kind=2, Q=NQ, C=NC, cols=4, saved=SAVED, burn=BURN, device="cpu", sampler_points=None,
                 concs=CONCS, seed=25, problem_ids=list(range(NQ)), prior=None, de=None,
                 make_points=lambda: wc.Points.single_level([[EXPERIMENT, EXPERIMENT]] * NQ))
    assert _refusal(kind, run) == REFUSALS[flags[-1] if flags[-1].startswith("--") else flags[0]]


@pytest.mark.parametrize("flags, kind", [
    (["--leave-experiment-out", "--marginal-every", "1"], an.ExperimentLoo),
    (["--quantiles", "--predictive-bands", "64", "--band-concs", "0.5,5"], an.Quantiles)])
def test_hierarchical_refusals(little_memory, flags, kind):
    run = an.Run(args=fit_args("--hierarchical", *flags), kind="hierarchical", Q=NQ, C=NC, cols=12, saved=SAVED, burn=BURN, device="cpu",
                 sampler_points=None, concs=CONCS, seed=25, problem_ids=list(range(NQ)), prior=None, de=None, seg_rows=4000,
                 make_points=lambda: wc.Points.hierarchical([[EXPERIMENT] * 3] * NQ))
    assert _refusal(kind, run) == REFUSALS["--leave-experiment-out" if kind is an.ExperimentLoo else "--predictive-bands"]


def test_tempered_refusal(little_memory):
    run = an.Run(args=tempered_args("--stepping-stone"), kind=2, Q=NQ, C=NC, cols=4, saved=SAVED, burn=BURN, device="cpu",
                 sampler_points=None, pair_index=[0] * NQ, rung_index=[0] * NQ, temperatures=[0.0, 1.0], num_pairs=NQ // 2, swap=0)
    assert _refusal(an.SteppingStone, run) == REFUSALS["--stepping-stone"]


def test_the_pooled_loo_check_says_what_the_adapter_says(little_memory):
    with pytest.raises(SystemExit) as e:
        an.check_memory(25.4e9, "cpu", an.Loo.what, an.Loo.hint)
    assert str(e.value) == REFUSALS["--loo"]


def test_enough_memory_is_no_refusal(monkeypatch):
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (10 ** 9, 10 ** 12))
    an.check_memory(0.8e9, "cpu", "--waic")                           # 80 % of the free memory is still taken
    with pytest.raises(SystemExit):
        an.check_memory(0.8e9 + 1, "cpu", "--waic")
