"""The life cycle the twelve streaming analyses share (pyhillfit_amd/accumulator.py) on the GPU, at the smallest shape that still
exercises every class: 2 problems, 70 chains (a full wavefront and a ragged one), 9 post-burn-in rows (an odd total: h = 4 and a dropped
middle row), a row stride one larger than the columns read (SavageDickey takes exactly the 4 columns of a model-2 row).

Per class: one accumulate call and calls of 1, 3 and 5 rows give the same bits; a call with a wrong shape, a non-contiguous view or one
row too many raises ValueError and leaves rows_seen and the device state as they were; result() before the last row raises where
the class has a completeness rule (PosteriorQuantiles and PowerScaling report running results by design, NextDose and SavageDickey
have no total); free() drops the device tensors."""
import os

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

Q, C, N = 2, 70, 9


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def dr():
    from pyhillfit_amd import doseresponse
    doseresponse.setup(os.path.join(REPO, "data", "crumb_dataset.json"))
    return doseresponse


PAIRS = [(np.array([0.01, 0.1, 1.0, 10.0, 100.0, 1.0, 10.0]), np.array([0.0, 4.0, 31.0, 77.0, 100.0, 35.0, 81.0])),
         (np.array([0.3, 3.0, 30.0, 300.0, 3.0]), np.array([2.0, 22.0, 64.0, 100.0, 18.0]))]


def model2_rows():
    """[9][2][4][70]: pIC50, Hill, sigma and a log-target column"""
    rng = np.random.default_rng(9)
    x = np.empty((N, Q, 4, C))
    x[:, :, 0] = rng.normal(0.0, 0.12, (N, Q, C)) + np.array([5.75, 4.9])[None, :, None]
    x[:, :, 1] = np.exp(rng.normal(-0.2, 0.1, (N, Q, C)))
    x[:, :, 2] = np.exp(rng.normal(2.0, 0.2, (N, Q, C)))
    x[:, :, 3] = -40.0 + rng.normal(0.0, 1.0, (N, Q, C))
    return x


def hier_rows(ne):
    """[9][2][5 + 2 Ne + 1][70]: the experiments' own columns and the spare one are never read"""
    rng = np.random.default_rng(10)
    x = np.full((N, Q, 5 + 2 * ne + 1, C), np.nan)
    s = (N, Q, C)
    x[:, :, 0], x[:, :, 1], x[:, :, 2], x[:, :, 3] = rng.uniform(0.5, 2, s), rng.uniform(2.5, 5, s), rng.uniform(3, 8, s), rng.uniform(0.05, 1, s)
    x[:, :, 4 + 2 * ne] = rng.uniform(4, 40, s)
    return x


def sl_points():
    from pyhillfit_amd import waic
    return waic.Points.single_level([[np.column_stack(p)] for p in PAIRS])


def hier_points(ne=2):
    from pyhillfit_amd import waic
    rng = np.random.default_rng(11)
    per = []
    for q in range(Q):
        expts = []
        for n in (5, 4)[:ne]:
            conc = 10.0 ** rng.uniform(-2, 2, n)
            expts.append(np.column_stack([conc, np.clip(100.0 / (1.0 + (3.0 / conc) ** 0.9) + rng.normal(0, 6, n), 0.5, 99.5)]))
        per.append(expts)
    return waic.Points.hierarchical(per)


def values(d):
    return [np.asarray(d[k]) for k in sorted(d)]


def of_points(acc, arrays):
    """arrays [Q][stride][...] -> per problem, the part of its own points (what lies beyond a problem's count is not defined)"""
    return [a[q, :n] for a in arrays for q, n in enumerate(acc.points.count)]


# name -> (make(device, dr) -> accumulator, rows, outcome(accumulator) -> list of numpy arrays, result() raises before the last row)
def specs():
    from pyhillfit_amd import (batch_means, correlations, design, diagnostics, loo, marginal, ppc, quantiles, savage_dickey, sensitivity,
                               stepping_stone, waic)
    from pyhillfit_amd.sampler import DevicePoints
    x = model2_rows()
    ln_doses = np.log(np.array([[0.1, 1.0, 10.0], [0.3, 3.0, 30.0]]))
    return {
        "ChainDiagnostics": (lambda g, dr: diagnostics.ChainDiagnostics(Q, C, 3, N, device=g), x,
                             lambda a: [a.reduced()] + values(a.result()), True),
        "BatchMeans": (lambda g, dr: batch_means.BatchMeans(Q, C, 3, N, g), x, lambda a: [a.reduced(), a.workspace()], True),
        "PosteriorCorrelations": (lambda g, dr: correlations.PosteriorCorrelations(Q, C, 3, N, g), x, lambda a: [a.reduced(), a.workspace()], True),
        "PointwiseWAIC": (lambda g, dr: waic.PointwiseWAIC(sl_points(), 2, Q, C, N, g), x, lambda a: of_points(a, a.reduced()), True),
        "PointwiseLOO": (lambda g, dr: loo.PointwiseLOO(sl_points(), 2, Q, C, N, g), x, lambda a: of_points(a, values(a.reduced(tail=True))), True),
        "PosteriorPredictiveCheck": (lambda g, dr: ppc.PosteriorPredictiveCheck(sl_points(), 2, Q, C, N, 7, None, 0, g), x,
                                     lambda a: [a.reduced()], True),
        "PosteriorQuantiles": (lambda g, dr: quantiles.PosteriorQuantiles(Q, C, 3, N, bins=256, device=g, curve_ln_doses=ln_doses, model=2), x,
                               lambda a: [a.reduced()] + list(a.counts()), False),
        "PowerScaling": (lambda g, dr: sensitivity.PowerScaling(DevicePoints(dr.PackedPoints(PAIRS), g), 2, Q, C, 3, N, 0.25, 256, g), x,
                         lambda a: list(a.reduced(per_chain=True)) + [a.counts()], False),
        "SteppingStone": (lambda g, dr: stepping_stone.SteppingStone(dr.PackedPoints(PAIRS), 2, [0, 1], [0.25, 0.0], C, N, g), x,
                          lambda a: [a.reduced()] + values(a.accumulators()), True),
        "ExperimentLOO": (lambda g, dr: marginal.ExperimentLOO(hier_points(), Q, C, N, 32, 1, g), hier_rows(2),
                          lambda a: list(a.waic.reduced()) + values(a.psis.reduced()) + [a.marginal.gap_maxima()], True),
        "NextDose": (lambda g, dr: design.NextDose(2, Q, C, np.exp(ln_doses), None, 128, 2, g), x, lambda a: [a.accumulators()], False),
        "SavageDickey": (lambda g, dr: savage_dickey.SavageDickey(dr.PackedPoints(PAIRS), Q, C, 16, 2, g), x, lambda a: [a.accumulators()], False),
    }


NAMES = ["ChainDiagnostics", "BatchMeans", "PosteriorCorrelations", "PointwiseWAIC", "PointwiseLOO", "PosteriorPredictiveCheck",
         "PosteriorQuantiles", "PowerScaling", "SteppingStone", "ExperimentLOO", "NextDose", "SavageDickey"]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def device_state(acc):
    """clones of the device tensors an accumulate call writes"""
    parts = [acc.waic, acc.psis] if hasattr(acc, "waic") else [acc]
    t = [getattr(p, name) for p in parts for name in ("ws", "acc") if getattr(p, name, None) is not None]
    if hasattr(acc, "marginal"):
        t.append(acc.marginal.gap_max)
    assert t
    return [v.clone() for v in t]


@pytest.mark.parametrize("name", NAMES)
def test_life_cycle(gpu, dr, name):
    from pyhillfit_amd import accumulator
    make, x, outcome, raises_incomplete = specs()[name]
    rows = torch.from_numpy(np.ascontiguousarray(x)).to(gpu)
    stride = rows.shape[2]
    whole = make(gpu, dr)
    assert isinstance(whole, accumulator.RowAccumulator) and type(whole).__name__ == name
    assert stride == (4 if name == "SavageDickey" else whole.min_cols + 1)
    whole.accumulate(rows)
    assert whole.rows_seen == N
    want = outcome(whole)

    cut = make(gpu, dr)
    cut.accumulate(rows[0:1])
    cut.accumulate(rows[1:4])
    assert cut.rows_seen == 4
    before = device_state(cut)
    wide = torch.zeros((5, Q, stride + 2, C), dtype=torch.float64, device=gpu)
    bad = {"chains": rows[4:9, :, :, :C - 1].contiguous(), "problems": rows[4:9, :1].contiguous(), "rank": rows[4],
           "columns": rows[4:9, :, :stride - 2].contiguous() if name != "SavageDickey" else wide,
           "non-contiguous": wide[:, :, :stride], "float32": rows[4:9].float(), "host": rows[4:9].cpu()}
    if whole.N is not None:
        bad["one row too many"] = torch.cat([rows[4:9], rows[:1]])
    for what, t in bad.items():
        with pytest.raises(ValueError):
            cut.accumulate(t)
        assert cut.rows_seen == 4, what
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.int64), b.view(torch.int64)) for a, b in zip(before, device_state(cut)))
    if raises_incomplete:
        with pytest.raises(ValueError, match="only 4 of 9 rows accumulated"):
            cut.result()
    cut.accumulate(rows[4:9])
    assert cut.rows_seen == N
    got = outcome(cut)
    assert len(got) == len(want) and all(same_bits(g, w) for g, w in zip(got, want))
    cut.result()

    if whole.N is not None:
        with pytest.raises(ValueError, match="10 rows would exceed total_rows = 9"):
            cut.accumulate(rows[:1])
        assert cut.rows_seen == N and all(same_bits(g, w) for g, w in zip(outcome(cut), want))
    assert cut.accumulate(rows[:0]) is None and cut.rows_seen == N            # no rows: nothing to do
    for acc in (whole, cut):
        acc.free()
        if name == "ExperimentLOO":                                           # its device tensors are its parts'
            assert acc.marginal is None and acc.waic.ws is None and acc.waic.dp is None and acc.psis.ws is None and acc.psis.dp is None
        else:
            assert all(getattr(acc, t) is None for t in acc.tensors)
