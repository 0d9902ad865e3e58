"""Convergence diagnostics on the GPU: the streaming accumulation (phf_diagnostics_*) against the direct numpy restatement of
test_diagnostics_host.py, bit-identical results however the rows are cut, the samplers and the command lines."""
import glob
import json
import os

import numpy as np
import pytest

from conftest import REPO
from test_diagnostics_host import ar1, restated

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return "cuda:0"


@pytest.fixture(scope="module")
def dr_setup():
    from pyhillfit_amd import doseresponse as dr
    dr.setup(os.path.join(REPO, "data", "crumb_dataset.json"))
    return dr


def synthetic_rows(seed, chains, cols, rows, problems=2):
    """[rows][problems][cols + 1][chains]: AR(1) columns with phi 0.3..0.8 around offsets up to -40 (a log-target-like column);
    the last column of the stride is NOT diagnosed (row_stride_cols > num_columns)"""
    rng = np.random.default_rng(seed)
    x = np.zeros((rows, problems, cols + 1, chains))
    for q in range(problems):
        for j in range(cols):
            phi = 0.3 + 0.5 * ((q * cols + j) % 5) / 4
            x[:, q, j, :] = ar1(rng, chains, rows, phi).T * (1 + j) - 40.0 * (j == cols - 1) + 3 * q
    x[:, :, cols, :] = np.nan
    return x


def run_diag(x, cols, lags, cuts, device):
    from pyhillfit_amd.diagnostics import ChainDiagnostics
    t = torch.from_numpy(np.ascontiguousarray(x)).to(device)
    d = ChainDiagnostics(x.shape[1], x.shape[3], cols, x.shape[0], lags, device)
    r = 0
    for n in cuts:
        d.accumulate(t[r:r + n])
        r += n
    assert r == x.shape[0]
    return d.result()


def compare(res, x, cols, lags):
    for q in range(x.shape[1]):
        for j in range(cols):
            rh, ess, mcse, flag, margin = restated(x[:, q, j, :].T, lags)
            assert margin > 1e-6, "a rounding difference could flip Geyer's cut on this seed"
            assert abs(res["rhat"][q, j] / rh - 1) < 1e-12, (q, j)
            assert bool(res["lag_limit_reached"][q, j]) == flag, (q, j)
            if flag:
                assert np.isnan(res["ess"][q, j]) and np.isnan(res["mcse_mean"][q, j])
            else:
                assert abs(res["ess"][q, j] / ess - 1) < 1e-9 and abs(res["mcse_mean"][q, j] / mcse - 1) < 1e-9, (q, j)


@pytest.mark.parametrize("chains,cols,rows,lags", [(1, 3, 301, 256), (2, 4, 300, 20), (63, 12, 121, 256), (64, 3, 400, 64),
                                                   (65, 4, 257, 100), (130, 3, 90, 256), (64, 12, 1000, 8)])
def test_accumulation_matches_restatement(gpu, chains, cols, rows, lags):
    x = synthetic_rows(chains * 7 + rows, chains, cols, rows)
    res = run_diag(x, cols, lags, [rows // 3, rows - rows // 3], gpu)
    compare(res, x, cols, lags)


def test_segmentation_invariance(gpu):
    x = synthetic_rows(11, 65, 4, 203)
    whole = run_diag(x, 4, 40, [203], gpu)
    sevens = run_diag(x, 4, 40, [7] * 29, gpu)
    ones = run_diag(x, 4, 40, [1] * 203, gpu)
    for k in ("rhat", "ess", "mcse_mean", "lag_limit_reached"):
        assert np.array_equal(whole[k], sevens[k], equal_nan=k != "lag_limit_reached")
        assert np.array_equal(whole[k], ones[k], equal_nan=k != "lag_limit_reached")


def test_single_level_sampler_streaming(gpu, dr_setup):
    from pyhillfit_amd import bestfit
    from pyhillfit_amd.diagnostics import ChainDiagnostics
    from pyhillfit_amd.sampler import SingleLevelSampler
    dr = dr_setup
    dr.define_model(2)
    ne, _, ex = dr.load_crumb_data("Amiodarone", "hERG")
    concs, y = dr.concatenate_experiments(ne, ex)
    th0 = bestfit.chain_start(bestfit.best_fit_batch([(concs, y)], 2)[0][0], 2)
    s = SingleLevelSampler(dr.PackedPoints([(concs, y)]), 2, [0], [1.0], 256, thinning=5, seed=25, adapt_start=3000, device=gpu)
    s.init(np.array([th0]), cov_identity=False, cov_scale=0.05)
    T, seg = 20000, 3000
    saved = T // 5 + 1
    burn = saved // 4
    d = ChainDiagnostics(1, 256, 4, saved - burn, 256, gpu)
    host, r, done = [s.row0.cpu().numpy()[None]], 1, 0
    while done < T:
        k = min(seg, T - done)
        rows = s.advance(k)
        first = max(0, burn - r)
        if first < rows.shape[0]:
            d.accumulate(rows[first:])
        host.append(rows.cpu().numpy())
        r += rows.shape[0]; done += k
    res = d.result()
    chain = np.concatenate(host)[burn:]
    compare(res, chain, 4, 256)
    assert np.all(res["rhat"] < 1.01) and np.all(np.isfinite(res["ess"]))      # a well-started run of this pair has mixed


def test_hierarchical_sampler_streaming(gpu, dr_setup):
    from pyhillfit_amd import hierarchical as H
    from pyhillfit_amd.diagnostics import ChainDiagnostics
    dr = dr_setup
    ne, _, ex = dr.load_crumb_data("Amiodarone", "hERG")
    assert ne == 3
    s = H.HierarchicalSampler(H.PackedHierPoints([ex]), [0], 100, thinning=5, seed=3, problem_ids=[1], device=gpu)
    th0 = np.array([1., 5., 6., .3, 6., .8, 6.1, .7, 6.0, .9, 0.5])
    s.init(th0[None], cov_scale=0.01)
    saved = 4000 // 5 + 1
    d = ChainDiagnostics(1, 100, 12, saved - 1, 64, gpu)
    host = []
    for k in (1500, 1000, 1500):
        rows = s.advance(k)
        d.accumulate(rows)
        host.append(rows.cpu().numpy())
    compare(d.result(), np.concatenate(host), 12, 64)


def test_planted_non_convergence(gpu, dr_setup):
    from pyhillfit_amd import bestfit
    from pyhillfit_amd.diagnostics import ChainDiagnostics
    from pyhillfit_amd.sampler import SingleLevelSampler
    dr = dr_setup
    dr.define_model(2)
    ne, _, ex = dr.load_crumb_data("Amiodarone", "hERG")
    concs, y = dr.concatenate_experiments(ne, ex)
    th0 = bestfit.chain_start(bestfit.best_fit_batch([(concs, y)], 2)[0][0], 2)
    C = 128
    starts = np.tile(th0, (1, C, 1))
    starts[0, :C // 2, 0], starts[0, C // 2:, 0] = 3.0, 9.0
    s = SingleLevelSampler(dr.PackedPoints([(concs, y)]), 2, [0], [1.0], C, thinning=5, seed=7, adapt_start=3000, device=gpu)
    s.init(starts, cov_identity=False, cov_scale=0.05)
    rows = s.advance(500)                                   # 100 rows, no burn-in dropped: the chains are still apart
    d = ChainDiagnostics(1, C, 4, rows.shape[0], 256, gpu)
    d.accumulate(rows)
    res = d.result()
    assert res["rhat"][0, 0] > 1.1


def _summaries(root):
    return {p: json.load(open(p)) for p in sorted(glob.glob(os.path.join(root, "**", "*_summary.json"), recursive=True))}


@pytest.fixture(scope="module")
def csv_file(tmp_path_factory, gpu):
    from pyhillfit_amd import doseresponse as dr
    dr.setup(os.path.join(REPO, "data", "crumb_dataset.json"))
    p = tmp_path_factory.mktemp("data") / "crumb_data.csv"
    dr.table.to_csv(str(p))
    return str(p)


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k] == b[k], k


def test_single_level_cli(csv_file, tmp_path):
    from pyhillfit_amd import PyHillFit
    from pyhillfit_amd.chain_diagnostics import diagnose_file
    base = ["--data-file", csv_file, "-m", "2", "-i", "20000", "--drugs", "Amiodarone,Bepridil", "--channels", "hERG",
            "--num-chains", "64", "--segment", "7000", "--save-all-chains"]
    PyHillFit.main(base + ["--output-root", str(tmp_path / "on"), "--diagnostics"])
    PyHillFit.main(base + ["--output-root", str(tmp_path / "off")])
    on, off = _summaries(str(tmp_path / "on")), _summaries(str(tmp_path / "off"))
    assert len(on) == 2 and len(off) == 2
    for (p_on, s_on), s_off in zip(on.items(), off.values()):
        assert "diagnostics" not in s_off
        dg = s_on.pop("diagnostics")
        s_on.pop("mh_samples_per_second"); s_off.pop("mh_samples_per_second")
        assert s_on == s_off
        got = diagnose_file(p_on.replace("_summary.json", "_all_chains.npy"))
        for k in ("rhat", "ess", "mcse_mean", "lag_limit_reached", "lags", "rows_per_half_chain", "half_chains", "method"):
            assert dg[k] == got[k], k
        assert dg["half_chains"] == 128 and len(dg["rhat"]) == len(s_on["columns"])


def test_hierarchical_cli_one_chain_equals_chain_file(csv_file, tmp_path):
    from pyhillfit_amd import PyHillFit
    from pyhillfit_amd.chain_diagnostics import diagnose_file
    base = ["--data-file", csv_file, "-m", "2", "--hierarchical", "-i", "10000", "--drugs", "Amiodarone", "--channels", "hERG",
            "--segment", "3000"]
    PyHillFit.main(base + ["--num-chains", "1", "--output-root", str(tmp_path / "one"), "--diagnostics"])
    (p, s), = _summaries(str(tmp_path / "one")).items()
    got = diagnose_file(p.replace("_summary.json", ".txt"))
    assert got["kind"] == "hierarchical text"
    for k in ("rhat", "ess", "mcse_mean", "lag_limit_reached", "rows_per_half_chain", "half_chains"):
        assert s["diagnostics"][k] == got[k], k
    PyHillFit.main(base + ["--num-chains", "128", "--output-root", str(tmp_path / "many"), "--diagnostics"])
    (_, s), = _summaries(str(tmp_path / "many")).items()
    dg = s["diagnostics"]
    assert len(dg["rhat"]) == len(dg["columns"]) == 12 and all(v is not None and np.isfinite(v) for v in dg["rhat"])
    PyHillFit.main(base + ["--num-chains", "128", "--output-root", str(tmp_path / "off")])
    (_, s), = _summaries(str(tmp_path / "off")).items()
    assert "diagnostics" not in s


def test_pyhilltemp_cli(csv_file, tmp_path):
    from pyhillfit_amd import PyHillTemp
    base = ["--data-file", csv_file, "-m", "1", "-d", "0", "-c", "0", "-i", "3000", "-t", "5", "--rungs", "4", "--num-chains", "64"]
    res = PyHillTemp.main(base + ["--output-root", str(tmp_path / "on"), "--diagnostics"])
    assert len(res) == 5 and all(len(r["diagnostics"]["rhat"]) == 3 for r in res)
    (ti_on,) = glob.glob(str(tmp_path / "on" / "**" / "thermodynamic_integration.json"), recursive=True)
    ti = json.load(open(ti_on))
    assert len(ti["diagnostics"]) == 5 and all(d_["half_chains"] == 128 for d_ in ti["diagnostics"])
    PyHillTemp.main(base + ["--output-root", str(tmp_path / "off")])
    (ti_off,) = glob.glob(str(tmp_path / "off" / "**" / "thermodynamic_integration.json"), recursive=True)
    off = json.load(open(ti_off))
    assert "diagnostics" not in off
    ti.pop("diagnostics")
    assert ti == off
