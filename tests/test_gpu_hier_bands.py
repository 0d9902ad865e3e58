"""Hierarchical dose-response bands on the GPU (phf_hier_band_draws, phf_quantiles_accumulate_hier_curves): the device draws equal
the host build of phf_hier_bands.h bit for bit, the band histograms equal the numpy restatement of test_quantiles_host.py fed with
the host's curve values count for count, results are bit-identical however the rows are cut, the brackets hold the exact sample
quantiles of sampler runs, the draws agree with the predictive CDFs, and --predictive-bands against chain_quantiles --hier-bands."""
import os

import numpy as np
import pytest

from test_gpu_waic import _chain_files, _summaries, csv_file, dr_setup, gpu  # noqa: F401
from test_hier_bands_host import build_shim, host_band_values, host_draws, sup_distance
from test_quantiles_host import Histogram

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PROBS = (0.0, 0.025, 0.05, 0.25, 0.5, 0.75, 0.95, 0.975, 1.0)
PIDS = (7, 0, 209)
CHAIN_BASE = 1000
SEED = 25
DRAW_ROWS = 45                            # 96 chains x 3 problems x 45 rows = 12 960 draws: the DKW argument of the distribution tests


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shim(tmp_path_factory.mktemp("hier_bands_gpu"))


def band_rows(rng, rows, Q, chains, stride=8):
    """[rows][Q][stride][chains] hierarchical rows with valid (alpha, beta, mu, s); the columns after them are never read"""
    x = np.full((rows, Q, stride, chains), np.nan)
    x[:, :, 0] = rng.uniform(0.3, 3, (rows, Q, chains))
    x[:, :, 1] = rng.uniform(0.5, 20, (rows, Q, chains))
    x[:, :, 2] = rng.uniform(2, 9, (rows, Q, chains))
    x[:, :, 3] = rng.uniform(0.05, 2, (rows, Q, chains))
    return x


def vectors_of(x, first_row):
    """(theta [m][4], counters [m][3]) of every (row, problem, chain) of x, the stream addressed as the accumulation addresses it"""
    rows, Q, _, chains = x.shape
    r, q, c = np.meshgrid(np.arange(rows), np.arange(Q), np.arange(chains), indexing="ij")
    theta = x[:, :, :4, :].transpose(0, 1, 3, 2).reshape(-1, 4)
    ctr = np.stack([CHAIN_BASE + c.ravel(), np.array(PIDS)[q.ravel()], first_row + r.ravel()], axis=1)
    return theta, ctr


# ---- 8. the draws --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chains", [5, 96])
@pytest.mark.parametrize("first_row", [0, 12345])
def test_draws_equal_the_host_bit_for_bit(gpu, shim, chains, first_row):
    from pyhillfit_amd.quantiles import hier_band_draws
    x = band_rows(np.random.default_rng(chains), DRAW_ROWS, 3, chains)
    theta, ctr = vectors_of(x, first_row)
    assert theta.shape[0] == chains * 3 * DRAW_ROWS
    theta = theta.copy()
    for i, (col, bad) in enumerate([(0, np.nan), (1, np.nan), (2, np.nan), (3, np.nan), (0, 0.0), (1, 0.0), (3, 0.0), (0, -1.5), (1, -0.5),
                                    (3, -2.0), (0, np.inf), (1, np.inf), (2, -np.inf), (3, np.inf)]):
        theta[3 * i + 1, col] = bad
    got, want = hier_band_draws(theta, ctr, SEED, gpu), host_draws(shim, theta, ctr, SEED)
    bad = np.zeros(len(theta), dtype=bool)
    bad[1:3 * 14:3] = True
    assert np.all(np.isnan(got[bad])) and np.all(np.isfinite(got[~bad]))
    assert np.array_equal(got, want, equal_nan=True)
    assert np.array_equal(got[~bad].view(np.uint64), want[~bad].view(np.uint64))


# ---- 9, 10. the histograms -----------------------------------------------------------------------------------------------------
def hist_rows(rng, chains):
    """300 rows x 3 problems, stride 8: valid rows, some draws with a NaN alpha, problem 2 NaN throughout"""
    x = band_rows(rng, 300, 3, chains)
    a = x[:, 0, 0]
    a[rng.random(a.shape) < 0.02] = np.nan
    x[0, 0, 0, 0] = np.nan                                              # the very first draw: the anchor is a later one
    x[7, 1, 1, chains - 1] = -1.0                                       # a negative beta
    x[9, 1, 3, 0] = 0.0                                                 # s = 0: no future experiment, the underlying effect stands
    x[:, 2, 0] = np.nan
    return x


def hist_doses():
    """D = 5 per problem: G = 3 grid doses, then 2 named concentrations"""
    from pyhillfit_amd.quantiles import band_doses
    return np.stack([band_doses(c, 3, (0.1, 10.0)) for c in ([0.1, 1.0, 30.0], [0.03, 3.0], [1.0, 100.0])])


def run_bands(x, ln_doses, cuts, device, bins, first_cols=4, probs=PROBS):
    from pyhillfit_amd.quantiles import PosteriorQuantiles
    q = PosteriorQuantiles(x.shape[1], x.shape[3], first_cols, x.shape[0], probs, bins, device, band_ln_doses=ln_doses, seed=SEED,
                           problem_ids=PIDS[:x.shape[1]], chain_id_base=CHAIN_BASE)
    t = torch.from_numpy(x).to(device)
    for part in np.split(np.arange(x.shape[0]), cuts):
        if part.size:
            q.accumulate(t[part[0]:part[-1] + 1].contiguous())
    return q


@pytest.mark.parametrize("chains,bins", [(5, 64), (96, 4096), (96, 64), (5, 4096)])
def test_band_counts_equal_restatement(gpu, shim, chains, bins):
    x = hist_rows(np.random.default_rng(100 + chains), chains)
    ln_doses = np.log(hist_doses())
    cuts = [1, 50, 51, 200]
    qs = run_bands(x, ln_doses, cuts, gpu, bins)
    counts, nf = qs.counts()
    res = qs.result()
    values = host_band_values(shim, x, ln_doses, PIDS, CHAIN_BASE, SEED)      # [Q][2 D][rows][chains]
    D = ln_doses.shape[1]
    assert counts.shape == (3, 4 + 2 * D, bins) and res["band_doses"] == D
    for q in range(3):
        for s in range(2 * D):
            h = Histogram(bins)
            for part in np.split(np.arange(x.shape[0]), cuts):
                h.feed(values[q, s, part])
            c = 4 + s
            assert np.array_equal(counts[q, c], h.counts), (q, s)
            assert nf[q, c] == h.nonfinite and res["non_finite"][q, c] == h.nonfinite
            if q == 2:                                                  # nothing finite: never anchored
                assert h.nonfinite == 300 * chains and np.isnan(res["min"][q, c]) and np.all(np.isnan(res["value"][q, c]))
                continue
            assert res["level"][q, c] == h.k and res["min"][q, c] == h.mn and res["max"][q, c] == h.mx
            assert res["bin_width"][q, c] == h.width
            got = np.stack([res["value"][q, c], res["lo"][q, c], res["hi"][q, c], res["bin"][q, c]], axis=1)
            assert np.array_equal(got, h.quantiles(PROBS)), (q, s)
            v = values[q, s]
            exact = np.quantile(v[np.isfinite(v)], PROBS, method="inverted_cdf")
            assert np.all(res["lo"][q, c] <= exact) and np.all(exact <= res["hi"][q, c])
    # s = 0 takes one draw from the future experiment only; NaN alphas from both
    assert np.all(nf[1, 4 + D:] == nf[1, 4:4 + D] + 1) and np.all(nf[0, 4:] == nf[0, 4])
    # the columns of the same workspace are the plain column quantiles
    for q in range(2):
        h = Histogram(bins)
        for part in np.split(np.arange(x.shape[0]), cuts):
            h.feed(x[part, q, 1, :])
        assert np.array_equal(counts[q, 1], h.counts)


def test_band_segmentation_bit_identical(gpu):
    x = hist_rows(np.random.default_rng(11), 96)
    ln_doses = np.log(hist_doses())
    ref = run_bands(x, ln_doses, [], gpu, 4096)
    want, wc = ref.reduced(), ref.counts()
    assert np.all(want[:2, 4:, 2] > 0)
    for cuts in ([1], [3, 4, 5, 250], list(range(37, 300, 37))):
        q = run_bands(x, ln_doses, cuts, gpu, 4096)
        assert np.array_equal(q.reduced(), want, equal_nan=True)
        got = q.counts()
        assert np.array_equal(got[0], wc[0]) and np.array_equal(got[1], wc[1])


# ---- 11. the sampler end to end --------------------------------------------------------------------------------------------------
def test_hierarchical_sampler_bands(gpu, shim, dr_setup):
    from pyhillfit_amd import hierarchical as H
    from pyhillfit_amd import quantiles as qn
    dr = dr_setup
    by_ne = {}
    for d in dr.drugs:
        for c in dr.channels:
            try:
                ne, _, ex = dr.load_crumb_data(d, c)
            except Exception:
                continue
            by_ne.setdefault(ne, ex)
    B = 16384
    for ne in (3, 4):
        ex = by_ne[ne]
        s = H.HierarchicalSampler(H.PackedHierPoints([ex]), [0], 100, thinning=5, seed=3, problem_ids=[1], device=gpu)
        th0 = np.array([1., 5., 6., .3] + [6., .8] * ne + [0.5])
        s.init(th0[None], cov_scale=0.01)
        doses = qn.band_doses(np.concatenate([np.asarray(e)[:, 0] for e in ex]), 4, (0.1, 10.0))
        ln_doses = np.log(doses)[None]
        q = qn.PosteriorQuantiles(1, 100, 6 + 2 * ne, 4000 // 5, PROBS, B, gpu, band_ln_doses=ln_doses, seed=SEED, problem_ids=[1],
                                  chain_id_base=0)
        rows_all = []
        for k in (1500, 1000, 1500):
            rows = s.advance(k)
            q.accumulate(rows)
            rows_all.append(rows.cpu().numpy())
        res = q.result()
        chain = np.concatenate(rows_all)
        assert chain.shape[0] == 800
        values = host_band_values(shim, chain, ln_doses, [1], 0, SEED)
        c0 = 6 + 2 * ne
        for slot in range(12):
            v = values[0, slot].ravel()
            c = c0 + slot
            assert res["draws"][0, c] == 800 * 100 == v.size and res["non_finite"][0, c] == 0
            exact = np.quantile(v, PROBS, method="inverted_cdf")
            assert np.all(res["lo"][0, c] <= exact) and np.all(exact <= res["hi"][0, c]), (ne, slot)
            assert res["min"][0, c] == v.min() and res["max"][0, c] == v.max()
            if res["level"][0, c] > 0:
                assert res["bin_width"][0, c] <= 4 * (res["max"][0, c] - res["min"][0, c]) / B
        rec = qn.hier_band_record(res, 0, doses, 4)
        assert rec["named_concentrations"] == [0.1, 10.0] and len(rec["future_experiment"]["value"]) == 6


# ---- 12. against the predictive CDFs (the path golden G7 pins) ---------------------------------------------------------------------
def test_draws_against_predictive_curves(gpu):
    """the 12 960 device draws of the 96-chain rows of the draw test against the mean log-logistic / logistic CDFs PredictiveCurves
    accumulates from the same rows; DKW: P(sup > 0.03) <= 2 exp(-2 12960 0.03^2) = 1.5e-10"""
    from pyhillfit_amd.predictive import PredictiveCurves
    from pyhillfit_amd.quantiles import hier_band_draws
    x = band_rows(np.random.default_rng(96), DRAW_ROWS, 3, 96)
    theta, ctr = vectors_of(x, 0)
    d = hier_band_draws(theta, ctr, SEED, gpu)
    assert d.shape == (12960, 2) and np.all(np.isfinite(d))
    pc = PredictiveCurves(3, gpu)
    pc.accumulate(torch.from_numpy(x).to(gpu))
    m = pc.means().cpu().numpy().mean(axis=0)                           # the problems hold equally many draws: [4][G]
    for col, grid, cdf in ((0, pc.hill_x_host, m[0]), (1, pc.pic50_x_host, m[1])):
        emp = np.searchsorted(np.sort(d[:, col]), grid, side="right") / d.shape[0]
        assert np.max(np.abs(emp - cdf)) <= 0.03, col
    assert sup_distance(d[:, 1], lambda g: np.interp(g, pc.pic50_x_host, m[1])) <= 0.03


# ---- 13. the command lines ---------------------------------------------------------------------------------------------------------
def test_hierarchical_cli_and_chain_tool(csv_file, tmp_path, capsys):  # noqa: F811
    from pyhillfit_amd import PyHillFit, chain_quantiles
    from pyhillfit_amd import doseresponse as dr
    base = ["--data-file", csv_file, "-m", "2", "--hierarchical", "-i", "6000", "--drugs", "Amiodarone", "--channels", "hERG",
            "--num-chains", "1", "--segment", "2000", "--quantiles"]
    PyHillFit.main(base + ["--output-root", str(tmp_path / "on"), "--predictive-bands", "8", "--band-concs", "0.1,10"])
    out_on = capsys.readouterr().out
    PyHillFit.main(base + ["--output-root", str(tmp_path / "off")])
    out_off = capsys.readouterr().out
    assert "non-finite band draws" in out_on and "band draws" not in out_off
    on_files, off_files = _chain_files(str(tmp_path / "on")), _chain_files(str(tmp_path / "off"))
    assert on_files and on_files == off_files                              # byte-identical chain (and sample) files
    on, off = _summaries(str(tmp_path / "on")), _summaries(str(tmp_path / "off"))
    assert len(on) == 1 and len(off) == 1
    (path, s_on), s_off = next(iter(on.items())), next(iter(off.values()))
    assert "hierarchical_bands" not in s_off
    band = s_on.pop("hierarchical_bands")
    s_on.pop("mh_samples_per_second"); s_off.pop("mh_samples_per_second")
    assert s_on == s_off
    assert len(band["doses"]) == 10 and band["grid_points"] == 8 and band["named_concentrations"] == [0.1, 10.0]
    assert band["doses"][8:] == [0.1, 10.0] and band["seed"] == 25
    P = len(band["probs"])
    for name in ("underlying", "future_experiment"):
        part = band[name]
        assert len(part["value"]) == 10 and part["non_finite"] == [0] * 10
        for g in range(7):                                              # every quantile is non-decreasing in dose, up to its brackets
            for p in range(P):
                assert part["lo"][g][p] <= part["hi"][g + 1][p], (name, g, p)
        for g in range(10):
            assert 0.0 <= part["min"][g] <= part["lo"][g][0] <= part["hi"][g][P - 1] <= part["max"][g] <= 100.0
    chain_file = path.replace("_summary.json", ".txt")
    assert os.path.exists(chain_file)
    pid = [(d, c) for d in dr.drugs for c in dr.channels].index(("Amiodarone", "hERG"))
    rec = chain_quantiles.main([chain_file, "--hier-bands", "8", "--band-concs", "0.1,10", "--data-file", csv_file, "--seed", "25",
                                "--problem-id", str(pid)])[0]
    assert rec["drug"] == "Amiodarone" and rec["channel"] == "hERG" and rec["problem_id"] == pid
    assert rec["hierarchical_bands"] == band
    # another seed is another future experiment, the same underlying effect
    other = chain_quantiles.main([chain_file, "--hier-bands", "8", "--band-concs", "0.1,10", "--data-file", csv_file, "--seed", "26"])[0]
    assert other["hierarchical_bands"]["underlying"] == band["underlying"]
    assert other["hierarchical_bands"]["future_experiment"] != band["future_experiment"]
