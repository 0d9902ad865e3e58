"""WAIC on the GPU: the batch evaluator and the streaming accumulation (phf_pointwise_*, phf_waic_*) against the numpy restatement of
test_waic_host.py, bit-identical results however the rows are cut, the single-level sampler and the command lines."""
import glob
import json
import os

import numpy as np
import pytest
from scipy.special import logsumexp

from conftest import REPO
from test_waic_host import HALF_LN_2PI, hier_loglik, sl_loglik

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


def _close(got, want, rtol):
    """relative to max(|want|, 1): a log-likelihood near 0 has no relative accuracy to speak of"""
    got, want = np.asarray(got), np.asarray(want)
    assert np.all(np.isfinite(got) == np.isfinite(want))
    f = np.isfinite(want)
    err = np.abs(got[f] - want[f]) / np.maximum(np.abs(want[f]), 1.0)
    assert err.max(initial=0.0) <= rtol, err.max()


def _crumb_experiments(dr):
    """(experiments, labels) of every Crumb pair with data, in drug x channel order"""
    from pyhillfit_amd.PyHillFit import experiments_and_labels
    out = []
    for d in dr.drugs:
        for c in dr.channels:
            try:
                out.append(experiments_and_labels(d, c))
            except ValueError:
                continue
    return out


def crumb_single_level(dr):
    from pyhillfit_amd import waic as wc
    return wc.Points.single_level(*zip(*_crumb_experiments(dr)))


@pytest.mark.parametrize("model", [1, 2])
def test_batch_single_level_all_crumb_pairs(gpu, dr_setup, model):
    from pyhillfit_amd import sampler, waic as wc
    dr = dr_setup
    pts = crumb_single_level(dr)
    assert pts.num_problems == 210
    rng = np.random.default_rng(model)
    reps = 4
    pi = np.repeat(np.arange(pts.num_problems), reps)
    m = len(pi)
    theta = np.column_stack([rng.uniform(3, 9, m)] + ([rng.uniform(0.2, 4, m)] if model == 2 else []) + [rng.uniform(0.5, 40, m)])
    got = wc.pointwise_loglik(pts, model, pi, theta, gpu)
    # the sampler's own t = 1 likelihood of the same pairs (merged entries, pi_bit over all points)
    dr.define_model(model)
    packed = dr.PackedPoints([dr.concatenate_experiments(len(e), e) for e, _ in _crumb_experiments(dr)])
    lik, _ = sampler.log_target_batch(packed, model, pi.astype(np.int32), np.ones(m), theta)
    for i in range(m):
        q, n = pi[i], pts.count[pi[i]]
        conc, y = np.exp(pts.ln_conc[q, :n]), pts.response[q, :n]
        want = sl_loglik(model, conc, y, theta[i])
        _close(got[i, :n], want, 1e-12)
        assert np.all(np.isnan(got[i, n:]))
        n_unc = int(np.sum(pts.tag[q, :n] == 0))
        ident = lik[i] + (packed.counts[q, 3] - n_unc) * HALF_LN_2PI
        assert np.sum(got[i, :n]) == pytest.approx(ident, rel=1e-11, abs=1e-9)


def synthetic_pair(rng, sizes):
    """(experiments, truth): one pair with len(sizes) experiments of sizes[i] points — a common (pIC50, Hill, sigma), a per-experiment
    scatter of pIC50 and Hill, doses within 1.5 decades of the IC50, y = clip(Hill curve + sigma z, 0, 100)"""
    pic50, hill, sigma = rng.uniform(4.0, 7.0), rng.uniform(0.7, 1.5), rng.uniform(3.0, 8.0)
    expts = []
    for n in sizes:
        p_i, h_i = pic50 + rng.normal(0.0, 0.15), hill * np.exp(rng.normal(0.0, 0.1))
        dose = 10.0 ** (6.0 - p_i + rng.uniform(-1.5, 1.5, n))
        pred = 100.0 * (1.0 - 1.0 / (1.0 + (dose / 10.0 ** (6.0 - p_i)) ** h_i))
        expts.append(np.column_stack([dose, np.clip(pred + sigma * rng.standard_normal(n), 0.0, 100.0)]))
    return expts, (pic50, hill, sigma)


def synthetic_points(rng, counts, ne=None):
    from pyhillfit_amd import waic as wc
    per = []
    for n in counts:
        k = ne or 1
        sizes = np.full(k, n // k)
        sizes[: n % k] += 1
        expts = []
        for s in sizes:
            conc = 10.0 ** rng.uniform(-3, 2, s)
            y = rng.uniform(0.5, 99.5, s)
            if ne is None:
                y[rng.random(s) < 0.3] = 0.0
                y[rng.random(s) < 0.1] = 100.0
            expts.append(np.column_stack([conc, y]))
        per.append(expts)
    return wc.Points.hierarchical(per) if ne else wc.Points.single_level(per)


@pytest.mark.parametrize("ne", [3, 4, 5, 6, 1, 2, 8, 9, 64])        # the Crumb set's 3..6, then both ends of 1 <= Ne <= 64 and 8 | 9
def test_batch_hierarchical(gpu, ne):
    from pyhillfit_amd import waic as wc
    rng = np.random.default_rng(ne)
    pts = synthetic_points(rng, [ne * 4, ne * 4 + 1, ne * 2 + 3], ne)
    m = 300
    pi = rng.integers(0, pts.num_problems, m)
    theta = np.column_stack([rng.uniform(0.5, 2, m), rng.uniform(2.5, 5, m), rng.uniform(3, 8, m), rng.uniform(0.05, 1, m)]
                            + [c for _ in range(ne) for c in (rng.uniform(3, 9, m), rng.uniform(0.2, 4, m))] + [rng.uniform(0.5, 40, m)])
    got = wc.pointwise_loglik(pts, "hierarchical", pi, theta, gpu)
    for i in range(m):
        q, n = pi[i], pts.count[pi[i]]
        want = hier_loglik(np.exp(pts.ln_conc[q, :n]), pts.response[q, :n], pts.tag[q, :n], theta[i])
        _close(got[i, :n], want, 1e-12)


def synthetic_rows(rng, pts, kind, chains, rows, extra=3):
    """[rows][Q][cols + extra][chains]; the extra columns are NaN (never read)"""
    Q = pts.num_problems
    if kind == "hierarchical":
        ne = pts.num_expts
        cols = 5 + 2 * ne
        x = np.full((rows, Q, cols + extra, chains), np.nan)
        x[:, :, :4] = 1.0
        for i in range(ne):
            x[:, :, 4 + 2 * i] = rng.normal(5.5, 0.4, (rows, Q, chains))
            x[:, :, 5 + 2 * i] = rng.uniform(0.6, 1.6, (rows, Q, chains))
        x[:, :, 4 + 2 * ne] = rng.uniform(4, 12, (rows, Q, chains))
    else:
        cols = kind + 1
        x = np.full((rows, Q, cols + extra, chains), np.nan)
        x[:, :, 0] = rng.normal(5.5, 0.4, (rows, Q, chains))
        if kind == 2:
            x[:, :, 1] = rng.uniform(0.6, 1.6, (rows, Q, chains))
        x[:, :, kind] = rng.uniform(4, 12, (rows, Q, chains))
    return x


def restated_waic(pts, kind, x):
    """direct numpy LSE and variance over every draw of every chain: [Q] lists"""
    lse, var = [], []
    for q in range(pts.num_problems):
        n = pts.count[q]
        conc, y, tag = np.exp(pts.ln_conc[q, :n]), pts.response[q, :n], pts.tag[q, :n]
        draws = x[:, q].transpose(0, 2, 1).reshape(-1, x.shape[2])
        if kind == "hierarchical":
            ll = np.array([hier_loglik(conc, y, tag, th[:5 + 2 * pts.num_expts]) for th in draws])
        else:
            ll = np.array([sl_loglik(kind, conc, y, th[:kind + 1]) for th in draws])
        lse.append(logsumexp(ll, axis=0))
        var.append(np.var(ll, axis=0, ddof=1))
    return lse, var


def run_stream(pts, kind, x, cuts, device):
    from pyhillfit_amd import waic as wc
    rows, Q, _, C = x.shape
    w = wc.PointwiseWAIC(pts, kind, Q, C, rows, device)
    xt = torch.from_numpy(np.ascontiguousarray(x)).to(device)
    b = 0
    for e in list(cuts) + [rows]:
        w.accumulate(xt[b:e])
        b = e
    return w


@pytest.mark.parametrize("kind,chains,counts,rows", [(1, 70, [1, 5, 24], 37), (2, 1, [3, 26], 50), (2, 130, [9, 4], 21),
                                                     ("hierarchical", 65, [13, 24, 17], 29)])
def test_accumulation_matches_restatement(gpu, kind, chains, counts, rows):
    rng = np.random.default_rng(chains)
    pts = synthetic_points(rng, counts, 4 if kind == "hierarchical" else None)
    x = synthetic_rows(rng, pts, kind, chains, rows)
    lse, var = run_stream(pts, kind, x, [7, 8], gpu).reduced()
    want_lse, want_var = restated_waic(pts, kind, x)
    for q, n in enumerate(pts.count):
        _close(lse[q, :n], want_lse[q], 1e-10)
        np.testing.assert_allclose(var[q, :n], want_var[q], rtol=1e-10, atol=1e-14)


def test_segmentation_invariance(gpu):
    rng = np.random.default_rng(11)
    for kind, ne in ((2, None), ("hierarchical", 3)):
        pts = synthetic_points(rng, [7, 12, 22] if ne else [11, 23, 2], ne)
        x = synthetic_rows(rng, pts, kind, 100, 60)
        outs = [run_stream(pts, kind, x, cuts, gpu).reduced() for cuts in ([], [1, 2, 3, 30], [17, 59], list(range(1, 60)))]
        for o in outs[1:]:
            assert np.array_equal(o[0], outs[0][0]) and np.array_equal(o[1], outs[0][1])


def test_known_answers_on_device(gpu):
    """constant rows: p_waic = 0 exactly and lppd_i = l_i(theta); alternating rows: the closed forms"""
    from pyhillfit_amd import waic as wc
    rng = np.random.default_rng(5)
    pts = synthetic_points(rng, [9])
    ta, tb = np.array([5.2, 1.1, 6.0]), np.array([5.9, 0.8, 9.0])
    S = 40
    x = np.zeros((S, 1, 3, 1))
    x[:, 0, :, 0] = ta
    res = run_stream(pts, 2, x, [13], gpu).result()[0]
    la = wc.pointwise_loglik(pts, 2, [0], ta, gpu)[0, :9]
    lb = wc.pointwise_loglik(pts, 2, [0], tb, gpu)[0, :9]
    assert res["p_waic"] == 0.0
    np.testing.assert_allclose(res["lppd_i"], la, rtol=1e-13)
    x[1::2, 0, :, 0] = tb
    res = run_stream(pts, 2, x, [13], gpu).result()[0]
    np.testing.assert_allclose(res["lppd_i"], np.logaddexp(la, lb) - np.log(2), rtol=1e-12)
    np.testing.assert_allclose(res["p_waic_i"], (la - lb) ** 2 / 4 * S / (S - 1), rtol=1e-10)


def test_single_level_sampler_streaming(gpu, dr_setup):
    from pyhillfit_amd import bestfit, waic as wc
    from pyhillfit_amd.PyHillFit import experiments_and_labels
    from pyhillfit_amd.sampler import SingleLevelSampler
    dr = dr_setup
    dr.define_model(2)
    names = [("Amiodarone", "hERG"), ("Quinidine", "Nav1.5-late")]
    el = [experiments_and_labels(d, c) for d, c in names]
    data = [dr.concatenate_experiments(len(e), e) for e, _ in el]
    th0 = [bestfit.chain_start(t, 2) for t in bestfit.best_fit_batch(data, 2)[0]]
    s = SingleLevelSampler(dr.PackedPoints(data), 2, [0, 1], [1.0, 1.0], 96, thinning=5, seed=25, adapt_start=3000, device=gpu)
    s.init(np.array(th0), cov_identity=False, cov_scale=0.05)
    chain = s.run(6000, segment=2000)                                  # [rows][2][4][96], every row kept
    burn = chain.shape[0] // 4
    pts = wc.Points.single_level(*zip(*el))
    w = wc.PointwiseWAIC(pts, 2, 2, 96, chain.shape[0] - burn, gpu)
    w.accumulate(chain[burn:burn + 100].contiguous())
    w.accumulate(chain[burn + 100:].contiguous())
    lse, var = w.reduced()
    want_lse, want_var = restated_waic(pts, 2, chain[burn:].cpu().numpy())
    for q, n in enumerate(pts.count):
        _close(lse[q, :n], want_lse[q], 1e-10)
        np.testing.assert_allclose(var[q, :n], want_var[q], rtol=1e-9, atol=1e-13)


# ---- command lines -------------------------------------------------------------------------------------------------------------
def _summaries(root):
    return {p: json.load(open(p)) for p in sorted(glob.glob(os.path.join(root, "**", "*_summary.json"), recursive=True))}


def _chain_files(root):
    return {os.path.relpath(p, root): open(p, "rb").read() for p in sorted(glob.glob(os.path.join(root, "**", "*.txt"), recursive=True))}


@pytest.fixture(scope="module")
def csv_file(tmp_path_factory, gpu):
    from pyhillfit_amd import doseresponse as dr
    dr.setup(os.path.join(REPO, "data", "crumb_dataset.json"))
    p = tmp_path_factory.mktemp("data") / "crumb_data.csv"
    dr.table.to_csv(str(p))
    return str(p)


def test_single_level_cli_and_compare(csv_file, tmp_path, capsys):
    from pyhillfit_amd import PyHillFit, compare_models
    from pyhillfit_amd.chain_waic import waic_file
    base = ["--data-file", csv_file, "-i", "20000", "--drugs", "Amiodarone,Bepridil", "--channels", "hERG", "--num-chains", "64",
            "--segment", "7000"]
    PyHillFit.main(base + ["-m", "2", "--output-root", str(tmp_path / "on"), "--waic", "--save-all-chains"])
    PyHillFit.main(base + ["-m", "2", "--output-root", str(tmp_path / "off"), "--save-all-chains"])
    assert _chain_files(str(tmp_path / "on")) == _chain_files(str(tmp_path / "off"))
    on, off = _summaries(str(tmp_path / "on")), _summaries(str(tmp_path / "off"))
    assert len(on) == 2 and len(off) == 2
    for (p_on, s_on), s_off in zip(on.items(), off.values()):
        assert "waic" not in s_off
        w = s_on.pop("waic")
        s_on.pop("mh_samples_per_second"); s_off.pop("mh_samples_per_second")
        assert s_on == s_off
        assert w["draws"] == 64 * s_on["saved_rows_after_burn_in"] and w["n_points"] == len(w["pointwise"]["elpd"])
        got = waic_file(p_on.replace("_summary.json", "_all_chains.npy"))
        assert got["draws"] == w["draws"]
        for k in ("elpd_waic", "p_waic", "lppd"):
            assert got[k] == pytest.approx(w[k], rel=1e-12), k
    PyHillFit.main(base + ["-m", "1", "--output-root", str(tmp_path / "m1"), "--waic"])
    capsys.readouterr()
    rows = compare_models.main([str(tmp_path / "m1"), str(tmp_path / "on")])
    assert len(rows) == 2
    for r in rows:
        assert "error" not in r and r["n_mixed"] == 0 and "warning" not in r and np.isfinite(r["elpd_diff"])
    assert json.loads(capsys.readouterr().out)["comparisons"] == rows


def test_hierarchical_cli_fused_on_off(csv_file, tmp_path):
    from pyhillfit_amd import PyHillFit
    base = ["--data-file", csv_file, "-m", "2", "--hierarchical", "-i", "6000", "--drugs", "Amiodarone,Bepridil,Quinidine",
            "--channels", "hERG,Cav1.2", "--segment", "2000", "--waic"]
    PyHillFit.main(base + ["--fused-launch", "on", "--output-root", str(tmp_path / "on")])
    PyHillFit.main(base + ["--fused-launch", "off", "--output-root", str(tmp_path / "off")])
    PyHillFit.main(base[:-1] + ["--fused-launch", "on", "--output-root", str(tmp_path / "plain")])
    on, off, plain = _summaries(str(tmp_path / "on")), _summaries(str(tmp_path / "off")), _summaries(str(tmp_path / "plain"))
    assert len(on) == len(off) == len(plain) > 1
    assert _chain_files(str(tmp_path / "on")) == _chain_files(str(tmp_path / "plain"))
    for s_on, s_off, s_plain in zip(on.values(), off.values(), plain.values()):
        assert s_on["waic"] == s_off["waic"]
        assert set(s_on["waic"]["points"]["kind"]) == {"truncated"}
        assert set(s_on) - set(s_plain) == {"waic"}
