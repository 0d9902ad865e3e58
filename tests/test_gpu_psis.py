"""PSIS-LOO on the GPU (phf_psis_*): the device tail is bit-identical to np.sort of the batch evaluator's log-likelihoods, k-hat, sigma-hat
and elpd_loo agree with the numpy restatement of test_psis_host.py, results are bit-identical however the rows are cut, the HBM sort
path, the undetermined-point rule, the single-level sampler and the command lines."""
import glob
import json
import os

import numpy as np
import pytest

from conftest import REPO
from test_gpu_waic import _chain_files, _summaries, csv_file, dr_setup, gpu, synthetic_points, synthetic_rows  # noqa: F401
from test_psis_host import psis_loo, tail_length

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _rel(got, want, rtol):
    """relative to max(|want|, 1); infinities and NaN must match"""
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
    assert np.array_equal(got[np.isinf(want)], want[np.isinf(want)])
    f = np.isfinite(want)
    err = np.abs(got[f] - want[f]) / np.maximum(np.abs(want[f]), 1.0)
    assert err.max(initial=0.0) <= rtol, err.max()


def evaluator_ll(pts, kind, x, device):
    """per problem q, [n_q][S]: the batch evaluator's log-likelihood of every draw of x [rows][Q][cols + extra][C]"""
    from pyhillfit_amd import waic as wc
    cols = wc.columns_read(kind, pts)
    out = []
    for q in range(pts.num_problems):
        th = x[:, q, :cols].transpose(0, 2, 1).reshape(-1, cols)
        ll = wc.pointwise_loglik(pts, kind, np.full(th.shape[0], q), th, device)
        out.append(ll[:, :pts.count[q]].T.copy())
    return out


def run_stream(pts, kind, x, cuts, device, tail_per_chain=0):
    from pyhillfit_amd import loo
    rows, Q, _, C = x.shape
    w = loo.PointwiseLOO(pts, kind, Q, C, rows, device, tail_per_chain)
    xt = torch.from_numpy(np.ascontiguousarray(x)).to(device)
    b = 0
    for e in list(cuts) + [rows]:
        w.accumulate(xt[b:e])
        b = e
    return w


def check_against_restatement(pts, kind, x, w, device, allow_undetermined=False):
    """every point against the restatement; with allow_undetermined, a point may instead be undetermined (all NaN) if some chain
    holds at least tail_per_chain of its M + 1 smallest draws (the exactness rule's necessary condition)"""
    r = w.reduced(tail=True)
    lls = evaluator_ll(pts, kind, x, device)
    M = tail_length(x.shape[0] * x.shape[3])
    assert w.M == M
    C = x.shape[3]
    for q, n in enumerate(pts.count):
        assert np.all(r["determined"][q, n:] == 0.0)
        for p in range(n):
            if r["determined"][q, p] != 1.0:
                assert allow_undetermined and r["determined"][q, p] == 0.0
                assert np.all(np.isnan([r[k][q, p] for k in ("elpd_loo", "lppd", "khat", "sigma")]))
                per_chain = np.bincount(np.argsort(lls[q][p], kind="stable")[:M + 1] % C, minlength=C)
                assert per_chain.max() >= w.k
                continue
            want = psis_loo(lls[q][p])
            assert np.array_equal(r["tail"][q, p], np.sort(lls[q][p])[:M + 1])       # bit-identical
            _rel(r["elpd_loo"][q, p], want["elpd"], 1e-10)
            _rel(r["lppd"][q, p], want["lppd"], 1e-10)
            _rel(r["khat"][q, p], want["khat"], 1e-10)
            _rel(r["sigma"][q, p], want["sigma"], 1e-10)
    return r


@pytest.mark.parametrize("kind,chains,counts,rows", [(1, 70, [1, 5, 24], 37), (2, 130, [9, 4], 21), (2, 1, [3, 26], 400),
                                                     ("hierarchical", 65, [13, 24, 17], 29)])
def test_accumulation_matches_restatement(gpu, kind, chains, counts, rows):
    rng = np.random.default_rng(chains + rows)
    pts = synthetic_points(rng, counts, 4 if kind == "hierarchical" else None)
    x = synthetic_rows(rng, pts, kind, chains, rows)
    check_against_restatement(pts, kind, x, run_stream(pts, kind, x, [7, 8], gpu), gpu)


@pytest.mark.parametrize("ne", [3, 5, 6, 1, 2, 9])
def test_hierarchical_ne(gpu, ne):
    rng = np.random.default_rng(40 + ne)
    pts = synthetic_points(rng, [ne * 3, ne * 2 + 1], ne)
    x = synthetic_rows(rng, pts, "hierarchical", 67, 23)
    check_against_restatement(pts, "hierarchical", x, run_stream(pts, "hierarchical", x, [11], gpu), gpu)


def test_segmentation_invariance(gpu):
    rng = np.random.default_rng(21)
    for kind, ne in ((2, None), ("hierarchical", 3)):
        pts = synthetic_points(rng, [7, 12, 22] if ne else [11, 23, 2], ne)
        x = synthetic_rows(rng, pts, kind, 100, 60)
        outs = [run_stream(pts, kind, x, cuts, gpu).reduced(tail=True) for cuts in ([], [1, 2, 3, 30], [17, 59], list(range(1, 60)))]
        for o in outs[1:]:
            for k in o:
                assert np.array_equal(o[k], outs[0][k], equal_nan=True), k


def test_threshold_blocks(gpu):
    """runs longer than the 1024-row blocks after which T (the bound on the cutoff) is recomputed: bit-identical over cuts that do and
    do not fall on block edges, and equal to the restatement, at the default capacity (M + 1) and at a small one"""
    rng = np.random.default_rng(31)
    pts = synthetic_points(rng, [5, 3])
    x = synthetic_rows(rng, pts, 2, 64, 3000)
    for k in (0, 40):
        outs = [run_stream(pts, 2, x, cuts, gpu, k) for cuts in ([], [1024, 2048], [1000, 1025, 2047, 2999], [7, 1500])]
        red = [w.reduced(tail=True) for w in outs]
        for o in red[1:]:
            for key in o:
                assert np.array_equal(o[key], red[0][key], equal_nan=True), key
        assert np.array_equal(outs[1].insertions(), outs[2].insertions())
        check_against_restatement(pts, 2, x, outs[0], gpu, allow_undetermined=k != 0)
    x = synthetic_rows(rng, pts, 2, 64, 10000)                        # past row 8192, where T is recomputed every 8192 rows
    outs = [run_stream(pts, 2, x, cuts, gpu) for cuts in ([], [8192], [8000, 8193, 9999])]
    red = [w.reduced(tail=True) for w in outs]
    for o in red[1:]:
        for key in o:
            assert np.array_equal(o[key], red[0][key], equal_nan=True), key
    check_against_restatement(pts, 2, x, outs[0], gpu)


def test_hbm_sort_path(gpu):
    """M + 1 > 8192 (the reduce's LDS tail): the sort runs in the workspace's HBM scratch"""
    rng = np.random.default_rng(8)
    pts = synthetic_points(rng, [3, 2])
    chains, rows = 1000, 7500
    x = synthetic_rows(rng, pts, 1, chains, rows, extra=0)
    assert tail_length(chains * rows) + 1 > 8192
    check_against_restatement(pts, 1, x, run_stream(pts, 1, x, [2500], gpu), gpu)


def test_one_chain_holds_the_tail(gpu):
    """chain 0 holds 110 of the M + 1 = 270 smallest l (its share is 68): with 80 kept per chain the point is not determined; with
    168 (2 ceil(270/4) + 32, the fallback rule) and with the default (M + 1) it is, and equals the restatement"""
    from pyhillfit_amd import loo
    pts = synthetic_points(np.random.default_rng(0), [1])
    pts.response[0, 0], pts.tag[0, 0] = 50.0, 0
    rng = np.random.default_rng(5)
    chains, rows = 4, 2000
    x = np.zeros((rows, 1, 2, chains))
    x[:, 0, 0] = rng.normal(6.0, 0.1, (rows, chains))
    x[:, 0, 1] = rng.uniform(8.0, 12.0, (rows, chains))
    bad = rng.choice(rows, 110, replace=False)
    x[bad, 0, 0, 0] = rng.uniform(1.0, 2.0, 110)                      # a poor fit of the point: l near -5000
    x[bad, 0, 1, 0] = 0.5
    assert tail_length(chains * rows) == 269 and loo.tail_capacity(1, 1, chains, rows) == 270
    r = run_stream(pts, 1, x, [900], gpu, tail_per_chain=80).reduced()
    assert r["determined"][0, 0] == 0.0 and np.all(np.isnan([r[k][0, 0] for k in ("elpd_loo", "lppd", "khat", "sigma")]))
    res = run_stream(pts, 1, x, [900], gpu, tail_per_chain=80).result()[0]
    assert res["n_undetermined"] == 1 and np.isnan(res["elpd_loo"])
    check_against_restatement(pts, 1, x, run_stream(pts, 1, x, [900], gpu, tail_per_chain=168), gpu)
    check_against_restatement(pts, 1, x, run_stream(pts, 1, x, [900], gpu), gpu)


def test_known_answers_on_device(gpu):
    """constant rows: elpd_loo_i == lppd_i exactly, k-hat 0; S = 20 (M = 4): k-hat +inf; a draw with sigma <= 1e-3: elpd_loo_i -inf"""
    rng = np.random.default_rng(5)
    pts = synthetic_points(rng, [9])
    x = np.zeros((300, 1, 3, 7))
    x[:, 0] = np.array([5.2, 1.1, 6.0])[:, None]
    r = run_stream(pts, 2, x, [13], gpu).reduced()
    assert np.array_equal(r["elpd_loo"][0, :9], r["lppd"][0, :9]) and np.all(r["khat"][0, :9] == 0.0)
    x = synthetic_rows(rng, pts, 2, 2, 10)
    w = run_stream(pts, 2, x, [3], gpu)
    assert w.M == 4
    r = check_against_restatement(pts, 2, x, w, gpu)
    assert np.all(r["khat"][0, :9] == np.inf)
    x = synthetic_rows(rng, pts, 2, 65, 30)
    x[17, 0, 2, 3] = 1e-3
    r = check_against_restatement(pts, 2, x, run_stream(pts, 2, x, [5], gpu), gpu)
    assert np.all(r["elpd_loo"][0, :9] == -np.inf) and np.all(r["khat"][0, :9] == np.inf)


def test_single_level_sampler_streaming(gpu, dr_setup):
    from pyhillfit_amd import bestfit, loo, waic as wc
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
    x = chain[burn:].cpu().numpy()
    M = tail_length(x.shape[0] * 96)
    # a short run: the chains have not mixed, so one chain can hold more than the fallback capacity 2 ceil((M + 1)/C) + 32 of a
    # point's tail (undetermined); the default here is M + 1 per chain: every point exact by construction
    for k in (2 * -(-(M + 1) // 96) + 32, 0):
        w = loo.PointwiseLOO(pts, 2, 2, 96, chain.shape[0] - burn, gpu, tail_per_chain=k)
        w.accumulate(chain[burn:burn + 100].contiguous())
        w.accumulate(chain[burn + 100:].contiguous())
        ins = w.insertions()
        assert np.all(ins[0, :pts.count[0]] >= w.k)
        r = check_against_restatement(pts, 2, x, w, gpu, allow_undetermined=k != 0)
        if not k:
            assert w.k == M + 1
            assert np.all(r["determined"][np.arange(pts.stride)[None, :] < pts.count[:, None]] == 1.0)


# ---- command lines -------------------------------------------------------------------------------------------------------------
def test_single_level_cli_and_compare(csv_file, tmp_path, capsys):  # noqa: F811
    from pyhillfit_amd import PyHillFit, compare_models
    from pyhillfit_amd.chain_loo import loo_file
    base = ["--data-file", csv_file, "-i", "20000", "--drugs", "Amiodarone,Bepridil", "--channels", "hERG", "--num-chains", "64",
            "--segment", "7000"]
    PyHillFit.main(base + ["-m", "2", "--output-root", str(tmp_path / "on"), "--loo", "--save-all-chains"])
    PyHillFit.main(base + ["-m", "2", "--output-root", str(tmp_path / "off"), "--save-all-chains"])
    assert _chain_files(str(tmp_path / "on")) == _chain_files(str(tmp_path / "off"))
    on, off = _summaries(str(tmp_path / "on")), _summaries(str(tmp_path / "off"))
    assert len(on) == 2 and len(off) == 2
    for (p_on, s_on), s_off in zip(on.items(), off.values()):
        assert "loo" not in s_off and "waic" not in s_on
        w = s_on.pop("loo")
        s_on.pop("mh_samples_per_second"); s_off.pop("mh_samples_per_second")
        assert s_on == s_off
        assert w["draws"] == 64 * s_on["saved_rows_after_burn_in"] and w["n_points"] == len(w["pointwise"]["elpd_loo"])
        assert w["n_undetermined"] == 0 and w["elpd_loo"] is not None and w["tail_per_chain"] == w["tail_length"] + 1
        got = loo_file(p_on.replace("_summary.json", "_all_chains.npy"))
        for k in ("elpd_loo", "p_loo", "lppd", "max_khat", "n_undetermined"):
            assert (got[k] is None and w[k] is None) or got[k] == pytest.approx(w[k], rel=1e-12), k
    # a capacity of M + 1 per chain (the request is capped there): every point exact, so the comparison has no refusals
    exact = ["--loo", "--loo-tail-per-chain", "1000000"]
    PyHillFit.main(base + ["-m", "1", "--output-root", str(tmp_path / "m1")] + exact)
    PyHillFit.main(base + ["-m", "2", "--output-root", str(tmp_path / "m2")] + exact)
    capsys.readouterr()
    rows = compare_models.main([str(tmp_path / "m1"), str(tmp_path / "m2"), "--criterion", "loo"])
    assert len(rows) == 2
    for r in rows:
        assert "error" not in r and r["n_mixed"] == 0 and np.isfinite(r["elpd_diff"]) and "khat_flagged" in r
    assert json.loads(capsys.readouterr().out)["comparisons"] == rows


def test_hierarchical_cli_fused_on_off(csv_file, tmp_path):  # noqa: F811
    from pyhillfit_amd import PyHillFit, compare_models
    base = ["--data-file", csv_file, "-m", "2", "--hierarchical", "-i", "6000", "--drugs", "Amiodarone,Bepridil,Quinidine",
            "--channels", "hERG,Cav1.2", "--segment", "2000", "--loo"]
    PyHillFit.main(base + ["--fused-launch", "on", "--output-root", str(tmp_path / "on")])
    PyHillFit.main(base + ["--fused-launch", "off", "--output-root", str(tmp_path / "off")])
    PyHillFit.main(base[:-1] + ["--fused-launch", "on", "--output-root", str(tmp_path / "plain")])
    on, off, plain = _summaries(str(tmp_path / "on")), _summaries(str(tmp_path / "off")), _summaries(str(tmp_path / "plain"))
    assert len(on) == len(off) == len(plain) > 1
    assert _chain_files(str(tmp_path / "on")) == _chain_files(str(tmp_path / "plain"))
    assert _chain_files(str(tmp_path / "off")) == _chain_files(str(tmp_path / "plain"))
    for s_on, s_off, s_plain in zip(on.values(), off.values(), plain.values()):
        assert s_on["loo"] == s_off["loo"] and s_on["loo"]["n_undetermined"] == 0
        assert set(s_on["loo"]["points"]["kind"]) == {"truncated"}
        assert set(s_on) - set(s_plain) == {"loo"}
    rows = compare_models.main([str(tmp_path / "on"), str(tmp_path / "off"), "--criterion", "loo"])
    assert len(rows) == len(on) and all("error" not in r and r["elpd_diff"] == 0.0 for r in rows)
