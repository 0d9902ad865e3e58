"""Posterior correlations on the GPU: the co-moment kernels against the host build of phf_comoments.h bit for bit (small-d and tiled
paths, ragged tiles, more than one chain block, calls that hold the half boundary and the dropped middle row), segmentation, the
diagonals against the diagnostics, both samplers through the analysis set, the command line end to end and the chain-file tool."""
import contextlib
import glob
import io
import json
import os

import numpy as np
import pytest

import comoments_twin as tw
from conftest import REPO

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return "cuda:0"


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return tw.build_shim(tmp_path_factory.mktemp("comoments"))


@pytest.fixture(scope="module")
def dr_setup():
    from pyhillfit_amd import doseresponse as dr
    dr.setup(os.path.join(REPO, "data", "crumb_dataset.json"))
    return dr


def device_run(rows, d, cuts, gpu):
    """the whole run in calls cut at the row indices `cuts` -> (workspace [Q][2][F][C], reduced [Q][out])"""
    from pyhillfit_amd.correlations import PosteriorCorrelations
    N, Q, _, Cn = rows.shape
    acc = PosteriorCorrelations(Q, Cn, d, N, gpu)
    x = torch.from_numpy(rows).to(gpu)
    lo = 0
    for hi in list(cuts) + [N]:
        acc.accumulate(x[lo:hi].contiguous())
        lo = hi
    out = acc.workspace(), acc.reduced()
    acc.free()
    return out


# ---- 1. device = twin, bit for bit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q,d,Cn,N", [(2, 2, 5, 9), (2, 3, 64, 8), (1, 11, 96, 33), (1, 17, 70, 40), (1, 133, 3, 10)])
def test_device_equals_twin(gpu, shim, Q, d, Cn, N):
    rows = tw.normal_rows(Q, d, Cn, N, seed=1000 + d, stride=d + 1, fill=np.nan)          # the log-target column: NaN, never read
    ws, red = device_run(rows, d, range(1, N, 3), gpu)                                    # row 0, then segments of 3 rows
    want_ws = tw.twin_accumulate(shim, rows, d, N)
    assert np.all(np.isfinite(want_ws)) and np.all(want_ws[:, :, -1] == 0) and np.all(want_ws[:, :, -2] == N // 2)
    assert ws.shape == want_ws.shape and np.array_equal(ws, want_ws)
    want_red = tw.twin_reduce(shim, want_ws, d, N)
    assert np.all(np.isfinite(want_red)) and np.array_equal(red, want_red)


def test_device_drops_what_the_twin_drops(gpu, shim):
    from pyhillfit_amd import correlations as cr
    d, Cn, N = 11, 70, 21
    rows = tw.normal_rows(1, d, Cn, N, seed=77, stride=d + 1, fill=np.nan)
    rows[3, 0, 9, 0] = np.nan                                                # chain 0, half 0: the reference half-chain moves on
    rows[N - 2, 0, 2, 65] = np.inf                                           # second chain block, half 1, first column block
    rows[N // 2] = np.nan                                                    # the middle row is never read
    ws, red = device_run(rows, d, [4, 10, 11], gpu)
    want_ws = tw.twin_accumulate(shim, rows, d, N)
    assert np.array_equal(ws[:, :, -2:], want_ws[:, :, -2:]) and want_ws[0, :, -1].sum() == 2
    used = want_ws[0, :, -1] == 0                                            # [2][C]
    assert all(np.array_equal(ws[0, k, :, c], want_ws[0, k, :, c]) for k in range(2) for c in range(Cn) if used[k, c])
    want_red = tw.twin_reduce(shim, want_ws, d, N)
    assert np.array_equal(red, want_red)
    res = cr.finalize_reduced(red[0], d)
    assert res["half_chains_dropped"] == 2 and res["half_chains"] == 2 * Cn - 2 and np.isfinite(res["rhat_multivariate"])


# ---- 2. segmentation ------------------------------------------------------------------------------------------------------------------
def test_segmentation(gpu):
    d, N = 17, 41
    rows = tw.normal_rows(1, d, 64, N, seed=2)
    ws, red = device_run(rows, d, [], gpu)
    for cuts in (range(1, N), range(7, N, 7)):
        ws2, red2 = device_run(rows, d, cuts, gpu)
        assert np.array_equal(ws, ws2) and np.array_equal(red, red2)


# ---- 3. against the diagnostics -------------------------------------------------------------------------------------------------------
def test_diagonals_against_the_diagnostics(gpu):
    from pyhillfit_amd import correlations as cr
    from pyhillfit_amd.diagnostics import ChainDiagnostics
    Q, d, Cn, N = 2, 3, 64, 512
    rows = tw.normal_rows(Q, d, Cn, N, seed=3)
    x = torch.from_numpy(rows).to(gpu)
    dg = ChainDiagnostics(Q, Cn, d, N, 64, gpu)
    dg.accumulate(x)
    rhat, acov0 = dg.result()["rhat"], dg.reduced()[..., 0]
    acc = cr.PosteriorCorrelations(Q, Cn, d, N, gpu)
    acc.accumulate(x)
    h = N // 2
    for q, res in enumerate(acc.result()):
        got, want = res["rhat_from_moments"], rhat[q]
        w, w_want = np.diag(res["W"]), acov0[q] * h / (h - 1.0)
        print("problem %d: R-hat %s (diagnostics %s), worst relative difference %.3g; W diagonal %.3g" % (
            q, got, want, np.max(np.abs(got - want) / want), np.max(np.abs(w - w_want) / w_want)))
        assert np.max(np.abs(got - want) / want) <= 1e-10
        assert np.max(np.abs(w - w_want) / w_want) <= 1e-10
        assert res["rhat_multivariate"] >= np.max(got) - 1e-12


# ---- 4. the samplers through the analysis set -----------------------------------------------------------------------------------------
KEYS = {"columns", "rows_per_half_chain", "half_chains", "half_chains_dropped", "mean", "sd", "correlation", "within_correlation",
        "rhat_from_moments", "rhat_multivariate", "lambda_max", "apart_direction", "principal_axes", "strongest_pair", "method"}


def check_record(rec, columns, h, m):
    d = len(columns)
    assert set(rec) == KEYS and rec["columns"] == columns
    assert (rec["rows_per_half_chain"], rec["half_chains"], rec["half_chains_dropped"]) == (h, m, 0)
    json.dumps(rec, allow_nan=False)
    for key in ("correlation", "within_correlation"):
        M = np.array(rec[key], dtype=np.float64)
        assert M.shape == (d, d) and np.array_equal(M, M.T) and np.all(np.diag(M) == 1.0) and np.all(np.abs(M) <= 1.0)
    assert len(rec["mean"]) == len(rec["sd"]) == len(rec["rhat_from_moments"]) == d
    assert rec["rhat_multivariate"] >= max(rec["rhat_from_moments"]) - 1e-12
    assert rec["rhat_multivariate"] == np.sqrt((h - 1.0) / h + rec["lambda_max"])
    a = np.array([rec["apart_direction"][c] for c in columns])
    assert abs(np.linalg.norm(a) - 1.0) <= 1e-12 and a[np.argmax(np.abs(a))] > 0
    ev = rec["principal_axes"]["eigenvalues"]
    assert len(ev) == d and all(x >= y for x, y in zip(ev, ev[1:])) and ev[-1] > 0 and abs(sum(ev) - d) <= 1e-9
    assert list(rec["principal_axes"]["longest_axis"]) == columns
    i, j = (columns.index(c) for c in rec["strongest_pair"]["columns"])
    W = np.abs(np.array(rec["within_correlation"])) - np.eye(d)
    assert i < j and W[i, j] == W.max() and rec["strongest_pair"]["within_correlation"] == rec["within_correlation"][i][j]


def drive(s, iterations, segments, columns, kind, gpu):
    """the sampler through an AnalysisSet of the new adapter alone -> (its records per problem, the saved rows after the burn-in)"""
    from pyhillfit_amd import analyses as an
    saved = iterations // s.thinning + 1
    burn = saved // 4
    aset = an.AnalysisSet([an.Correlations], an.Run(args=None, kind=kind, Q=s.Q, C=s.C, cols=s.d + 1, columns=columns, saved=saved,
                                                    burn=burn, device=gpu, de=None))
    aset.feed_start(s.row0)
    host, r = [s.row0.cpu().numpy()[None]], 1
    for k in segments:
        rows = s.advance(k)
        aset.feed(rows, r, rows.shape[0])
        host.append(rows.cpu().numpy())
        r += rows.shape[0]
    assert r == saved
    aset.finish()
    recs = []
    for q in range(s.Q):
        summ = {}
        aset.record(summ, q)
        assert list(summ) == ["correlations"]
        recs.append(summ["correlations"])
    return recs, np.concatenate(host)[burn:]


def test_single_level_sampler(gpu, dr_setup):
    from pyhillfit_amd import bestfit
    from pyhillfit_amd import correlations as cr
    from pyhillfit_amd.PyHillFit import experiments_and_labels
    from pyhillfit_amd.sampler import SingleLevelSampler
    dr = dr_setup
    dr.define_model(2)
    el = [experiments_and_labels(d, c) for d, c in (("Amiodarone", "hERG"), ("Quinidine", "Nav1.5-late"))]
    data = [dr.concatenate_experiments(len(e), e) for e, _ in el]
    th0 = [bestfit.chain_start(t, 2) for t in bestfit.best_fit_batch(data, 2)[0]]
    s = SingleLevelSampler(dr.PackedPoints(data), 2, [0, 1], [1.0, 1.0], 64, thinning=5, seed=25, adapt_start=600, device=gpu)
    s.init(np.array(th0), cov_identity=False, cov_scale=0.05)
    columns = ["pIC50", "Hill", "sigma", "log-target"]
    recs, chain = drive(s, 2000, (700, 700, 600), columns, 2, gpu)
    assert chain.shape == (301, 2, 4, 64)
    for q, rec in enumerate(recs):
        check_record(rec, columns[:-1], 150, 128)
        assert rec == cr.json_record(cr.correlations_of_draws(chain[:, q, :3], columns[:-1], gpu))
        pooled = np.corrcoef(np.transpose(chain[:, q, :3], (0, 2, 1)).reshape(-1, 3)[np.r_[0:150 * 64, 151 * 64:301 * 64]], rowvar=False)
        assert np.max(np.abs(np.array(rec["correlation"]) - pooled)) <= 1e-9


def test_hierarchical_sampler(gpu, dr_setup):
    from pyhillfit_amd import correlations as cr
    from pyhillfit_amd import hierarchical as H
    dr = dr_setup
    ne, _, ex = dr.load_crumb_data("Amiodarone", "hERG")
    assert ne == 3
    s = H.HierarchicalSampler(H.PackedHierPoints([ex]), [0], 64, thinning=5, seed=3, problem_ids=[1], device=gpu)
    s.init(np.array([1., 5., 6., .3, 6., .8, 6.1, .7, 6.0, .9, 0.5])[None], cov_scale=0.01)
    columns = H.hierarchical_columns(ne)
    recs, chain = drive(s, 2000, (700, 700, 600), columns, "hierarchical", gpu)
    assert chain.shape == (301, 1, 12, 64) and len(columns) == 12
    check_record(recs[0], columns[:-1], 150, 128)
    assert recs[0] == cr.json_record(cr.correlations_of_draws(chain[:, 0, :11], columns[:-1], gpu))
    line = cr.report_line(0, ["Amiodarone + hERG"], [cr.correlations_of_draws(chain[:, 0, :11], columns[:-1], gpu)])
    assert line.startswith("correlations [rank 0]: ") and "strongest pIC50-Hill within correlation: Amiodarone + hERG (pic50_" in line


# ---- 5. the command line end to end ---------------------------------------------------------------------------------------------------
def _summaries(root):
    return {p: json.load(open(p)) for p in sorted(glob.glob(os.path.join(root, "**", "*_summary.json"), recursive=True))}


def _chain_files(root):
    return {os.path.relpath(p, root): open(p, "rb").read() for p in sorted(glob.glob(os.path.join(root, "**", "*.txt"), recursive=True))}


def _main(argv):
    from pyhillfit_amd import PyHillFit
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        PyHillFit.main(argv)
    return out.getvalue().splitlines()


@pytest.fixture(scope="module")
def csv_file(tmp_path_factory, gpu):
    from pyhillfit_amd import doseresponse as dr
    dr.setup(os.path.join(REPO, "data", "crumb_dataset.json"))
    p = tmp_path_factory.mktemp("data") / "crumb_data.csv"
    dr.table.to_csv(str(p))
    return str(p)


def _on_off(base, root):
    on, off = os.path.join(root, "on"), os.path.join(root, "off")
    lines_on = _main(base + ["--output-root", on, "--correlations"])
    lines_off = _main(base + ["--output-root", off])
    assert not [l for l in lines_off if l.startswith("correlations [rank")]
    assert _chain_files(on) == _chain_files(off) and len(_chain_files(on)) >= 1
    s_on, s_off = _summaries(on), _summaries(off)
    assert len(s_on) == len(s_off) >= 1
    for a, b in zip(s_on.values(), s_off.values()):
        assert "correlations" in a and "correlations" not in b
        a, b = dict(a), dict(b)
        a.pop("correlations"); a.pop("mh_samples_per_second"); b.pop("mh_samples_per_second")
        assert a == b
    return on, s_on, [l for l in lines_on if l.startswith("correlations [rank")]


@pytest.fixture(scope="module")
def single_level_cli(csv_file, tmp_path_factory):
    base = ["--data-file", csv_file, "-m", "2", "-i", "20000", "--drugs", "Amiodarone,Bepridil", "--channels", "hERG", "--num-chains", "64",
            "--segment", "7000", "--save-all-chains"]
    return _on_off(base, str(tmp_path_factory.mktemp("sl_cli")))


def test_single_level_command_line(single_level_cli):
    root, summaries, lines = single_level_cli
    assert len(summaries) == 2 and len(lines) == 1
    assert lines[0].startswith("correlations [rank 0]: ") and " of 2 with a multivariate R-hat > 1.01" in lines[0]
    assert "strongest pIC50-Hill within correlation: " in lines[0]
    for s in summaries.values():
        rows = s["saved_rows_after_burn_in"]
        check_record(s["correlations"], ["pIC50", "Hill", "sigma"], rows // 2, 128)


def test_hierarchical_command_line(csv_file, tmp_path):
    base = ["--data-file", csv_file, "-m", "2", "--hierarchical", "-i", "6000", "--drugs", "Amiodarone", "--channels", "hERG",
            "--num-chains", "64", "--segment", "2000"]
    root, summaries, lines = _on_off(base, str(tmp_path))
    assert len(summaries) == 1 and len(lines) == 1 and " of 1 with a multivariate R-hat > 1.01" in lines[0]
    from pyhillfit_amd.hierarchical import hierarchical_columns
    s = next(iter(summaries.values()))
    saved = 6000 // 5 + 1
    check_record(s["correlations"], hierarchical_columns(3)[:-1], (saved - saved // 4) // 2, 128)
    assert "note" not in s["correlations"]
    # with the differential-evolution moves the chains are coupled: the record says so, as the diagnostics' does
    de_root = os.path.join(root, "de")
    _main(base + ["--output-root", de_root, "--correlations", "--diagnostics", "--de-every", "10"])
    s = next(iter(_summaries(de_root).values()))
    assert s["correlations"]["note"] == s["diagnostics"]["note"] and s["correlations"]["chains_coupled_within_populations_of"] == 64


# ---- 6. the chain tool ----------------------------------------------------------------------------------------------------------------
def test_chain_tool(single_level_cli, gpu, capsys):
    from pyhillfit_amd import chain_correlations as cc
    from pyhillfit_amd import chainio
    from pyhillfit_amd import correlations as cr
    root, summaries, _ = single_level_cli
    names = ["pIC50", "Hill", "sigma"]
    for path, s in summaries.items():
        npy = path.replace("_summary.json", "_all_chains.npy")
        x = np.load(npy)
        capsys.readouterr()
        cc.main([npy, "--device", gpu])
        got = json.loads(capsys.readouterr().out)
        want = cr.json_record(cr.correlations_of_draws(x[:, :3], names, gpu))
        assert {k: got[k] for k in want} == want and got["chains"] == 64 and got["rows"] == x.shape[0] and got["kinds"] == ["all chains"]
        assert want == s["correlations"]                                     # the file holds the rows the run fed, bit for bit
    # reference-format text files: one chain each, several files side by side
    texts = sorted(glob.glob(os.path.join(root, "**", "*_chain_single-level.txt"), recursive=True))
    assert len(texts) == 2
    loaded = [chainio.load_chain(p) for p in texts]
    n = min(len(a) for a in loaded)
    draws = np.stack([a[:n, :3] for a in loaded], axis=2)
    capsys.readouterr()
    cc.main(texts + ["--device", gpu])
    got = json.loads(capsys.readouterr().out)
    want = cr.json_record(cr.correlations_of_draws(draws, names, gpu))
    assert {k: got[k] for k in want} == want and got["chains"] == 2 and got["half_chains"] == 4 and got["kinds"] == ["text", "text"]
