"""Batch means on the GPU: the device workspace against the host build of phf_batch_means.h bit for bit, the reduced ladder against the
numpy restatement of test_batch_means_host.py, bit-identity however the rows are cut, the stream contract and the command lines."""
import glob
import json
import os

import numpy as np
import pytest

from conftest import REPO
from test_batch_means_host import build_shim, host_state, levels_of, make_rows, numpy_reduced

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

Q, COLS, STRIDE = 2, 3, 5


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return "cuda:0"


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shim(tmp_path_factory.mktemp("batch_means_gpu"))


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def rows_of(N, chains, seed):
    """[N][Q][STRIDE][chains]; the columns beyond COLS are NaN and must not be read into anything"""
    x = np.stack([make_rows(N, COLS, STRIDE, chains, seed + q) for q in range(Q)], axis=1)
    x[:, :, COLS:] = np.nan
    return x


def run_device(x, cuts, device):
    """(workspace [Q][COLS][5 NL + 2][C], reduced [Q][COLS][NL + 1]) after feeding x in calls that end at `cuts`"""
    from pyhillfit_amd.batch_means import BatchMeans
    N = x.shape[0]
    t = torch.from_numpy(np.ascontiguousarray(x)).to(device)
    d = BatchMeans(Q, x.shape[3], COLS, N, device)
    first = 0
    for end in sorted(set(int(c) for c in cuts if 0 < c < N)) + [N]:
        d.accumulate(t[first:end])
        first = end
    ws, red = d.workspace(), d.reduced()
    d.free()
    return ws, red


@pytest.mark.parametrize("N", [70, 1027, 2048])
@pytest.mark.parametrize("chains", [40, 64, 128])
def test_accumulate_and_reduce(gpu, shim, chains, N):
    x = rows_of(N, chains, seed=7 * N + chains)
    ws, red = run_device(x, [], gpu)
    nl = levels_of(N // 2)
    assert ws.shape == (Q, COLS, 5 * nl + 2, chains) and red.shape == (Q, COLS, nl + 1)
    for q in range(Q):
        assert _same_bits(ws[q], host_state(shim, x[:, q], COLS)), q         # every x0, pending sum, S1 and S2
        for j in range(COLS):
            want = numpy_reduced(x[:, q, j])
            ladder = np.r_[0:nl - 1, nl]                                      # the levels' variances and B/h: 1e-12 relative
            assert np.all(want[ladder] > 0)
            assert np.max(np.abs(red[q, j, ladder] / want[ladder] - 1.0)) <= 1e-12, (q, j)
            assert abs(red[q, j, nl - 1] - want[nl - 1]) <= 1e-12 * max(abs(want[nl - 1]), np.sqrt(want[0])), (q, j)   # the mean: of its scale


def test_cut_anywhere_same_bits(gpu):
    N, chains = 1027, 70
    h = N // 2
    x = rows_of(N, chains, seed=5)
    ws, red = run_device(x, [], gpu)
    for cuts in (range(1, N), range(31, N, 31), range(32, N, 32), range(33, N, 33), [h - 1], [h], [h + 1], [N - h - 1, N - h, N - h + 1]):
        ws2, red2 = run_device(x, cuts, gpu)
        assert _same_bits(ws2, ws) and _same_bits(red2, red), list(cuts)[:3]


def test_result_on_another_stream(gpu):
    from pyhillfit_amd.batch_means import BatchMeans, diagnose
    x = rows_of(300, 64, seed=9)
    t = torch.from_numpy(np.ascontiguousarray(x)).to(gpu)
    torch.cuda.synchronize()

    def run():
        d = BatchMeans(Q, 64, COLS, 300, gpu)
        d.accumulate(t[:111])
        d.accumulate(t[111:])
        return d.result()

    want = run()
    with torch.cuda.stream(torch.cuda.Stream(device=gpu)):
        got = run()
    torch.cuda.synchronize()
    assert want.keys() == got.keys()
    for k in want:
        assert np.array_equal(want[k], got[k], equal_nan=want[k].dtype.kind == "f"), k
    one = diagnose(x[:, 1, :COLS], gpu)                                     # arrays in memory: [rows][cols][chains] of one problem
    for k in want:
        assert np.array_equal(want[k][1], one[k], equal_nan=want[k].dtype.kind == "f"), k
    assert np.all(np.isfinite(want["ess"][:, 2]))                           # white noise: a plateau at once


# ---- the command lines ---------------------------------------------------------------------------------------------------------------
FIELDS = ("ess", "mcse_mean", "tau", "tau_rel_se", "tau_lugsail", "level", "batch_rows", "plateau_reached", "chains_agree", "ess_upper_bound")


@pytest.fixture(scope="module")
def csv_file(tmp_path_factory, gpu):
    from pyhillfit_amd import doseresponse as dr
    dr.setup(os.path.join(REPO, "data", "crumb_dataset.json"))
    p = tmp_path_factory.mktemp("data") / "crumb_data.csv"
    dr.table.to_csv(str(p))
    return str(p)


def _files(root, pattern):
    return sorted(glob.glob(os.path.join(root, "**", pattern), recursive=True))


def _check_record(bm_rec, columns, draws):
    assert sorted(bm_rec) == sorted(FIELDS + ("method",))
    columns = len(bm_rec["ess"]) if columns is None else columns
    for k in FIELDS:
        assert len(bm_rec[k]) == columns, k
    for j in range(columns):
        if bm_rec["ess"][j] is not None:
            assert bm_rec["plateau_reached"][j] and bm_rec["chains_agree"][j] and bm_rec["ess_upper_bound"][j] is None
            assert abs(bm_rec["ess"][j] * bm_rec["tau"][j] / draws - 1.0) < 1e-12 and bm_rec["mcse_mean"][j] > 0
            assert bm_rec["batch_rows"][j] >= 2 and bm_rec["level"][j] >= 1
        else:
            assert bm_rec["ess_upper_bound"][j] is not None and bm_rec["mcse_mean"][j] is None and bm_rec["tau"][j] is None


def _compare_runs(on_root, off_root, columns, draws):
    """summaries of the run with the flag against the run without: (batch_means objects); everything else identical"""
    out = []
    on, off = _files(on_root, "*_summary.json"), _files(off_root, "*_summary.json")
    assert len(on) == len(off) >= 1
    for p_on, p_off in zip(on, off):
        s_on, s_off = json.load(open(p_on)), json.load(open(p_off))
        bm_rec = s_on["diagnostics"].pop("batch_means")
        assert columns is None or len(s_on["diagnostics"]["rhat"]) == columns
        assert len(bm_rec["ess"]) == len(s_on["diagnostics"]["rhat"])
        assert "batch_means" not in s_off["diagnostics"]
        assert s_on["diagnostics"] == s_off["diagnostics"]                   # every existing key untouched
        _check_record(bm_rec, columns, draws)
        out.append((p_on, bm_rec))
    chains_on, chains_off = _files(on_root, "*chain*.txt"), _files(off_root, "*chain*.txt")
    assert len(chains_on) == len(chains_off) >= 1
    for a, b in zip(chains_on, chains_off):
        assert open(a, "rb").read() == open(b, "rb").read(), a               # the chain files: byte-identical
    return out


def test_hierarchical_cli(csv_file, tmp_path, capsys):
    from pyhillfit_amd import PyHillFit
    base = ["--data-file", csv_file, "-m", "2", "--hierarchical", "-i", "20000", "--drugs", "Amiodarone", "--channels", "hERG",
            "--num-chains", "64", "--diagnostics"]
    PyHillFit.main(base + ["--output-root", str(tmp_path / "on"), "--diagnostic-batch-means"])
    assert "batch means [rank 0]: " in capsys.readouterr().out
    PyHillFit.main(base + ["--output-root", str(tmp_path / "off")])
    assert "batch means" not in capsys.readouterr().out
    (_, rec), = _compare_runs(str(tmp_path / "on"), str(tmp_path / "off"), 12, 64 * 2 * (3001 // 2))


def test_hierarchical_cli_fused_on_off(csv_file, tmp_path):
    """several launch groups through the one fused grid: the same batch means as a launch per group, and the chain files of a run
    without the flag"""
    from pyhillfit_amd import PyHillFit
    base = ["--data-file", csv_file, "-m", "2", "--hierarchical", "-i", "6000", "--drugs", "Amiodarone,Bepridil,Quinidine",
            "--channels", "hERG,Cav1.2", "--segment", "2000", "--diagnostics"]
    PyHillFit.main(base + ["--diagnostic-batch-means", "--fused-launch", "on", "--output-root", str(tmp_path / "on")])
    PyHillFit.main(base + ["--diagnostic-batch-means", "--fused-launch", "off", "--output-root", str(tmp_path / "off")])
    PyHillFit.main(base + ["--fused-launch", "on", "--output-root", str(tmp_path / "plain")])
    recs = _compare_runs(str(tmp_path / "on"), str(tmp_path / "plain"), None, 128 * 2 * (901 // 2))
    assert len(recs) > 1
    for (p_on, rec), p_off in zip(recs, _files(str(tmp_path / "off"), "*_summary.json")):
        assert json.load(open(p_off))["diagnostics"]["batch_means"] == rec, p_on


def test_single_level_cli_equals_chain_file_tool(csv_file, tmp_path):
    from pyhillfit_amd import PyHillFit
    from pyhillfit_amd.chain_diagnostics import diagnose_file
    base = ["--data-file", csv_file, "-m", "2", "-i", "20000", "--drugs", "Amiodarone", "--channels", "hERG", "--num-chains", "64",
            "--segment", "7000", "--save-all-chains", "--diagnostics"]
    PyHillFit.main(base + ["--output-root", str(tmp_path / "on"), "--diagnostic-batch-means"])
    PyHillFit.main(base + ["--output-root", str(tmp_path / "off")])
    (p_on, rec), = _compare_runs(str(tmp_path / "on"), str(tmp_path / "off"), 4, 64 * 2 * (3001 // 2))
    got = diagnose_file(p_on.replace("_summary.json", "_all_chains.npy"), batch_means=True)       # the same rows, from the disk
    assert got["batch_means"] == rec
    assert "batch_means" not in diagnose_file(p_on.replace("_summary.json", "_all_chains.npy"))


def test_pyhilltemp_cli(csv_file, tmp_path):
    from pyhillfit_amd import PyHillTemp
    base = ["--data-file", csv_file, "-m", "1", "-d", "0", "-c", "0", "-i", "3000", "-t", "5", "--rungs", "1", "--num-chains", "64",
            "--diagnostics"]
    res = PyHillTemp.main(base + ["--output-root", str(tmp_path / "on"), "--diagnostic-batch-means"])
    off = PyHillTemp.main(base + ["--output-root", str(tmp_path / "off")])
    assert len(res) == len(off) == 2
    (ti_on,) = _files(str(tmp_path / "on"), "thermodynamic_integration.json")
    (ti_off,) = _files(str(tmp_path / "off"), "thermodynamic_integration.json")
    ti, ti0 = json.load(open(ti_on)), json.load(open(ti_off))
    for r_on, r_off, d_on in zip(res, off, ti["diagnostics"]):
        assert d_on["batch_means"] == r_on["diagnostics"]["batch_means"]
        _check_record(d_on.pop("batch_means"), 3, 64 * 2 * (451 // 2))
        r_on["diagnostics"].pop("batch_means", None)
        assert r_on["diagnostics"] == r_off["diagnostics"] and "batch_means" not in r_off["diagnostics"]
    assert ti == ti0
    for a, b in zip(_files(str(tmp_path / "on"), "*.txt"), _files(str(tmp_path / "off"), "*.txt")):
        assert open(a, "rb").read() == open(b, "rb").read(), a
