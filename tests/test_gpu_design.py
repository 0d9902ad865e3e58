"""Expected information gain of a next dose on the GPU: phf_design_accumulate against the host build of phf_design.h (the twin,
tests/test_design_host.py) bit for bit — one draw at the edges of the parameter space, sums over chains and rows, row cuts and
thinning, the chain-parity halves — and the command line's --next-dose against chain_design on the run's own files."""
import glob
import json
import os

import numpy as np
import pytest

from conftest import REPO
from test_design_host import build_shim, make_rows, twin_accumulate, twin_pred

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shim(tmp_path_factory.mktemp("design_gpu"))


def stack_rows(model, draws):
    """draws [Q][n][C][model + 1] -> rows [n][Q][model + 2][C]"""
    return np.ascontiguousarray(np.concatenate([make_rows(model, d) for d in draws], axis=1))


def run_gpu(model, rows, doses, K, gpu, every=1, cuts=None, first_row=0, slots=None):
    """the rows through NextDose, cut into calls of the sizes `cuts` -> (accumulators, the object)"""
    from pyhillfit_amd import design as ds
    nd = ds.NextDose(model, rows.shape[1], rows.shape[3], doses, None, K, every, gpu, slots)
    nd.rows_seen = first_row
    t = torch.from_numpy(rows).to(gpu)
    r = 0
    for n in cuts or [rows.shape[0]]:
        nd.accumulate(t[r:r + n].contiguous())
        r += n
    assert r == rows.shape[0]
    return nd.accumulators(), nd


def random_draws(rng, Q, n, Cn):
    return np.stack([rng.uniform(4.5, 7.0, (Q, n, Cn)), rng.uniform(0.3, 4.0, (Q, n, Cn)), rng.uniform(0.3, 25.0, (Q, n, Cn))], axis=3)


# ---- 1. one draw equals the twin ---------------------------------------------------------------------------------------------------
EDGE_DOSES = [[1e-300, 0.3, 30.0], [1e-3, 1.0, 1e4]]
EDGE_DRAWS = [([5.5, 10.0, 3.0], [5.5, 0.0, 3.0]),                        # Hill = 10; Hill = 0
              ([30.0, 1.0, 2.0], [6.0, 10.0, 1.0000001e-3]),              # a prediction of exactly 100; sigma just above its floor
              ([5.0, 1.0, 50.0], [9.0, 0.5, 1.0000001e-3])]               # sigma = 50


@pytest.mark.parametrize("model", [1, 2])
@pytest.mark.parametrize("K", [128, 1024])
def test_one_draw_equals_the_twin(shim, gpu, K, model):
    assert twin_pred(shim, model, 0.3, 30.0, 1.0) == 100.0                 # the cases are what they claim to be
    assert twin_pred(shim, model, 1e-300, 5.5, 10.0) == 0.0
    for pair in EDGE_DRAWS:
        d = np.array(pair, dtype=np.float64)[:, None, None, :]            # [Q = 2][rows = 1][C = 1][3]
        if model == 1:
            d = d[..., [0, 2]]
        rows = stack_rows(model, d)
        assert rows.shape == (1, 2, model + 2, 1)
        got, nd = run_gpu(model, rows, EDGE_DOSES, K, gpu)
        want = twin_accumulate(shim, model, K, rows, EDGE_DOSES, nd.slots)
        assert got.shape == want.shape == (2, 3, 2, K + 132)
        assert np.array_equal(got, want), (pair, np.argwhere(got != want)[:5])
        assert np.all(got[:, :, 0, K + 130] == 1) and np.all(got[:, :, 1] == 0)
        assert np.all(np.abs(got[:, :, 0, :K + 2].sum(axis=2) - 1.0) <= 1e-14)


# ---- 2. sums --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("Cn", [3, 64, 65])
def test_sums_equal_the_twin(shim, gpu, Cn, G):
    """the order of every sum is fixed and restated in the twin: equality, not a tolerance"""
    rng = np.random.default_rng(100 * Cn + G)
    rows = stack_rows(2, random_draws(rng, 2, 5, Cn))
    doses = [[0.01, 1.0, 100.0][:G], [3.0, 0.05, 20.0][:G]]
    got, nd = run_gpu(2, rows, doses, 256, gpu)
    assert nd.slots == {3: 2, 64: 64, 65: 64}[Cn]
    want = twin_accumulate(shim, 2, 256, rows, doses, nd.slots)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert np.all(got[..., 256 + 130].sum(axis=2) == 5 * Cn)
    again, _ = run_gpu(2, rows, doses, 256, gpu)
    assert np.array_equal(got, again)
    # the slots are a device detail: another number of them moves every result by rounding only (sums of n <= 325 terms >= 0)
    from pyhillfit_amd import design as ds
    two, _ = run_gpu(2, rows, doses, 256, gpu, slots=2)
    for q in range(2):
        a, b = ds.finalize(got[q], doses[q], [], 256, 1, Cn), ds.finalize(two[q], doses[q], [], 256, 1, Cn)
        assert np.allclose(a["eig"], b["eig"], rtol=0, atol=1e-12) and np.all(a["eig"] > 0)


# ---- 3. row cuts and thinning --------------------------------------------------------------------------------------------------------
def test_row_cuts_and_thinning(shim, gpu):
    rng = np.random.default_rng(7)
    d = random_draws(rng, 2, 5, 5)
    d[1, 1, 3, 2] = 1e-3                                                   # a skipped draw in global row 2, which is used
    d[0, 0, 0, 0] = np.nan                                                 # and one in global row 1, which is not
    rows = stack_rows(2, d)
    doses = [[0.1, 10.0], [1.0, 100.0]]
    whole, nd = run_gpu(2, rows, doses, 256, gpu, every=2, first_row=1)
    cut, _ = run_gpu(2, rows, doses, 256, gpu, every=2, first_row=1, cuts=[2, 3])
    ones, _ = run_gpu(2, rows, doses, 256, gpu, every=2, first_row=1, cuts=[1, 1, 1, 1, 1])
    assert np.array_equal(whole, cut) and np.array_equal(whole, ones)
    assert np.array_equal(whole, twin_accumulate(shim, 2, 256, rows, doses, nd.slots, 1, 2))
    # the global rows 2 and 4 of the rows 1..5
    assert np.array_equal(whole, twin_accumulate(shim, 2, 256, rows[[1, 3]], doses, nd.slots, 0, 1))
    res = nd.result()
    assert [r["draws_used"] for r in res] == [2 * 5, 2 * 5 - 1] and [r["draws_skipped"] for r in res] == [0, 1]
    # a call whose rows hold no used row changes nothing
    from pyhillfit_amd import design as ds
    idle = ds.NextDose(2, 2, 5, doses, None, 256, 2, gpu)
    idle.rows_seen = 1
    idle.accumulate(torch.from_numpy(rows[:1]).to(gpu))
    assert idle.rows_seen == 2 and not idle.accumulators().any()
    idle.accumulate(torch.from_numpy(rows[1:]).to(gpu))
    assert np.array_equal(idle.accumulators(), whole)


# ---- 4. chain parity -----------------------------------------------------------------------------------------------------------------
def test_chain_parity(shim, gpu):
    from pyhillfit_amd import design as ds
    rng = np.random.default_rng(9)
    d = random_draws(rng, 1, 6, 3)
    doses = [[0.1, 1.0, 10.0]]
    acc, nd = run_gpu(2, stack_rows(2, d), doses, 256, gpu)
    assert nd.slots == 2 and np.all(acc[0, :, 0, 256 + 130] == 12) and np.all(acc[0, :, 1, 256 + 130] == 6)
    res = nd.result()[0]
    even, odd = d.copy(), d.copy()
    odd[:, :, [0, 2], 0] = np.nan                                          # chains 0 and 2 skipped: chain 1 alone
    even[:, :, 1, 0] = np.nan
    for half, part in ((0, even), (1, odd)):
        r = run_gpu(2, stack_rows(2, part), doses, 256, gpu)[1].result()[0]
        assert np.array_equal(r["eig"], res["eig_parity"][:, half])
        assert r["draws_used"] == (12, 6)[half]
    rec = ds.json_record(res)
    assert all(len(c["eig_by_chain_parity"]) == 2 for c in rec["candidates"])
    # one chain: the odd half is empty, and the record says null
    acc1, nd1 = run_gpu(2, stack_rows(2, d[:, :, :1]), doses, 256, gpu)
    assert not acc1[:, :, 1].any() and np.all(acc1[0, :, 0, 256 + 130] == 6)
    rec1 = ds.json_record(nd1.result()[0])
    assert all(c["eig_by_chain_parity"] is None for c in rec1["candidates"]) and all(np.isfinite(c["eig"]) for c in rec1["candidates"])


# ---- 5. the command line --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def csv_file(gpu, tmp_path_factory):
    from pyhillfit_amd import doseresponse as dr
    dr.setup(os.path.join(REPO, "data", "crumb_dataset.json"))
    p = tmp_path_factory.mktemp("data") / "crumb_data.csv"
    dr.table.to_csv(str(p))
    return str(p)


def _summaries(root):
    out = {}
    for path in sorted(glob.glob(os.path.join(root, "**", "*_summary.json"), recursive=True)):
        with open(path) as f:
            out[path] = json.load(f)
    return out


def _strip(s):
    s.pop("mh_samples_per_second")                                         # a wall-clock rate
    return s


def test_command_line(csv_file, tmp_path):
    from pyhillfit_amd import PyHillFit
    from pyhillfit_amd.chain_design import design_file
    base = ["--data-file", csv_file, "-m", "2", "-i", "4000", "--drugs", "Amiodarone,Bepridil", "--channels", "hERG", "--num-chains", "64",
            "--segment", "1500", "--save-all-chains"]
    PyHillFit.main(base + ["--output-root", str(tmp_path / "on"), "--next-dose", "4", "--next-dose-concs", "1.0", "--next-dose-every", "1"])
    PyHillFit.main(base + ["--output-root", str(tmp_path / "off")])
    on, off = _summaries(str(tmp_path / "on")), _summaries(str(tmp_path / "off"))
    assert len(on) == 2 and len(off) == 2
    for (path, s_on), (path_off, s_off) in zip(on.items(), off.items()):
        for ext in (".txt", "_all_chains.npy"):
            with open(path.replace("_summary.json", ext), "rb") as f, open(path_off.replace("_summary.json", ext), "rb") as g:
                assert f.read() == g.read(), ext
        assert "next_dose" not in s_off
        rec = s_on.pop("next_dose")
        assert _strip(s_on) == _strip(s_off)
        assert rec["bins"] == 256 and rec["every"] == 1 and rec["draws_skipped"] == 0
        assert rec["draws_used"] == 64 * s_off["saved_rows_after_burn_in"]
        assert len(rec["candidates"]) == 5 and rec["candidates"][4]["dose"] == 1.0
        for c in rec["candidates"]:
            assert np.isfinite(c["eig"]) and c["eig"] >= c["eig_coarse"] - 1e-12 and c["eig_coarse"] >= -1e-12
            assert len(c["eig_by_chain_parity"]) == 2
        assert rec["best"] in rec["candidates"]
        tool = design_file(path.replace("_summary.json", "_all_chains.npy"), doses=4, concs=(1.0,), every=1)
        assert tool["chains"] == 64 and tool["draws_used"] == rec["draws_used"]
        for a, b in zip(tool["candidates"], rec["candidates"]):
            assert a["dose"] == b["dose"] and a["already_tested"] == b["already_tested"]
            assert abs(a["eig"] - b["eig"]) <= 1e-12 and abs(a["eig_coarse"] - b["eig_coarse"]) <= 1e-12
