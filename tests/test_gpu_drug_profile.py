"""The drug profile on the GPU (phf_drug_profile_*): device histograms and tallies equal the host build of phf_drug_profile.h count for
count, the workspace is bit-identical however the rows are cut, a slot split over two workgroups, non-finite draws, the reference's
Verapamil samples through the tool, and PyHillFit's --drug-profile-concs against the draws of --save-all-chains."""
import glob
import json
import os

import numpy as np
import pytest

from drug_profile_twin import (CRUMB_CHANNELS, GOLDEN, VERAPAMIL_CMAX_UM, numpy_block, shim, twin_histograms, twin_profile,  # noqa: F401
                               verapamil)
from test_gpu_waic import _chain_files, _summaries, csv_file, gpu  # noqa: F401

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PROBS = (0.0, 0.025, 0.25, 0.5, 0.75, 0.975, 1.0)
# 2 drugs over 3 channel places: the first has all three (problems 0, 2, 3), the second the middle one alone (problem 1)
MAP = [[0, 2, 3], [-1, 1, -1]]
WEIGHTS = [1.0, -1.0, 0.5]
DOSES = [[0.3, 3.0], [1.0, 10.0]]


def synthetic(rng, rows, chains, Q=4, stride=3):
    """[rows][Q][stride][chains]: pIC50, Hill, and a column that is never read"""
    x = np.full((rows, Q, stride, chains), np.nan)
    x[:, :, 0] = rng.normal(5.5, 0.5, (rows, Q, chains))
    x[:, :, 1] = rng.uniform(0.5, 2.0, (rows, Q, chains))
    return x


def run(x, model, cuts, device, bins=64, cp=MAP, weights=WEIGHTS, doses=DOSES, probs=PROBS):
    from pyhillfit_amd.drug_profile import DrugProfile
    acc = DrugProfile(model, x.shape[1], x.shape[3], cp, weights, doses, x.shape[0], probs, bins, device)
    t = torch.from_numpy(x).to(device)
    for part in np.split(np.arange(x.shape[0]), cuts):
        if part.size:
            acc.accumulate(t[part[0]:part[-1] + 1].contiguous())
    return acc


def check_against_twin(acc, lib, x, model, cuts, bins, cp=MAP, weights=WEIGHTS, doses=DOSES, probs=PROBS):
    values, tally, live = twin_profile(lib, model, x, cp, weights, doses)
    hists = twin_histograms(values, bins, cuts)
    counts, nf, got_tally = acc.counts()
    res = acc.result()
    K = len(cp[0])
    assert np.array_equal(got_tally.astype(np.int64), tally)
    for d, j, k in np.ndindex(*live.shape):
        s = j * (K + 1) + k
        if not live[d, j, k]:
            assert not counts[d, j, k].any() and nf[d, j, k] == 0 and res["draws"][d, s] == 0
            continue
        h = hists[d, j, k]
        assert np.array_equal(counts[d, j, k], h.counts), (d, j, k)
        assert nf[d, j, k] == h.nonfinite == res["non_finite"][d, s] and res["level"][d, s] == h.k
        assert res["min"][d, s] == h.mn and res["max"][d, s] == h.mx and res["bin_width"][d, s] == h.width
        got = np.stack([res["value"][d, s], res["lo"][d, s], res["hi"][d, s], res["bin"][d, s]], axis=1)
        assert np.array_equal(got, h.quantiles(probs)), (d, j, k)
    return values, tally, res


@pytest.mark.parametrize("model", [1, 2])
@pytest.mark.parametrize("chains", [5, 65])
def test_device_counts_equal_twin(gpu, shim, model, chains):  # noqa: F811
    x = synthetic(np.random.default_rng(10 * chains + model), 7, chains)
    acc = run(x, model, [3], gpu)
    _, tally, res = check_against_twin(acc, shim, x, model, [3], 64)
    assert np.all(res["level"][0] > 0)                                       # 64 bins: the grid was coarsened and merged
    assert tally[0, :, :, 4].sum() == 2 * 7 * chains and tally[:, :, :, 5].sum() == 0


def test_segmentation_gives_identical_workspaces(gpu):  # noqa: F811
    x = synthetic(np.random.default_rng(7), 7, 65)
    x[2, 2, 0, 7] = np.nan
    ref = run(x, 2, [], gpu).ws.view(torch.int64).cpu()
    for cuts in ([3], [1]):
        assert torch.equal(run(x, 2, cuts, gpu).ws.view(torch.int64).cpu(), ref), cuts


def test_a_slot_split_over_two_workgroups(gpu, shim):  # noqa: F811
    """2049 rows x 64 chains = 131 136 values per slot, just past the 131 072 one bin workgroup takes"""
    x = synthetic(np.random.default_rng(2049), 2049, 64, Q=2, stride=2)
    cp, w, doses = [[0, 1]], [1.0, -1.0], [[1.0]]
    acc = run(x, 2, [], gpu, 64, cp, w, doses)
    _, tally, _ = check_against_twin(acc, shim, x, 2, [], 64, cp, w, doses)
    assert tally[0, 0, :, 3].sum() == 2049 * 64


def test_non_finite_draws(gpu, shim):  # noqa: F811
    x = synthetic(np.random.default_rng(3), 5, 6)
    x[1, 0, 0, 2] = np.nan                                       # pIC50 of drug 0's channel 0
    x[3, 3, 1, 5] = np.inf                                       # Hill of drug 0's channel 2
    acc = run(x, 2, [2], gpu)
    check_against_twin(acc, shim, x, 2, [2], 64)
    _, nf, tally = acc.counts()
    for j in range(2):
        assert nf[0, j].tolist() == [1, 0, 1, 2] and nf[1, j].tolist() == [0, 0, 0, 0]
        both = tally[0, j, 0] + tally[0, j, 1]
        assert both[4] == 28 and both[5] == 2 and both[:3].sum() == 28
    acc1 = run(x, 1, [2], gpu)                                   # model 1 does not read the Hill column
    assert acc1.counts()[1][0, 0].tolist() == [1, 0, 0, 1]


def test_fixture_through_the_tool(gpu, capsys):  # noqa: F811
    from pyhillfit_amd import drug_profile as dp
    argv = ["--cmax-nM", "45", "--drug", "Verapamil", "--bins", "4096", "--device", gpu]
    for ch in CRUMB_CHANNELS:
        argv += ["--channel", "%s=%s" % (ch, os.path.join(GOLDEN, "Verapamil_%s_hill_pic50_samples.txt" % ch))]
    capsys.readouterr()
    dp.main(argv)
    rec = json.loads(capsys.readouterr().out)
    assert rec["rows_used"] == 500 and rec["chains_used"] == 1 and rec["model"] == 2 and rec["cmax_uM"] == VERAPAMIL_CMAX_UM
    assert all(f["rows_dropped"] == 0 and f["chains_dropped"] == 0 for f in rec["files_by_channel"].values())
    hill, pic50 = verapamil()
    w = np.array([rec["weights"][ch] for ch in CRUMB_CHANNELS])
    assert list(w) == [1.0, -1.0, -1.0, -1.0, 1.0, 1.0, 1.0]
    for j, (m, positive) in enumerate(zip((1.0, 3.0, 10.0), (41, 10, 18))):
        d = rec["doses"][j]
        assert d["dose_uM"] == m * VERAPAMIL_CMAX_UM
        block = numpy_block(np.log(m * VERAPAMIL_CMAX_UM), hill, pic50)
        net = np.zeros(500)
        for k in range(7):
            net = net + w[k] * block[k]
        for got, v in [(d["block"][ch], block[k]) for k, ch in enumerate(CRUMB_CHANNELS)] + [(d["net"], net)]:
            want = np.quantile(v, rec["probs"], method="inverted_cdf")
            slack = 1e-12 * np.maximum(np.abs(want), 100.0)      # numpy's exp against the device's, as for the curve bands
            assert np.all(np.array(got["lo"]) - slack <= want) and np.all(want <= np.array(got["hi"]) + slack)
            assert got["draws"] == 500 and got["non_finite"] == 0
            assert got["bin_width"] <= 4.0 * (got["max"] - got["min"]) / 4096
            assert np.all(np.array(got["hi"]) - np.array(got["lo"]) <= got["bin_width"])
        assert d["net_positive_draws"] == positive and d["p_net_positive"] == positive / 500 and d["draws_used"] == 500
        dominant = np.bincount(np.argmax(block, axis=0), minlength=7)
        assert [d["dominant_draws"][ch] for ch in CRUMB_CHANNELS] == dominant.tolist()
        assert d["by_chain_parity"]["odd"]["draws_used"] == 0 and d["by_chain_parity"]["even"]["net_positive_draws"] == positive


def test_command_line(csv_file, tmp_path, capsys):  # noqa: F811
    from pyhillfit_amd import PyHillFit
    from pyhillfit_amd import quantiles as qn
    channels = ["hERG", "Cav1.2", "Nav1.5-peak"]
    base = ["--data-file", csv_file, "-m", "2", "-i", "20000", "--drugs", "Verapamil,Quinidine", "--channels", ",".join(channels),
            "--segment", "7000", "--save-all-chains"]
    capsys.readouterr()
    PyHillFit.main(base + ["--output-root", str(tmp_path / "on"), "--drug-profile-concs", "0.045,1.5"])
    out = capsys.readouterr().out
    PyHillFit.main(base + ["--output-root", str(tmp_path / "off")])
    assert "drug-profile [rank 0]: 2 drugs" in out and "drug-profile" not in capsys.readouterr().out
    on, off = _summaries(str(tmp_path / "on")), _summaries(str(tmp_path / "off"))
    assert len(on) == 6 and [os.path.relpath(p, tmp_path / "on") for p in on] == [os.path.relpath(p, tmp_path / "off") for p in off]
    for s_on, s_off in zip(on.values(), off.values()):
        s_on.pop("mh_samples_per_second"); s_off.pop("mh_samples_per_second")
        assert s_on == s_off
    assert _chain_files(str(tmp_path / "on")) == _chain_files(str(tmp_path / "off"))
    npys = sorted(glob.glob(str(tmp_path / "on" / "**" / "*_all_chains.npy"), recursive=True))
    for p in npys:
        assert open(p, "rb").read() == open(p.replace(str(tmp_path / "on"), str(tmp_path / "off")), "rb").read()
    assert not glob.glob(str(tmp_path / "off" / "**" / "drug_profiles"), recursive=True)
    files = sorted(glob.glob(str(tmp_path / "on" / "**" / "drug_profiles" / "*_drug_profile.json"), recursive=True))
    assert [os.path.basename(f) for f in files] == ["Quinidine_drug_profile.json", "Verapamil_drug_profile.json"]
    for f in files:
        rec = json.load(open(f))
        drug = rec["drug"]
        assert rec["channels"] == rec["channels_loaded"] == ["hERG", "Nav1.5-peak", "Cav1.2"]        # the data file's order
        assert rec["probs"] == list(qn.DEFAULT_PROBS) and rec["bins"] == 4096 and "convention" in rec["weights_note"]
        draws = {ch: np.load(next(p for p in npys if "/%s/%s/" % (drug, ch) in p)) for ch in rec["channels"]}
        w = [rec["weights"][ch] for ch in rec["channels"]]
        assert w == [1.0, -1.0, -1.0] and [d["dose_uM"] for d in rec["doses"]] == [0.045, 1.5]
        for d in rec["doses"]:
            block = [qn.hill_curve(2, np.log(d["dose_uM"]), draws[ch][:, 0, :], draws[ch][:, 1, :]) for ch in rec["channels"]]
            net = np.zeros_like(block[0])
            for k in range(3):
                net = net + w[k] * block[k]
            for got, v in [(d["block"][ch], block[k]) for k, ch in enumerate(rec["channels"])] + [(d["net"], net)]:
                want = np.quantile(v.ravel(), rec["probs"], method="inverted_cdf")
                slack = 1e-12 * np.maximum(np.abs(want), 100.0)
                assert np.all(np.array(got["lo"]) - slack <= want) and np.all(want <= np.array(got["hi"]) + slack)
                assert got["draws"] == v.size and got["non_finite"] == 0
            assert d["draws_used"] == net.size and d["draws_skipped"] == 0
            even, odd = d["by_chain_parity"]["even"], d["by_chain_parity"]["odd"]
            assert even["draws_used"] == odd["draws_used"] == net.size // 2
            assert even["net_positive_draws"] + odd["net_positive_draws"] == d["net_positive_draws"]
            # numpy's exp and the device's differ in the last places: a draw within 1e-9 of a decision boundary may fall either way
            near = int(np.sum(np.abs(net) < 1e-9))
            assert abs(d["net_positive_draws"] - int(np.sum(net > 0.0))) <= near
            top = np.sort(np.stack(block), axis=0)
            close = int(np.sum(top[-1] - top[-2] < 1e-9))
            dominant = np.bincount(np.argmax(np.stack(block), axis=0).ravel(), minlength=3)
            assert np.all(np.abs(np.array([d["dominant_draws"][ch] for ch in rec["channels"]]) - dominant) <= close)
