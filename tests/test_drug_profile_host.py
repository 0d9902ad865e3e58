"""The drug profile without a GPU: the host build of phf_drug_profile.h (the twin of the kernels) against numpy on the reference's
Verapamil samples, the net block and the integer counts there, the default weights, ties, non-finite draws, the Cmax file, the
command lines' flags, shard_drugs and the C ABI's argument checks."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import REPO
from drug_profile_twin import (CRUMB_CHANNELS, GOLDEN, VERAPAMIL_CMAX_UM, numpy_block, shim, twin_profile, verapamil,  # noqa: F401
                               verapamil_rows)

MULTIPLES = (1.0, 3.0, 10.0)
NET_POSITIVE = (41, 10, 18)             # of 500 draws at 1, 3 and 10 x Cmax


def default_weights(lib, channels):
    return np.array([lib.v_weight(ch.encode()) for ch in channels])


@pytest.fixture(scope="module")
def fixture_profile(shim):  # noqa: F811
    """the twin over the fixture at 1, 3, 10 x 45 nM: (values [3][8][500], tally [3][2][10], weights)"""
    w = default_weights(shim, CRUMB_CHANNELS)
    doses = np.array([[m * VERAPAMIL_CMAX_UM for m in MULTIPLES]])
    values, tally, live = twin_profile(shim, 2, verapamil_rows(), np.arange(7)[None, :], w, doses)
    assert np.all(live == 1)
    return values[0, :, :, :, 0], tally[0], w


def test_twin_values_against_numpy(fixture_profile):
    values, _, _ = fixture_profile
    hill, pic50 = verapamil()
    for j, m in enumerate(MULTIPLES):
        want = numpy_block(np.log(m * VERAPAMIL_CMAX_UM), hill, pic50)
        slack = 1e-12 * np.maximum(np.abs(want), 100.0)        # the slack test_gpu_quantiles.py gives curve values
        assert np.all(np.abs(values[j, :7] - want) <= slack), j


def test_net_block_and_counts_on_the_fixture(fixture_profile):
    values, tally, w = fixture_profile
    assert list(w) == [1.0, -1.0, -1.0, -1.0, 1.0, 1.0, 1.0]
    for j in range(3):
        block = values[j, :7]
        net = np.zeros(500)
        for k in range(7):                                      # the ordered sum, plain multiplies and adds
            net = net + w[k] * block[k]
        assert np.array_equal(values[j, 7], net)
        both = tally[j, 0] + tally[j, 1]
        assert both[7] == NET_POSITIVE[j] == int(np.sum(net > 0.0))
        assert np.array_equal(both[:7], np.bincount(np.argmax(block, axis=0), minlength=7))
        assert both[8] == 500 and both[9] == 0
        assert np.all(tally[j, 1] == 0)                          # one chain: everything is of even parity
    # the margins that make exact equality the condition: the smallest |net| and the smallest gap between the two largest blocks
    assert np.min(np.abs(values[:, 7])) > 0.017
    top = np.sort(values[:, :7], axis=1)
    assert np.min(top[:, -1] - top[:, -2]) > 0.007


def test_default_weights_and_overrides(shim):  # noqa: F811
    from pyhillfit_amd import drug_profile as dp
    assert [shim.v_weight(n) for n in (b"hERG", b"KvLQT1_mink", b"Kv4.3", b"Kir2.1")] == [1.0] * 4
    assert [shim.v_weight(n) for n in (b"Nav1.5-peak", b"Nav1.5-late", b"Cav1.2")] == [-1.0] * 3
    assert [shim.v_weight(n) for n in (b"", b"herg", b"hERGx", b"hER", b"KvLQT1/mink", b"Nav1.5")] == [0.0] * 6
    assert dp.parse_weights("hERG=2,Cav1.2=-0.5, other = 1e-1") == {"hERG": 2.0, "Cav1.2": -0.5, "other": 0.1}
    for bad in ("", "hERG", "hERG=", "=1", "hERG=x", "hERG=nan", "hERG=inf"):
        with pytest.raises(ValueError):
            dp.parse_weights(bad)
    w = dp.default_weights(["hERG", "Cav1.2", "unknown"], {"Cav1.2": -0.25})      # the library's, the same header
    assert list(w) == [1.0, -0.25, 0.0]
    with pytest.raises(ValueError, match="not there"):
        dp.default_weights(["hERG"], {"Cav1.2": 1.0})


def test_ties_go_to_the_lowest_index(shim):  # noqa: F811
    rows = np.zeros((2, 3, 2, 4))
    rows[:, :, 0] = 6.0
    rows[:, :, 1] = 1.0
    rows[1, 2, 0, :] = 6.5                                       # row 1: channel 2 alone is the largest
    rows[0, 0, 0, 3] = 5.0                                       # row 0, chain 3: channels 1 and 2 tie above channel 0
    values, tally, _ = twin_profile(shim, 2, rows, [[0, 1, 2]], [1.0, 1.0, 1.0], [[1.0]])
    assert values[0, 0, 0, 0, 0] == values[0, 0, 1, 0, 0] == values[0, 0, 2, 0, 0]            # a three-way tie
    assert values[0, 0, 1, 0, 3] == values[0, 0, 2, 0, 3] > values[0, 0, 0, 0, 3]
    both = tally[0, 0, 0] + tally[0, 0, 1]
    assert list(both[:3]) == [3, 1, 4]
    assert list(tally[0, 0, 1][:3]) == [1, 1, 2]                 # the odd chains 1 and 3


def test_non_finite_draws_are_counted_apart(shim):  # noqa: F811
    rng = np.random.default_rng(3)
    rows = np.zeros((5, 4, 2, 6))
    rows[:, :, 0] = rng.normal(5.5, 0.5, (5, 4, 6))
    rows[:, :, 1] = rng.uniform(0.5, 2.0, (5, 4, 6))
    rows[1, 0, 0, 2] = np.nan                                    # pIC50 of drug 0's channel 0
    rows[3, 2, 1, 5] = np.inf                                    # Hill of drug 0's channel 2
    rows[2, 3, 0, 1] = np.nan                                    # pIC50 of drug 1's only channel
    cp = [[0, 1, 2], [-1, 3, -1]]
    values, tally, live = twin_profile(shim, 2, rows, cp, [1.0, -1.0, 1.0], [[0.3, 3.0], [0.3, 3.0]])
    bad = ~np.isfinite(values)
    assert live.tolist() == [[[1, 1, 1, 1]] * 2, [[0, 1, 0, 1]] * 2]
    for j in range(2):
        want = np.zeros((4, 5, 6), dtype=bool)
        want[0, 1, 2] = want[3, 1, 2] = True                     # the channel's slot and the net slot, nowhere else
        want[2, 3, 5] = want[3, 3, 5] = True
        assert np.array_equal(bad[0, j], want)
        both = tally[0, j, 0] + tally[0, j, 1]
        assert both[4] == 28 and both[5] == 2 and both[:3].sum() == 28
        assert tally[0, j, 0][5] == 1 and tally[0, j, 1][5] == 1
        want1 = np.zeros((5, 6), dtype=bool)
        want1[2, 1] = True
        assert np.array_equal(bad[1, j, 1], want1) and np.array_equal(bad[1, j, 3], want1)
        assert np.all(bad[1, j, 0]) and np.all(bad[1, j, 2])      # never fed
        both = tally[1, j, 0] + tally[1, j, 1]
        assert both[4] == 29 and both[5] == 1 and both[1] == 29 and both[0] == both[2] == 0
    # model 1 does not read the Hill column
    values1, tally1, _ = twin_profile(shim, 1, rows, cp, [1.0, -1.0, 1.0], [[0.3, 3.0], [0.3, 3.0]])
    assert (tally1[0, 0, 0] + tally1[0, 0, 1])[5] == 1 and np.isfinite(values1[0, 0, 2, 3, 5])


def test_a_dose_the_drug_does_not_have_is_never_fed(shim):  # noqa: F811
    rows = np.full((3, 2, 2, 2), 6.0)
    values, tally, live = twin_profile(shim, 2, rows, [[0], [1]], [1.0], [[0.1, 1.0], [0.1, np.nan]])
    assert live[:, :, 0].tolist() == [[1, 1], [1, 0]] and live[:, :, 1].tolist() == [[1, 1], [1, 0]]
    assert np.all(tally[1, 1] == 0) and tally[1, 0].sum() == tally[0, 1].sum() > 0


def test_cmax_file():
    from pyhillfit_amd import drug_profile as dp
    cmax = dp.read_cmax(os.path.join(GOLDEN, "drug_list.txt"))
    assert len(cmax) == 30 and cmax["Verapamil"] == 45.0 / 1000.0 and cmax["Amiodarone"] == 0.7 / 1000.0
    assert "Drug" not in cmax and "NoSuchDrug" not in cmax
    assert dp.doses_of("Verapamil", None, cmax, (1.0, 3.0, 10.0)) == [0.045, 3.0 * 0.045, 10.0 * 0.045]
    assert dp.doses_of("NoSuchDrug", None, cmax, (1.0, 3.0, 10.0)) is None
    assert dp.doses_of("NoSuchDrug", (0.5,), cmax, (1.0,)) == [0.5]
    plan = dp.Plan([("Verapamil", "hERG"), ("NoSuchDrug", "hERG"), ("Verapamil", "Cav1.2"), ("Quinidine", "Cav1.2")],
                   CRUMB_CHANNELS, None, cmax, (1.0, 3.0))
    assert plan.drugs == ["Verapamil", "Quinidine"] and plan.skipped == ["NoSuchDrug"] and plan.channels == ["hERG", "Cav1.2"]
    assert plan.map.tolist() == [[0, 2], [-1, 3]] and list(plan.weights) == [1.0, -1.0]
    assert plan.doses.shape == (2, 2) and plan.doses[0, 1] == 3.0 * 0.045 and plan.first_problem(1) == 3
    both = dp.Plan([("Verapamil", "hERG"), ("NoSuchDrug", "hERG")], CRUMB_CHANNELS, (0.5,), cmax, (1.0,))
    assert both.skipped == [] and both.doses[0].tolist() == [0.045, 0.5] and both.doses[1, 0] == 0.5 and np.isnan(both.doses[1, 1])


def test_cmax_file_refusals(tmp_path):
    from pyhillfit_amd import drug_profile as dp
    for body in ("Drug EFTPCmax(nM)\nA x 1\n", "Drug EFTPCmax(nM)\nA\n", "Drug EFTPCmax(nM)\nA -3\n"):
        f = tmp_path / "list.txt"
        f.write_text(body)
        with pytest.raises(ValueError):
            dp.read_cmax(str(f))


def _args(*flags):
    from pyhillfit_amd import PyHillFit
    p = PyHillFit.build_parser()
    a = p.parse_args(["--data-file", "x.csv", "-m", "2"] + list(flags))
    PyHillFit.check_args(p, a)
    return a


def test_concentration_flags():
    from pyhillfit_amd import analyses as an
    a = _args()
    assert a.drug_profile is False and an.DrugProfile not in an.fit_analyses(a)
    a = _args("--drug-profile-concs", "0.045,0.45")
    assert a.drug_profile and a.drug_profile_concs == (0.045, 0.45) and a.drug_profile_bins == 4096 and a.drug_profile_cmax is None
    assert an.fit_analyses(a) == [an.DrugProfile]
    a = _args("--savage-dickey", "--drug-profile-cmax", os.path.join(GOLDEN, "drug_list.txt"), "--drug-profile-bins", "64",
              "--drug-profile-weights", "hERG=2")
    assert a.drug_profile_cmax["Verapamil"] == 0.045 and a.drug_profile_multiples == (1.0, 3.0, 10.0) and a.drug_profile_bins == 64
    assert a.drug_profile_weights == {"hERG": 2.0} and an.fit_analyses(a) == [an.SavageDickeyBF, an.DrugProfile]
    assert _args("--drug-profile-cmax", os.path.join(GOLDEN, "drug_list.txt"), "--drug-profile-multiples", "2,4").drug_profile_multiples == (2.0, 4.0)


@pytest.mark.parametrize("extra,word", [
    (["--drug-profile-concs", ",".join(str(i + 1) for i in range(17))], "1 to 16"),
    (["--drug-profile-concs", "1,2,3,4,5,6,7,8,9,10,11,12,13,14", "--drug-profile-cmax", os.path.join(GOLDEN, "drug_list.txt")], "at most 16"),
    (["--drug-profile-concs", "0.1,-1"], "> 0"),
    (["--hierarchical", "--drug-profile-concs", "0.1"], "pyhillfit_amd.drug_profile"),
    (["--drug-profile-concs", "0.1", "--drug-profile-multiples", "1,2"], "needs --drug-profile-cmax"),
    (["--drug-profile-multiples", "1,2"], "needs --drug-profile-concs or --drug-profile-cmax"),
    (["--drug-profile-weights", "hERG=1"], "needs --drug-profile-concs or --drug-profile-cmax"),
    (["--drug-profile-bins", "64"], "needs --drug-profile-concs or --drug-profile-cmax"),
    (["--drug-profile-concs", "0.1", "--drug-profile-bins", "100"], "power of two"),
    (["--drug-profile-cmax", "no-such-file.txt"], "no-such-file.txt"),
])
def test_flag_refusals(extra, word, capsys):
    from pyhillfit_amd import PyHillFit
    with pytest.raises(SystemExit) as e:
        PyHillFit.main(["--data-file", "does-not-exist.csv", "-m", "2"] + extra)
    assert e.value.code == 2 and word in capsys.readouterr().err


def test_tool_flags(capsys):
    from pyhillfit_amd import drug_profile as dp
    ap = dp.build_parser()
    a, named, doses, cmax, multiples, weights, probs = dp.parse_tool_args(ap, ["--cmax-nM", "45", "--channel", "hERG=a.txt,b.txt",
                                                                               "--channel", "Cav1.2=c.npy", "--weights", "hERG=2"])
    assert named == [("hERG", ["a.txt", "b.txt"]), ("Cav1.2", ["c.npy"])] and doses == [0.045, 3 * 0.045, 10 * 0.045]
    assert cmax == 0.045 and weights == {"hERG": 2.0} and probs is None
    for bad in (["--channel", "hERG=a.txt"], ["--concs", "1", "--channel", "hERG"], ["--concs", "1", "--multiples", "2", "--channel", "h=a"],
                ["--concs", "1", "--channel", "h=a", "--channel", "h=b"], ["--concs", "1", "--channel", "h=a", "--weights", "x=1"],
                ["--concs", "1", "--channel", "h=a", "--bins", "100"]):
        with pytest.raises(SystemExit):
            dp.parse_tool_args(ap, bad)


def test_shard_drugs():
    from pyhillfit_amd.distributed import shard_drugs
    rng = np.random.default_rng(11)
    drugs = [d for d in "ABCDEFGHIJK" for _ in range(rng.integers(1, 8))]
    order = rng.permutation(len(drugs))
    drug_of = [drugs[i] for i in order]
    costs = rng.integers(0, 60, len(drugs)).astype(float)
    for world in (1, 2, 3, 8, 16):
        parts = shard_drugs(costs, drug_of, world)
        assert len(parts) == world
        assert sorted(np.concatenate(parts).tolist()) == list(range(len(drugs)))          # every problem once
        owner = {}
        for r, part in enumerate(parts):
            for q in part:
                assert owner.setdefault(drug_of[q], r) == r                                 # no drug is split
        again = shard_drugs(list(costs), list(drug_of), world)
        assert all(np.array_equal(a, b) for a, b in zip(parts, again))                      # deterministic
        loads = [costs[p].sum() for p in parts]
        per_drug = max(costs[[q for q, d in enumerate(drug_of) if d == name]].sum() for name in set(drug_of))
        assert max(loads) - min(loads) <= per_drug                                          # greedy: within one drug of each other
    assert [p.tolist() for p in shard_drugs([1, 1, 5, 1], ["a", "b", "c", "a"], 2)] == [[2], [0, 1, 3]]


# ---- the C ABI without a GPU ---------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ["phf_drug_profile_workspace_bytes", "phf_drug_profile_tally_offset", "phf_drug_profile_default_weight",
               "phf_drug_profile_init", "phf_drug_profile_accumulate", "phf_drug_profile_reduce"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from pyhillfit_amd import _lib
    return _lib.load()


def test_symbols_declared_and_exported(lib, shim):  # noqa: F811
    from pyhillfit_amd import _lib
    with open(os.path.join(REPO, "include", "pyhillfit_amd.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(lib, name) and (name + "(") in header, name
    assert _lib.ABI_VERSION == 7 and lib.phf_version() == 7
    for ch in CRUMB_CHANNELS + ["other"]:
        assert lib.phf_drug_profile_default_weight(ch.encode()) == shim.v_weight(ch.encode())
    assert shim.v_max_channels() == 16 and shim.v_max_doses() == 16


def test_abi_validation(lib):
    S = 2 * 3 * (7 + 1)
    grid = S * 256 * 8 + S * 8 * 8 + S * 8
    assert lib.phf_drug_profile_tally_offset(2, 7, 3, 256) == grid == lib.phf_quantiles_workspace_bytes(2, 0, 3 * 8, 256)
    assert lib.phf_drug_profile_workspace_bytes(2, 7, 3, 256) == grid + 2 * 3 * 2 * 10 * 8
    for bad in [(0, 7, 3, 256), (2, 0, 3, 256), (2, 17, 3, 256), (2, 7, 0, 256), (2, 7, 17, 256), (2, 7, 3, 100), (2, 7, 3, 32), (2, 7, 3, 65536)]:
        assert lib.phf_drug_profile_workspace_bytes(*bad) == 0 and lib.phf_last_error(), bad
        assert lib.phf_drug_profile_tally_offset(*bad) == 0
    assert lib.phf_drug_profile_workspace_bytes(2, 7, 17, 256) == 0 and b"num_doses in [1, 16]" in lib.phf_last_error()
    fake, big = C.c_void_p(8), C.c_size_t(1 << 40)
    assert lib.phf_drug_profile_init(2, 7, 3, 256, None, big, None) == -1 and b"null" in lib.phf_last_error()
    assert lib.phf_drug_profile_init(2, 7, 3, 256, fake, C.c_size_t(16), None) == -1 and b"smaller" in lib.phf_last_error()
    assert lib.phf_drug_profile_init(2, 7, 3, 1000, fake, big, None) == -1 and b"power of two" in lib.phf_last_error()

    def acc(n=10, Q=9, stride=4, chains=64, model=2, drugs=2, K=7, D=3, cp=fake, w=fake, doses=fake, B=256, first=0, total=100, ws=fake,
            wsb=big, rows=fake):
        return lib.phf_drug_profile_accumulate(rows, n, Q, stride, chains, model, drugs, K, D, cp, w, doses, B, first, total, ws, wsb, None)
    assert acc(model=3) == -1 and b"model" in lib.phf_last_error()
    assert acc(K=17) == -1 and b"num_channels" in lib.phf_last_error()
    assert acc(D=17) == -1 and b"num_doses" in lib.phf_last_error()
    assert acc(B=100) == -1 and b"power of two" in lib.phf_last_error()
    assert acc(Q=0) == -1 and b"positive" in lib.phf_last_error()
    assert acc(stride=1) == -1 and b"row_stride_cols" in lib.phf_last_error()
    assert acc(stride=1, model=1, n=0) == 0
    assert acc(first=95) == -1 and b"total_rows" in lib.phf_last_error()
    assert acc(n=1 << 20, chains=4096, total=1 << 21) == -1 and b"2^31" in lib.phf_last_error()
    for name in ("cp", "w", "doses"):
        assert acc(**{name: None}) == -1 and b"null channel_problem, weights or ln_doses" in lib.phf_last_error()
    assert acc(rows=None) == -1 and b"null rows" in lib.phf_last_error()
    assert acc(ws=None) == -1 and b"null workspace" in lib.phf_last_error()
    assert acc(wsb=C.c_size_t(8)) == -1 and b"phf_drug_profile_workspace_bytes" in lib.phf_last_error()
    assert acc(n=0, first=100) == 0                                # nothing to do: no launch

    probs = (C.c_double * 3)(0.1, 0.5, 0.9)
    assert lib.phf_drug_profile_reduce(2, 7, 3, 256, probs, 3, None, big, fake, None) == -1 and b"null workspace" in lib.phf_last_error()
    assert lib.phf_drug_profile_reduce(2, 7, 3, 256, probs, 3, fake, C.c_size_t(grid), fake, None) == -1 and b"smaller" in lib.phf_last_error()
    assert lib.phf_drug_profile_reduce(2, 7, 3, 256, probs, 0, fake, big, fake, None) == -1
    assert lib.phf_drug_profile_reduce(2, 7, 3, 256, (C.c_double * 1)(1.5), 1, fake, big, fake, None) == -1 and b"[0, 1]" in lib.phf_last_error()
    assert lib.phf_drug_profile_reduce(2, 7, 3, 256, probs, 3, fake, big, None, None) == -1 and b"null out" in lib.phf_last_error()
    assert lib.phf_drug_profile_reduce(2, 17, 3, 256, probs, 3, fake, big, fake, None) == -1 and b"num_channels" in lib.phf_last_error()


def test_records(shim):  # noqa: F811
    """json_record and report_line from a result() built by hand from the twin's tallies (the device's are tested on the GPU)"""
    from pyhillfit_amd import drug_profile as dp
    K, D, P = 2, 1, 3
    tally = np.array([[[[5, 3, 2, 8, 1], [4, 4, 6, 8, 0]]]])
    z = np.zeros((1, D * (K + 1)))
    per = np.zeros((1, D * (K + 1), P))
    per[0, 2] = [-3.0, 1.0, 4.0]
    res = {"min": z, "max": z, "draws": z + 16, "non_finite": z, "bin_width": z + 0.1, "level": z, "value": per, "lo": per - 0.05,
           "hi": per + 0.05, "bin": per, "probs": np.array([0.025, 0.5, 0.975]), "tally": tally, "K": K, "D": D, "bins": 64, "model": 2,
           "chains": 2, "rows": 8, "loaded": np.array([[True, True]]), "doses": np.array([[0.045]]), "weights": np.array([1.0, -1.0])}
    rec = dp.json_record(res, 0, "Verapamil", ["hERG", "Cav1.2"], 0.045, (1.0,))
    json.dumps(rec)
    d0 = rec["doses"][0]
    assert d0["draws_used"] == 16 and d0["draws_skipped"] == 1 and d0["net_positive_draws"] == 8 and d0["p_net_positive"] == 0.5
    assert d0["dominant_draws"] == {"hERG": 9, "Cav1.2": 7} and d0["dominant_probability"]["hERG"] == 9 / 16
    assert d0["by_chain_parity"]["even"]["p_net_positive"] == 0.25 and d0["by_chain_parity"]["odd"]["p_net_positive"] == 0.75
    assert d0["net"]["ci95"] == [-3.0, 4.0] and "convention" in rec["weights_note"] and rec["weights"] == {"hERG": 1.0, "Cav1.2": -1.0}
    assert "not an action-potential prediction" in rec["method"]
    line = dp.report_line(0, [rec], ["NoSuchDrug"])
    assert line.startswith("drug-profile [rank 0]: 1 drugs") and "Verapamil at 0.045 uM" in line and "NoSuchDrug" in line
    assert dp.report_line(1, [], ["X"]) == "drug-profile [rank 1]: 0 drugs; 0 draws skipped; skipped, no Cmax: X"


def test_drug_profile_file(tmp_path):
    from pyhillfit_amd import doseresponse as dr
    old_root, old_dir = dr.output_root, getattr(dr, "dir_name", None)
    try:
        dr.output_root, dr.dir_name = str(tmp_path), "crumb_data"
        path = dr.drug_profile_file("Verapamil")
        assert path == "{}/crumb_data/single-level/Verapamil/drug_profiles/Verapamil_drug_profile.json".format(tmp_path)
        assert os.path.isdir(os.path.dirname(path))
    finally:
        dr.output_root, dr.dir_name = old_root, old_dir
