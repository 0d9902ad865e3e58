"""The on-device run analyses only read the rows: a run of the command line with all of them gives each one the record, the report
line and the files it gets when it runs alone, and leaves the chain files as a run without any.  Single-level: 401 saved rows, burn-in
100, segments of 140 rows (the burn-in ends inside the first segment, the last segment is short).  Hierarchical: a 3-experiment and a
4-experiment pair, so two launch groups."""
import contextlib
import glob
import io
import os
import re

import pytest

from test_gpu_waic import _summaries, csv_file, dr_setup, gpu  # noqa: F401

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ADDED_KEYS = ("diagnostics", "waic", "loo", "loo_experiment", "quantiles", "curve_band", "hierarchical_bands", "ppc", "sensitivity")
BAND_SUFFIX = re.compile(r"; \d+ non-finite band draws$")

# case -> (its flags, the summary keys it adds, the first words of its report lines)
SINGLE_LEVEL = {
    "diagnostics": (["--diagnostics"], ["diagnostics"], ["diagnostics"]),
    "batch_means": (["--diagnostics", "--diagnostic-batch-means"], ["diagnostics"], ["diagnostics", "batch means"]),
    "waic": (["--waic"], ["waic"], ["waic"]),
    "loo": (["--loo"], ["loo"], ["loo"]),
    "quantiles": (["--quantiles"], ["quantiles"], ["quantiles"]),
    "curve_bands": (["--quantiles", "--curve-bands", "8"], ["quantiles", "curve_band"], ["quantiles"]),
    "ppc": (["--ppc"], ["ppc"], ["ppc"]),
    "sensitivity": (["--sensitivity"], ["sensitivity"], ["sensitivity"]),
}
HIERARCHICAL = {
    "predictive_cdfs": (["--predictive-cdfs"], [], []),
    "diagnostics": SINGLE_LEVEL["diagnostics"],
    "batch_means": SINGLE_LEVEL["batch_means"],
    "waic": SINGLE_LEVEL["waic"],
    "loo": SINGLE_LEVEL["loo"],
    "leave_experiment_out": (["--leave-experiment-out", "--marginal-nodes", "32", "--marginal-every", "10"], ["loo_experiment"],
                             ["loo-experiment"]),
    "quantiles": SINGLE_LEVEL["quantiles"],
    "predictive_bands": (["--quantiles", "--predictive-bands", "4"], ["quantiles", "hierarchical_bands"], ["quantiles"]),
    "ppc": SINGLE_LEVEL["ppc"],
    "sensitivity": SINGLE_LEVEL["sensitivity"],
}


def _run(base, flags, root):
    """one run of the command line into root -> (its summaries by relative path, its stdout lines, its other files' bytes)"""
    from pyhillfit_amd import PyHillFit
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        PyHillFit.main(base + flags + ["--output-root", root])
    summaries = {os.path.relpath(p, root): s for p, s in _summaries(root).items()}
    files = {os.path.relpath(p, root): open(p, "rb").read() for p in sorted(glob.glob(os.path.join(root, "**", "*"), recursive=True))
             if os.path.isfile(p) and not p.endswith("_summary.json")}
    return summaries, out.getvalue().splitlines(), files


def _lines(stdout, word):
    return [l for l in stdout if l.startswith(word + " [rank")]


def _check_case(alone, everything, keys, words, band_suffix=False):
    """the case's sections, report lines and files equal those of the run with every analysis"""
    (s_one, out_one, f_one), (s_all, out_all, f_all) = alone, everything
    assert list(s_one) == list(s_all) and len(s_one) == 2
    for path in s_one:
        for k in keys:
            one, both = s_one[path][k], s_all[path][k]
            if k == "diagnostics" and "batch_means" not in one:
                both = {n: v for n, v in both.items() if n != "batch_means"}
            assert one == both, (path, k)
        assert [k for k in s_one[path] if k in ADDED_KEYS] == keys
    for w in words:
        want = _lines(out_all, w)
        if band_suffix:                             # the count of non-finite band draws belongs to --predictive-bands
            want = [BAND_SUFFIX.sub("", l) for l in want]
        assert len(want) == 1 and _lines(out_one, w) == want
    assert f_one and all(f_all[p] == f_one[p] for p in f_one)   # chain files and the rest: byte for byte


def _check_none(none, everything):
    (s_none, out_none, f_none), (s_all, _, f_all) = none, everything
    assert list(s_none) == list(s_all) and len(s_none) == 2
    for path in s_none:
        a = {k: v for k, v in s_none[path].items() if k != "mh_samples_per_second"}
        b = {k: v for k, v in s_all[path].items() if k != "mh_samples_per_second" and k not in ADDED_KEYS}
        assert a == b and not any(k in s_none[path] for k in ADDED_KEYS)
    assert not any(re.match(r"[a-z\- ]+ \[rank", l) and not l.startswith("timing") for l in out_none)
    assert f_none and all(f_all[p] == f_none[p] for p in f_none)


# ---- single-level -----------------------------------------------------------------------------------------------------------------
def _sl_base(csv):
    return ["--data-file", csv, "-m", "2", "-i", "2000", "--drugs", "Amiodarone,Bepridil", "--channels", "hERG", "--num-chains", "64",
            "--segment", "700"]


@pytest.fixture(scope="module")
def sl_all(csv_file, tmp_path_factory):  # noqa: F811
    flags = ["--diagnostics", "--diagnostic-batch-means", "--waic", "--loo", "--quantiles", "--curve-bands", "8", "--ppc", "--sensitivity"]
    return _run(_sl_base(csv_file), flags, str(tmp_path_factory.mktemp("sl_all")))


@pytest.mark.parametrize("case", list(SINGLE_LEVEL))
def test_single_level_alone_equals_all(csv_file, sl_all, tmp_path, case):  # noqa: F811
    flags, keys, words = SINGLE_LEVEL[case]
    _check_case(_run(_sl_base(csv_file), flags, str(tmp_path)), sl_all, keys, words)
    assert sl_all[0][next(iter(sl_all[0]))]["saved_rows_after_burn_in"] == 301


def test_single_level_none(csv_file, sl_all, tmp_path):  # noqa: F811
    _check_none(_run(_sl_base(csv_file), [], str(tmp_path)), sl_all)


# ---- hierarchical -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hier_base(csv_file, dr_setup):  # noqa: F811
    dr = dr_setup
    pick = None
    for ch in dr.channels:                                       # one channel with a 3-experiment and a 4-experiment pair
        by_ne = {}
        for d in dr.drugs:
            try:
                by_ne.setdefault(dr.load_crumb_data(d, ch)[0], d)
            except Exception:
                continue
        if 3 in by_ne and 4 in by_ne:
            pick = (by_ne[3], by_ne[4], ch)
            break
    assert pick is not None
    return ["--data-file", csv_file, "-m", "2", "--hierarchical", "-i", "2000", "--drugs", pick[0] + "," + pick[1], "--channels", pick[2],
            "--num-chains", "64", "--segment", "700"]


@pytest.fixture(scope="module")
def hier_all(hier_base, tmp_path_factory):
    flags = ["--predictive-cdfs", "--diagnostics", "--diagnostic-batch-means", "--waic", "--loo", "--leave-experiment-out",
             "--marginal-nodes", "32", "--marginal-every", "10", "--quantiles", "--predictive-bands", "4", "--ppc", "--sensitivity"]
    run = _run(hier_base, flags, str(tmp_path_factory.mktemp("hier_all")))
    assert sorted(s["num_expts"] for s in run[0].values()) == [3, 4]
    return run


@pytest.fixture(scope="module")
def hier_none(hier_base, tmp_path_factory):
    return _run(hier_base, [], str(tmp_path_factory.mktemp("hier_none")))


@pytest.mark.parametrize("case", list(HIERARCHICAL))
def test_hierarchical_alone_equals_all(hier_base, hier_all, hier_none, tmp_path, case):
    flags, keys, words = HIERARCHICAL[case]
    alone = _run(hier_base, flags, str(tmp_path))
    _check_case(alone, hier_all, keys, words, band_suffix=case == "quantiles")
    if case == "predictive_cdfs":                                # the files the flag adds are all there, and are the all-on run's
        assert set(alone[2]) == set(hier_all[2]) and len(alone[2]) > len(hier_none[2])
    else:
        assert set(alone[2]) == set(hier_none[2])


def test_hierarchical_none(hier_none, hier_all):
    _check_none(hier_none, hier_all)
