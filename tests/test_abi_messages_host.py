"""The C ABI's argument checks without a GPU: every faulty call of tests/abi_message_cases.py returns the code and leaves the message
that tests/golden/abi_messages.json recorded (tests/golden/make_golden_abi_messages.py).  The pointers are fake: no launch is reached."""
import json
import os

import pytest

import abi_message_cases
from conftest import REPO

GOLDEN = os.path.join(REPO, "tests", "golden", "abi_messages.json")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from pyhillfit_amd import _lib
    return _lib.load()


def test_messages_and_codes_are_the_recorded_ones(lib):
    from pyhillfit_amd import _lib
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert golden["abi_version"] == _lib.ABI_VERSION
    got = abi_message_cases.run(lib, _lib)
    assert sorted(got) == sorted(golden["cases"])
    wrong = ["%s: %r, recorded %r" % (k, got[k], golden["cases"][k]) for k in sorted(got) if got[k] != golden["cases"][k]]
    assert not wrong, "\n".join(wrong)


def test_table_covers_every_entry_of_the_nine_families():
    from pyhillfit_amd import _lib
    families = ("diagnostics", "batch_means", "comoments", "waic", "psis", "ppc", "quantiles", "sensitivity", "stepping_stone")
    steps = ("_workspace_bytes", "_init", "_accumulate", "_reduce")
    want = {e for e in _lib.EXPORTS if e.startswith(tuple("phf_" + f for f in families)) and any(s in e for s in steps)}
    assert len(want) >= 4 * len(families)
    covered = {entry for _, entry, _, _, _ in abi_message_cases.cases(_lib)}
    assert want <= covered, sorted(want - covered)
    with open(GOLDEN) as f:
        cases = json.load(f)["cases"]
    two_faults = [k for k in cases if "+" in k]
    assert len(two_faults) >= 3 * len(families)
    assert all(rc in (0, -1) or k.split("[")[0].endswith(abi_message_cases.SIZES) for k, (rc, _) in cases.items())
