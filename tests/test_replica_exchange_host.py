"""Replica exchange without a GPU: the partition of PyHillTemp keeps every pair's rungs on one rank, --swap-every refuses K < 0, the C
ABI's argument validation, the standard errors over replica sets against direct restatements, and the per-pair records."""
import ctypes as C
import math

import numpy as np
import pytest

from pyhillfit_amd import PyHillTemp
from pyhillfit_amd import replica_exchange as rxm


@pytest.mark.parametrize("pairs,world", [(1, 1), (1, 4), (5, 3), (7, 8), (210, 8)])
def test_partition_keeps_pairs_whole(pairs, world):
    R = 41
    rng = np.random.default_rng(pairs + world)
    points = rng.integers(4, 20, pairs)
    parts = PyHillTemp.partition_units(points, R, world, whole_pairs=True)
    assert len(parts) == world
    allu = np.sort(np.concatenate(parts))
    assert np.array_equal(allu, np.arange(pairs * R))
    for p in parts:
        assert np.array_equal(p, np.sort(p))
        assert len(p) % R == 0
        for i in range(0, len(p), R):                                   # whole pairs, rungs in order: what the swap kernel needs
            assert np.array_equal(p[i:i + R], p[i] + np.arange(R)) and p[i] % R == 0
    assert sum(len(p) == 0 for p in parts) == max(0, world - pairs)
    # without swaps the partition is the one it always was
    assert all(np.array_equal(a, b) for a, b in zip(PyHillTemp.partition_units(points, R, world),
                                                    PyHillTemp.partition_units(points, R, world, whole_pairs=False)))


def test_negative_swap_interval_is_refused(capsys):
    with pytest.raises(SystemExit) as e:
        PyHillTemp.main(["--data-file", "unused.csv", "-m", "1", "-d", "0", "-c", "0", "--swap-every", "-1"])
    assert e.value.code == 2 and "--swap-every" in capsys.readouterr().err
    assert PyHillTemp.build_parser().parse_args(["--data-file", "x", "-m", "1", "-d", "0", "-c", "0"]).swap_every == 0


@pytest.fixture(scope="module")
def lib():
    from pyhillfit_amd import _lib
    return _lib.load()


def test_abi_validation(lib):
    assert lib.phf_replica_exchange_stats_bytes(3, 6, 128) == (2 * 3 * 5 * 2 + 3 * 128) * 8
    assert lib.phf_replica_exchange_stats_bytes(1, 2, 65) == (2 * 1 * 1 * 2 + 65) * 8
    for bad in [(0, 6, 64), (3, 1, 64), (3, 6, 0), (1 << 16, 1 << 10, 1 << 10)]:
        assert lib.phf_replica_exchange_stats_bytes(*bad) == 0
        assert lib.phf_last_error()
    assert lib.phf_replica_exchange_stats_init(3, 6, 64, None, C.c_size_t(1 << 20), None) != 0
    assert lib.phf_replica_exchange_labels_init(3, 1, 64, None, None) != 0
    assert lib.phf_replica_exchange_round(None, 1, 6, 1, 1, None, None, None, C.c_size_t(0), None, None) != 0
    assert b"null problems" in lib.phf_last_error()
    assert lib.phf_stepping_stone_reduce_joint(0, 6, 64, 10, None, C.c_size_t(0), None, None, None) != 0


def acc_from_draws(ll, delta):
    from pyhillfit_amd import stepping_stone as ss
    return ss.chain_accumulators(ll, delta)


def test_joint_se_is_the_delta_method_over_replica_sets():
    from pyhillfit_amd import stepping_stone as ss
    rng = np.random.default_rng(3)
    P, R, Cn, n = 2, 5, 40, 60
    t = np.array([0.0, 0.05, 0.2, 0.6, 1.0])
    dl = ss.deltas(t)
    acc = {k: np.zeros((P * R, Cn)) for k in ss.FIELDS}
    lr = np.zeros((P * R, Cn)); pooled = np.zeros(P * R)
    for q in range(P * R):
        ll = rng.normal(-30.0 + q, 4.0, (Cn, n))
        a = acc_from_draws(ll, dl[q % R])
        for k in ss.FIELDS:
            acc[k][q] = a[k]
        f = ss.finalize(a)
        lr[q], pooled[q] = f["log_r_chains"], f["log_r"]
    got = rxm.joint_se_numpy(acc, pooled, P, R)
    for p in range(P):
        v = sum(np.exp(lr[p * R + k] - pooled[p * R + k]) for k in range(R - 1))
        assert got[p] == pytest.approx(np.std(v, ddof=1) / math.sqrt(Cn), rel=1e-13)
    # with independent rungs it agrees with sqrt(sum se_k^2) to within its own sampling error
    se_k = np.array([ss.finalize({k: acc[k][q] for k in ss.FIELDS})["se"] for q in range(R - 1)])
    assert got[0] == pytest.approx(np.sqrt(np.sum(se_k ** 2)), rel=0.5)


def test_replica_set_ti_se():
    from pyhillfit_amd import doseresponse as dr
    rng = np.random.default_rng(5)
    t = dr.temperature_ladder(6)
    P, R, Cn = 3, len(t), 50
    ll1 = rng.normal(-40.0, 2.0, (P * R, Cn))
    got = rxm.replica_set_ti_se(ll1, t, P)
    for p in range(P):
        per_chain = [dr.trapezium_rule(t, ll1[p * R:(p + 1) * R, c]) for c in range(Cn)]
        assert got[p] == pytest.approx(np.std(per_chain, ddof=1) / math.sqrt(Cn), rel=1e-12)


def test_records():
    P, R, Cn = 2, 4, 64
    stats = {"attempts": np.array([[640, 576, 640], [640, 576, 640]]), "accepts": np.array([[600, 100, 320], [0, 0, 0]]),
             "round_trips": np.arange(P * Cn).reshape(P, Cn) % 3}
    v = rxm.unit_columns(stats, 200, P, R, se_joint=np.array([0.01, 0.02]), ti_se=np.array([0.03, np.nan]))
    assert v.shape == (P * R, len(rxm.UNIT_COLUMNS))
    t = [0.0, 0.1, 0.5, 1.0]
    rec = rxm.json_record(v[:R], t, Cn, 10)
    assert rec["accept_rate"] == [600 / 640, 100 / 576, 0.5] and rec["lowest_accept_rung_pair"] == [1, 2]
    assert rec["rounds"] == 200 and rec["round_trips"] == int(stats["round_trips"][0].sum())
    assert rec["round_trips_per_replica_set"] == stats["round_trips"][0].sum() / Cn
    assert "lowest accept rate 0.174 between rungs 1 and 2" in rxm.report_line("A", "B", 1, rec, t)
    rungs = [{} for _ in range(P * R)]
    tis = [{}, {}]
    ss_recs = [{"se": 1.0}, {"se": 2.0}]
    rows = np.zeros((P * R, 3))
    rows[:, 0] = np.repeat(np.arange(P), R); rows[:, 1] = np.tile(np.arange(R), P)
    gathered = np.concatenate([rows, v], axis=1)[::-1]                  # any order
    PyHillTemp.attach_replica_exchange(rungs, tis, gathered, 3, t, Cn, 10, ss_recs)
    assert [r["swap_accept_rate"] for r in rungs[:R]] == rec["accept_rate"] + [None]
    assert tis[0]["expectation_se_replica_sets"] == 0.03 and tis[1]["expectation_se_replica_sets"] is None
    assert ss_recs[1] == {"se": 0.02, "se_independent_rungs": 2.0, "se_method": "replica_sets"}
    assert tis[1]["replica_exchange"]["accept_rate"] == [0.0, 0.0, 0.0]
