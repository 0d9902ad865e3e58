"""The steady bodies with their wave-uniform work on the scalar unit ("round 11": Philox round 1's uniform word and
round 2's product from scalar copies of two key words, no temperature-0 select in the straight-line bodies, the shared Hill denominators'
LDS offsets computed once per call) on the GPU (-m gpu), bit for bit against the scalar CPU twin and against the same library with
PHF_SL_STEADY=0 (every call on the general iteration, which keeps the parent's forms).

One launch of seven problems: three Crumb pairs, one each of the shapes 4 uncensored + 1 censored entry (its Hill denominator shared: the
body that reads a slot at a precomputed offset),
4 + 0 and 0 + 2, at temperature 1, and the 4 + 1 pair again at temperatures 0, 0.5, -0.0 and NaN (0, -0.0 and NaN run the run-time-loop
body, which keeps the select).  3 200 iterations from t = 0 with adapt_start = 3 000: the call crosses it and ends in a steady body.
Run plain, and through the queued entry point with two quanta and chain_id_base = 2^32 - 64 (chain numbers wrap past 2^32 - 1):
  - with 64 chains per problem: seven wavefronts, each with a SIMD to itself — the lone-wavefront build, whose key words stay scalar;
  - with just over two wavefronts per SIMD of the chip in all: the two-wavefront build, which is the one that draws through
    phf_philox_mh_t_uniform, and which the library does run as a queue.
PHF_SL_STEADY is read once per process, so the runs are made by two fresh child processes; they hand back the checked lanes and a digest
of everything."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED, T, ADAPT = 4242, 3200, 3000
NAMES = [("Amiodarone", "Nav1.5-late"), ("Amiodarone", "Kv4.3"), ("Rufinamide", "Kir2.1")]
SHAPES = [(4, 1), (4, 0), (0, 2)]
PAIR_INDEX = [0, 1, 2, 0, 0, 0, 0]
TEMPS = [1.0, 1.0, 1.0, 0.0, 0.5, -0.0, float("nan")]
THETA0 = [5.0, 1.0, 9.0]
BASE_WRAP = 2 ** 32 - 64
# name -> (wide, queue_quanta, chain_id_base, thinning)
RUNS = {"lone_plain": (False, 0, 0, 5), "lone_queued": (False, 2, BASE_WRAP, 5),
        "wide_plain": (True, 0, 0, 400), "wide_queued": (True, 2, BASE_WRAP, 400)}

CHILD = r"""
import hashlib
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import torch
from test_gpu_sl_uniform import NAMES, PAIR_INDEX, RUNS, SEED, T, ADAPT, TEMPS, THETA0, lanes_of
from pyhillfit_amd import _lib
from pyhillfit_amd import doseresponse as dr
from pyhillfit_amd.sampler import SingleLevelSampler
dr.setup(sys.argv[1] + "/data/crumb_dataset.json")
dr.define_model(2)
packed = dr.pack_single_level(NAMES)
slots = 2 * int(_lib.load().phf_simd_count())
out = {"counts": np.asarray(packed.counts)}
for name, (wide, quanta, base, thin) in RUNS.items():
    chains = 64 * (slots // len(PAIR_INDEX) + 1) - 63 if wide else 64          # wide: just over `slots` blocks, a ragged last block each
    s = SingleLevelSampler(packed, 2, PAIR_INDEX, TEMPS, chains, thinning=thin, seed=SEED, adapt_start=ADAPT, chain_id_base=base,
                           device="cuda:0", queue_quanta=quanta)
    s.init(THETA0, cov_identity=False, cov_scale=0.05)
    rows = s.advance(T).cpu().numpy()
    state = s.state.cpu().numpy().reshape(s.S, len(PAIR_INDEX), chains)
    s.check_queue()
    torch.cuda.synchronize()
    acc = state[2 * s.d + 2 + s.d * (s.d + 1) // 2] / T                       # the call's accept count over its length (one host division)
    queue = np.zeros(1, dtype=np.int32) if s._queue is None else s._queue.cpu().numpy()
    lanes = lanes_of(chains)
    out[name + "/chains"] = np.array(chains)
    out[name + "/blocks"] = np.array(s.nblocks)
    out[name + "/slots"] = np.array(slots)
    out[name + "/queue"] = queue
    out[name + "/rows"] = rows[:, :, :, lanes]
    out[name + "/state"] = state[:, :, lanes]
    out[name + "/acceptance"] = acc[:, lanes]
    out[name + "/digest"] = np.frombuffer(hashlib.sha256(rows.tobytes() + state.tobytes() + acc.tobytes()).digest(), dtype=np.uint8)
np.savez(sys.argv[2], **out)
"""


def lanes_of(chains):
    return sorted({0, 1, 31, 63, chains - 1} | ({64, chains - 64} if chains > 64 else set()))


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """the four runs of RUNS, by the library as it is ("default") and with PHF_SL_STEADY=0 ("off")"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    d = tmp_path_factory.mktemp("sl_uniform")
    script = d / "child.py"
    script.write_text(CHILD)
    got = {}
    for name, value in (("default", None), ("off", "0")):
        env = {k: v for k, v in os.environ.items() if k != "PHF_SL_STEADY"}
        if value is not None:
            env["PHF_SL_STEADY"] = value
        path = d / (name + ".npz")
        subprocess.run([sys.executable, str(script), REPO, str(path)], env=env, check=True, timeout=300)
        got[name] = dict(np.load(str(path)))
    return got


@pytest.fixture(scope="module")
def twin():
    """per run name: rows [R][Q][4][lanes], final state [S][Q][lanes] and log-prior of every saved row [R][Q][lanes] from the CPU twin —
    computed once per (thinning, chain number) and shared"""
    from oracle import c_oracle as co
    from pyhillfit_amd import doseresponse as dr
    from pyhillfit_amd.sampler import gamma_table
    dr.setup(os.path.join(REPO, "data", "crumb_dataset.json"))
    dr.define_model(2)
    gam = gamma_table(T)
    pks = []
    for q, p in enumerate(PAIR_INDEX):
        ne, _, ex = dr.load_crumb_data(*NAMES[p])
        concs, y = dr.concatenate_experiments(ne, ex)
        pks.append(co.PackedPair(concs, y, 2, TEMPS[q]))
    cache = {}

    def one(q, thin, chain_id):
        key = (q, thin, chain_id)
        if key not in cache:
            st = pks[q].init_state(THETA0, False, 0.05)
            rows = pks[q].advance(st, 0, T, thin, ADAPT, False, gam, seed=SEED, chain_id=chain_id, problem_id=q)
            prior = np.array([pks[q].log_prior(r[:3]) for r in rows])
            cache[key] = (rows, st, prior)
        return cache[key]

    def of(name, chains):
        _, _, base, thin = RUNS[name]
        lanes = lanes_of(chains)
        per = [[one(q, thin, (base + c) % 2 ** 32) for c in lanes] for q in range(len(PAIR_INDEX))]
        rows = np.array([[per[q][i][0] for i in range(len(lanes))] for q in range(len(PAIR_INDEX))]).transpose(2, 0, 3, 1)
        state = np.array([[per[q][i][1] for i in range(len(lanes))] for q in range(len(PAIR_INDEX))]).transpose(2, 0, 1)
        prior = np.array([[per[q][i][2] for i in range(len(lanes))] for q in range(len(PAIR_INDEX))]).transpose(2, 0, 1)
        return rows, state, prior
    return of


def test_the_pairs_have_the_shapes_and_the_launches_the_builds(runs):
    from test_sl_shared_denominators import share_map
    from pyhillfit_amd import doseresponse as dr
    dr.setup(os.path.join(REPO, "data", "crumb_dataset.json"))
    dr.define_model(2)
    p = dr.pack_single_level(NAMES)
    assert [(int(c[0]), int(c[1] + c[2])) for c in p.counts] == SHAPES
    assert share_map(p.ln_conc[0, :5], 4, 1) == [0]                       # the censored entry sits at the first uncensored entry's dose
    assert (p.ln_conc[:, :5][np.isfinite(p.ln_conc[:, :5])] > -50.0).all()   # (straight-line bodies: no dose needs the lower clamp)
    d = runs["default"]
    for name, (wide, quanta, _, _) in RUNS.items():
        blocks, slots = int(d[name + "/blocks"]), int(d[name + "/slots"])
        if wide:
            assert slots < blocks <= 16 * slots                            # more than one wavefront per SIMD: the two-wavefront build
            if quanta:                                                     # ... and run as a queue of two quanta per block
                qw = d[name + "/queue"]
                assert qw[-1] == 0 and qw[0] >= 2 * blocks and (qw[1:1 + blocks] == 2).all()
        else:
            assert blocks == 7 and blocks <= slots // 2                    # a SIMD per wavefront: the lone-wavefront build


@pytest.mark.parametrize("name", sorted(RUNS))
def test_bit_identical_to_the_twin(name, runs, twin):
    d = runs["default"]
    chains = int(d[name + "/chains"])
    rows, state, _ = twin(name, chains)
    assert d[name + "/rows"].shape == (T // RUNS[name][3], 7, 4, len(lanes_of(chains)))
    for q in range(7):
        assert _same_bits(d[name + "/rows"][:, q], rows[:, q]), (name, q)
        assert _same_bits(d[name + "/state"][:, q], state[:, q]), (name, q)
    nacc = state[2 * 3 + 2 + 6]                                             # accepts of the call, an integer: the acceptance is its one division
    assert _same_bits(d[name + "/acceptance"], nacc / T)
    assert (nacc[:6] > 0).all() and (nacc[:6] < T).all()                    # both outcomes occurred in every live problem


@pytest.mark.parametrize("name", sorted(RUNS))
def test_bit_identical_to_the_general_iteration(name, runs):
    a, b = runs["default"], runs["off"]
    assert int(a[name + "/chains"]) == int(b[name + "/chains"])
    assert a[name + "/digest"].tobytes() == b[name + "/digest"].tobytes()  # rows, states and acceptance of EVERY chain
    for what in ("rows", "state", "acceptance"):
        assert _same_bits(a[name + "/" + what], b[name + "/" + what]), (name, what)


@pytest.mark.parametrize("name", sorted(RUNS))
def test_likelihood_at_temperature_zero_and_nan(name, runs, twin):
    """temperature 0 and -0.0: lik is exactly 0, so every saved log-target lik + prior is the prior's own double (the twin's log-prior of
    the saved theta); temperature NaN: lik and the log-target are NaN from the start, nothing is ever accepted — what the twin gives"""
    d = runs["default"]
    chains = int(d[name + "/chains"])
    trows, tstate, prior = twin(name, chains)
    rows, state = d[name + "/rows"], d[name + "/state"]
    for q in (3, 5):
        assert TEMPS[q] == 0.0
        assert np.isfinite(prior[:, q]).all()
        assert _same_bits(rows[:, q, 3], prior[:, q]), (name, q)
        assert T % RUNS[name][3] == 0 and _same_bits(state[3, q], prior[-1, q])      # (the last iteration is a saved one)
    assert np.isnan(TEMPS[6])
    assert np.isnan(rows[:, 6, 3]).all() and np.isnan(trows[:, 6, 3]).all() and np.isnan(state[3, 6]).all()
    assert (rows[:, 6, :3] == np.array(THETA0)[None, :, None]).all() and (d[name + "/acceptance"][6] == 0.0).all()
