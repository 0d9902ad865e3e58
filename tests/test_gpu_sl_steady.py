"""The advance kernel's steady bodies (launches and quanta with t_begin >= adapt_start: no adapting compare, no gamma select, no reset
selects, 32-bit iteration bookkeeping, integer accept count) on the GPU (-m gpu), against the scalar CPU twin bit for bit: launches that
end before, straddle, start exactly at and lie after adapt_start, 64 and 65 chains per pair, a shared-denominator, a plain and a
run-time-loop shape, models 1 and 2, moments on and off, four temperatures on one pair, a queued launch whose quanta take different
paths, and PHF_SL_STEADY=0 against the default in fresh processes."""
import ctypes as C
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from conftest import REPO
from test_sl_shared_denominators import share_map

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

THIN, SEED = 5, 4242
# (concentrations, responses): 2 uncensored + 1 censored entry, the censored one at an uncensored entry's dose (share mask 0x1);
# 3 uncensored entries, nothing to share; 6 uncensored + 1 censored entries (no straight-line body: the run-time loops)
PAIRS = [(np.array([0.1, 0.1, 1.0]), np.array([0.0, 12.0, 45.0])),
         (np.array([0.1, 1.0, 10.0, 10.0]), np.array([15.0, 40.0, 77.0, 81.0])),
         (np.array([0.01, 0.03, 0.1, 0.3, 1.0, 3.0, 10.0]), np.array([0.0, 8.0, 20.0, 35.0, 52.0, 70.0, 88.0]))]
SHAPES = [(2, 1), (3, 0), (6, 1)]


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from pyhillfit_amd import _lib
    _lib.load()
    return "cuda:0"


@pytest.fixture(scope="module")
def packed():
    from pyhillfit_amd.doseresponse import PackedPoints
    p = PackedPoints(PAIRS)
    assert [(int(c[0]), int(c[1] + c[2])) for c in p.counts] == SHAPES
    assert share_map(p.ln_conc[0, :3], 2, 1) == [0]                       # pair 0 runs the shared-denominator body of its shape
    return p


def _theta0(model):
    return [5.0, 1.0, 9.0] if model == 2 else [5.0, 9.0]


def _check(packed, gpu, model, chains, launches, adapt, reset, moments, pair_index=(0, 1, 2), temps=(1.0, 1.0, 1.0)):
    """advance by `launches`, then compare rows, final state (acceptance count included) and moments with the twin"""
    from oracle import c_oracle as co
    from pyhillfit_amd.sampler import SingleLevelSampler, gamma_table
    Q, T = len(pair_index), sum(launches)
    s = SingleLevelSampler(packed, model, list(pair_index), list(temps), chains, thinning=THIN, seed=SEED, adapt_start=adapt,
                           reset_mean_at_adapt_start=reset, device=gpu)
    s.init(_theta0(model), cov_identity=False, cov_scale=0.05)
    after = THIN                                                            # the moments skip the first saved row
    if moments:
        s.enable_moments(after_iteration=after)
    chain = np.concatenate([s.advance(k).cpu().numpy() for k in launches])
    assert chain.shape == (T // THIN, Q, s.d + 1, chains)
    state = s.state.cpu().numpy().reshape(s.S, Q, chains)
    mom = None if not moments else s.moments.cpu().numpy().reshape(2 * (s.d + 1) + 1, Q, chains)
    gam = gamma_table(T)
    nacc_row = 2 * s.d + 2 + s.d * (s.d + 1) // 2
    for q in range(Q):
        concs, y = PAIRS[pair_index[q]]
        pk = co.PackedPair(concs, y, model, temps[q])
        for c in sorted({0, 1, 31, 63, chains - 1}):
            st = pk.init_state(_theta0(model), False, 0.05)
            rows = pk.advance(st, 0, T, THIN, adapt, reset, gam, seed=SEED, chain_id=c, problem_id=q)
            assert np.array_equal(chain[:, q, :, c], rows), (q, c)
            assert np.array_equal(state[:, q, c], st), (q, c)
            assert state[nacc_row, q, c] == st[nacc_row] and 0 <= st[nacc_row] <= T and st[nacc_row] == int(st[nacc_row])
            if moments:
                # the kernel's accumulators replayed exactly: sum x and sum of the untempered log-likelihood are plain sums in save
                # order, sum x^2 is the chain m2 = fma(x, x, m2) — one rounding of the exact x^2 + m2 (Fraction arithmetic is exact
                # and float() of a Fraction rounds to nearest even).  The log-likelihood of every saved row is the last word of the
                # twin's state there, so a second twin chain is advanced one thinning period at a time.
                st2 = pk.init_state(_theta0(model), False, 0.05)
                m1, m2, mll = np.zeros(s.d + 1), [0.0] * (s.d + 1), 0.0
                for k in range(T // THIN):
                    r = pk.advance(st2, k * THIN, (k + 1) * THIN, THIN, adapt, reset, gam, seed=SEED, chain_id=c, problem_id=q)[0]
                    assert np.array_equal(r, rows[k]), (q, c, k)
                    if (k + 1) * THIN > after:
                        m1 = m1 + r
                        m2 = [float(Fraction(float(x)) * Fraction(float(x)) + Fraction(m)) for x, m in zip(r, m2)]
                        mll = mll + st2[-1]
                assert np.array_equal(st2, st), (q, c)
                assert np.array_equal(mom[:, q, c], np.concatenate([m1, m2, [mll]])), (q, c)
    return chain, state


@pytest.mark.parametrize("moments", [False, True])
@pytest.mark.parametrize("chains", [64, 65])
@pytest.mark.parametrize("model", [2, 1])
def test_launches_before_across_and_after_adapt_start(model, chains, moments, gpu, packed):
    """0->7 before adapt_start = 10, 7->13 across it, 13->14 one steady iteration, 14->40 steady"""
    _check(packed, gpu, model, chains, (7, 6, 1, 26), 10, False, moments)


@pytest.mark.parametrize("moments", [False, True])
@pytest.mark.parametrize("reset", [False, True])
@pytest.mark.parametrize("chains", [64, 65])
@pytest.mark.parametrize("model", [2, 1])
def test_steady_launch_starts_exactly_at_adapt_start(model, chains, reset, moments, gpu, packed):
    """0->10, 10->15: the reset of the mean (when on) fires in the last iteration of the general path, the first adapting iteration
    is the first of a steady launch"""
    _check(packed, gpu, model, chains, (10, 5), 10, reset, moments)


@pytest.mark.parametrize("model", [2, 1])
def test_temperatures_of_one_launch_take_their_own_paths(model, gpu, packed):
    temps = (1.0, 0.5, (1.0 / 40.0) ** 3, 0.0)
    _check(packed, gpu, model, 65, (7, 6, 1, 26), 10, True, False, pair_index=(0, 0, 0, 0), temps=temps)


def test_queued_launch_with_general_straddling_and_steady_quanta(gpu, packed):
    """15 iterations in quanta of 5 with adapt_start = 7: the first quantum lies before it, the second straddles it (both the general
    path), the third is steady; just over 2 x phf_simd_count() blocks, so that the library does queue the launch"""
    from oracle import c_oracle as co
    from pyhillfit_amd import _lib
    from pyhillfit_amd.sampler import SingleLevelSampler, _ptr, _stream_ptr, gamma_table
    model, T, quantum, adapt = 2, 15, 5, 7
    slots = 2 * int(_lib.load().phf_simd_count())
    bpp = slots // 3 + 1
    chains = 64 * bpp - 63                                                   # a ragged last block per pair
    s = SingleLevelSampler(packed, model, [0, 1, 2], [1.0, 1.0, 1.0], chains, thinning=THIN, seed=SEED, adapt_start=adapt, device=gpu,
                           queue_quanta=0)
    assert slots < s.nblocks <= 16 * slots
    s.init(_theta0(model), cov_identity=False, cov_scale=0.05)
    cfg = s._config(T)
    rows = torch.empty((T // THIN, 3, s.d + 1, chains), dtype=torch.float64, device=gpu)
    queue = torch.zeros(2 + s.nblocks, dtype=torch.int32, device=gpu)
    _lib.check(s.lib.phf_single_level_advance_queued(C.byref(s.points.struct), C.byref(s.prob), C.byref(cfg), 0, T, _ptr(s.state),
                                                     _ptr(rows), None, 0, quantum, _ptr(queue), _stream_ptr(s.device)),
               "phf_single_level_advance_queued")
    torch.cuda.synchronize()
    qw = queue.cpu().numpy()
    assert qw[-1] == 0 and qw[0] >= 3 * s.nblocks and (qw[1:1 + s.nblocks] == 3).all()      # it ran as a queue of three quanta per block
    chain = rows.cpu().numpy()
    state = s.state.cpu().numpy().reshape(s.S, 3, chains)
    gam = gamma_table(T)
    for q in range(3):
        pk = co.PackedPair(*PAIRS[q], model, 1.0)
        for c in (0, 63, 64, chains - 1):
            st = pk.init_state(_theta0(model), False, 0.05)
            want = pk.advance(st, 0, T, THIN, adapt, False, gam, seed=SEED, chain_id=c, problem_id=q)
            assert np.array_equal(chain[:, q, :, c], want), (q, c)
            assert np.array_equal(state[:, q, c], st), (q, c)


CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from test_gpu_sl_steady import PAIRS, SEED, THIN, _theta0
from pyhillfit_amd.doseresponse import PackedPoints
from pyhillfit_amd.sampler import SingleLevelSampler
s = SingleLevelSampler(PackedPoints(PAIRS), 2, [0, 1, 2], [1.0, 0.5, 1.0], 65, thinning=THIN, seed=SEED, adapt_start=10,
                       reset_mean_at_adapt_start=True, device="cuda:0")
s.init(_theta0(2), cov_identity=False, cov_scale=0.05)
rows = np.concatenate([s.advance(k).cpu().numpy() for k in (7, 6, 1, 26)])
np.concatenate([rows.ravel(), s.state.cpu().numpy().ravel()]).tofile(sys.argv[2])
"""


def test_switch_off_in_the_environment_gives_the_same_bytes(gpu, tmp_path):
    """PHF_SL_STEADY=0 (read once per process, so two fresh processes): every launch on the general path; same rows and state"""
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    out = {}
    for name, value in (("default", None), ("off", "0")):
        env = {k: v for k, v in os.environ.items() if k != "PHF_SL_STEADY"}
        if value is not None:
            env["PHF_SL_STEADY"] = value
        out[name] = tmp_path / (name + ".bin")
        subprocess.run([sys.executable, str(script), REPO, str(out[name])], env=env, check=True, timeout=300)
    a, b = out["default"].read_bytes(), out["off"].read_bytes()
    assert len(a) == 8 * (8 * 3 * 4 * 65 + 16 * 3 * 65) and a == b
