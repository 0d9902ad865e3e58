"""The steady bodies without their dead guards (proposals outside the prior's support rejected by predicate, no lower clamp on the Hill
exponentials of pairs whose doses bound their arguments, Cholesky pivot selects only when some lane of the wavefront has a non-positive pivot, accepts counted under the accepting
lanes' mask) on the GPU (-m gpu) against the scalar CPU twin, bit for bit: rows, final state with accept count and untempered
log-likelihood, moments.  Besides ordinary runs: starts on every bound of the support with a unit proposal covariance (about half the
first proposals fall outside), starts outside it (log-target -inf), a zero covariance (every pivot non-positive on every iteration), a
zero pivot in half the lanes of a wavefront only, pairs with a dose of 0 and of 1e-30, and PHF_SL_STEADY=0 against the default."""
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

THIN, SEED = 5, 977
# 2 uncensored + 1 censored entry at an uncensored entry's dose (share mask 0x1); 3 uncensored; 4 uncensored + 1 censored, shared; 6
# uncensored + 1 censored (no straight-line body: the run-time loops); a pair with dose 0 (ln_conc = -inf, its censored entry sharing that
# entry's denominator); a pair with dose 1e-30 (ln_conc = -69.1)
PAIRS = [(np.array([0.1, 0.1, 1.0]), np.array([0.0, 12.0, 45.0])),
         (np.array([0.1, 1.0, 10.0, 10.0]), np.array([15.0, 40.0, 77.0, 81.0])),
         (np.array([0.1, 0.1, 1.0, 10.0, 100.0]), np.array([0.0, 6.0, 31.0, 72.0, 94.0])),
         (np.array([0.01, 0.03, 0.1, 0.3, 1.0, 3.0, 10.0]), np.array([0.0, 8.0, 20.0, 35.0, 52.0, 70.0, 88.0])),
         (np.array([0.0, 0.0, 0.1, 1.0, 10.0]), np.array([0.0, 3.0, 11.0, 48.0, 90.0])),
         (np.array([1e-30, 0.1, 1.0]), np.array([2.0, 21.0, 63.0]))]
SHAPES = [(2, 1), (3, 0), (4, 1), (6, 1), (4, 1), (3, 0)]


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
    for q in (0, 2, 4):
        assert share_map(p.ln_conc[q, :sum(SHAPES[q])], *SHAPES[q]) == [0]     # these run the shared-denominator body of their shape
    assert np.isneginf(p.ln_conc[4, 0]) and p.ln_conc[5, 0] < -50.0
    return p


def _theta0(model):
    return [5.0, 1.0, 9.0] if model == 2 else [5.0, 9.0]


def _same_bits(a, b):
    """equal as bit patterns (a log-target of -inf or a NaN must be reproduced, not merely compare equal)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _check(packed, gpu, model, chains, launches, adapt, pair_index, temps=None, moments=False, reset=False, theta0=None,
           cov_identity=False, cov_scale=0.05, lanes=None):
    """advance by `launches`, then compare rows, final state (accept count and ll1 included) and moments with the twin.
    theta0: None (the usual start), or a function (q, c) -> theta.  Returns the per-problem mean acceptance of the checked chains."""
    from oracle import c_oracle as co
    from pyhillfit_amd.sampler import SingleLevelSampler, gamma_table
    Q, T = len(pair_index), sum(launches)
    temps = [1.0] * Q if temps is None else list(temps)
    start = (lambda q, c: _theta0(model)) if theta0 is None else theta0
    s = SingleLevelSampler(packed, model, list(pair_index), temps, chains, thinning=THIN, seed=SEED, adapt_start=adapt,
                           reset_mean_at_adapt_start=reset, device=gpu)
    s.init(np.array([[start(q, c) for c in range(chains)] for q in range(Q)]), cov_identity=cov_identity, cov_scale=cov_scale)
    after = THIN
    if moments:
        s.enable_moments(after_iteration=after)
    chain = np.concatenate([s.advance(k).cpu().numpy() for k in launches])
    assert chain.shape == (T // THIN, Q, s.d + 1, chains)
    state = s.state.cpu().numpy().reshape(s.S, Q, chains)
    mom = None if not moments else s.moments.cpu().numpy().reshape(2 * (s.d + 1) + 1, Q, chains)
    gam = gamma_table(T)
    nacc_row = 2 * s.d + 2 + s.d * (s.d + 1) // 2
    acceptance = np.zeros(Q)
    lanes = sorted({0, 1, 31, 32, 63, chains - 1}) if lanes is None else lanes
    for q in range(Q):
        concs, y = PAIRS[pair_index[q]]
        pk = co.PackedPair(concs, y, model, temps[q])
        for c in lanes:
            st = pk.init_state(start(q, c), cov_identity, cov_scale)
            rows = pk.advance(st, 0, T, THIN, adapt, reset, gam, seed=SEED, chain_id=c, problem_id=q)
            assert _same_bits(chain[:, q, :, c], rows), (q, c)
            assert _same_bits(state[:, q, c], st), (q, c)
            assert 0 <= st[nacc_row] <= T and st[nacc_row] == int(st[nacc_row])
            acceptance[q] += st[nacc_row]                                    # (integers: the sum is exact)
            if moments:
                # the accumulators replayed exactly (as tests/test_gpu_sl_steady.py does): plain sums in save order, sum x^2 one rounding of
                # the exact x^2 + m2 per step; the untempered log-likelihood of a saved row is the last word of the twin's state there
                st2 = pk.init_state(start(q, c), cov_identity, cov_scale)
                m1, m2, mll = np.zeros(s.d + 1), [0.0] * (s.d + 1), 0.0
                for k in range(T // THIN):
                    r = pk.advance(st2, k * THIN, (k + 1) * THIN, THIN, adapt, reset, gam, seed=SEED, chain_id=c, problem_id=q)[0]
                    if (k + 1) * THIN > after:
                        m1 = m1 + r
                        m2 = [float(Fraction(float(x)) * Fraction(float(x)) + Fraction(m)) for x, m in zip(r, m2)]
                        mll = mll + st2[-1]
                assert _same_bits(st2, st), (q, c)
                assert _same_bits(mom[:, q, c], np.concatenate([m1, m2, [mll]])), (q, c)
    return acceptance / (T * len(lanes))


@pytest.mark.parametrize("moments", [False, True])
@pytest.mark.parametrize("chains", [64, 65])
@pytest.mark.parametrize("model", [2, 1])
@pytest.mark.parametrize("pairs", [(0, 1, 2), (3,)])
def test_launches_before_across_and_after_adapt_start(pairs, model, chains, moments, gpu, packed):
    """0->7 before adapt_start = 10, 7->13 across it, 13->14 one steady iteration, 14->300 steady; shapes (2, 1) shared, (3, 0),
    (4, 1) shared, and (6, 1) for the run-time loops"""
    acc = _check(packed, gpu, model, chains, (7, 6, 1, 286), 10, pairs, moments=moments, reset=True)
    assert (acc > 0.02).all() and (acc < 0.98).all()


@pytest.mark.parametrize("model", [2, 1])
def test_temperatures_one_half_and_zero_on_one_pair_in_one_launch(model, gpu, packed):
    _check(packed, gpu, model, 65, (7, 6, 1, 186), 10, (2, 2, 2), temps=(1.0, 0.5, 0.0))
    _check(packed, gpu, model, 64, (10, 90), 10, (3, 3, 3), temps=(0.0, 1.0, 0.5))


def test_queued_launch_with_steady_quanta(gpu, packed):
    """30 iterations in quanta of 5 with adapt_start = 7: the first quantum lies before it, the second straddles it, the other four are
    steady; just over 2 x phf_simd_count() blocks, so that the library does queue the launch"""
    from oracle import c_oracle as co
    from pyhillfit_amd import _lib
    from pyhillfit_amd.sampler import SingleLevelSampler, _ptr, _stream_ptr, gamma_table
    model, T, quantum, adapt, pairs = 2, 30, 5, 7, (0, 2, 3)
    slots = 2 * int(_lib.load().phf_simd_count())
    bpp = slots // 3 + 1
    chains = 64 * bpp - 63                                                   # a ragged last block per pair
    s = SingleLevelSampler(packed, model, list(pairs), [1.0, 1.0, 0.5], chains, thinning=THIN, seed=SEED, adapt_start=adapt, device=gpu,
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
    assert qw[-1] == 0 and qw[0] >= 6 * s.nblocks and (qw[1:1 + s.nblocks] == 6).all()      # it ran as a queue of six quanta per block
    chain = rows.cpu().numpy()
    state = s.state.cpu().numpy().reshape(s.S, 3, chains)
    gam = gamma_table(T)
    for q in range(3):
        pk = co.PackedPair(*PAIRS[pairs[q]], model, [1.0, 1.0, 0.5][q])
        for c in (0, 63, 64, chains - 1):
            st = pk.init_state(_theta0(model), False, 0.05)
            want = pk.advance(st, 0, T, THIN, adapt, False, gam, seed=SEED, chain_id=c, problem_id=q)
            assert _same_bits(chain[:, q, :, c], want), (q, c)
            assert _same_bits(state[:, q, c], st), (q, c)


ON_BOUNDS = {2: [[-3.0, 1.0, 9.0], [5.0, 0.0, 9.0], [5.0, 10.0, 9.0], [5.0, 1.0, 1e-3]],
             1: [[-3.0, 9.0], [5.0, 1e-3]]}


@pytest.mark.parametrize("temp", [1.0, 0.5])
@pytest.mark.parametrize("model", [2, 1])
def test_many_proposals_outside_the_support(model, temp, gpu, packed):
    """one problem per bound, every chain started ON it (sigma = 1e-3 is itself outside: that problem starts at -inf) with the identity
    as proposal covariance: about half the proposals of the first iterations fall outside.  All iterations steady (adapt_start = 0)."""
    starts = ON_BOUNDS[model]
    acc = _check(packed, gpu, model, 65, (5, 195), 0, (2,) * len(starts), temps=[temp] * len(starts), moments=True,
                 theta0=lambda q, c: starts[q], cov_identity=True, cov_scale=1.0)
    assert (acc > 0.0).all() and (acc < 1.0).all(), acc                      # both outcomes occurred


@pytest.mark.parametrize("model", [2, 1])
def test_starts_outside_the_support(model, gpu, packed):
    """Hill = -1 and sigma = 5e-4: the log-target starts at -inf, and stays there for as long as the chain has not stepped inside"""
    starts = [[5.0, -1.0, 9.0], [5.0, 1.0, 5e-4]] if model == 2 else [[5.0, 5e-4], [-4.0, 9.0]]
    for identity, scale in ((True, 1.0), (False, 0.05)):
        acc = _check(packed, gpu, model, 65, (5, 145), 0, (2, 0), theta0=lambda q, c: starts[q], cov_identity=identity, cov_scale=scale)
        if identity:
            assert (acc > 0.0).all() and (acc < 1.0).all(), acc


@pytest.mark.parametrize("model", [2, 1])
def test_zero_covariance_every_pivot_non_positive(model, gpu, packed):
    """cov_scale = 0 from a start whose coordinates are powers of two: the running mean gamma theta + (1 - gamma) mean reproduces theta
    exactly, so the covariance stays zero — every pivot of every lane non-positive on every iteration — the proposal is the state itself
    and is always accepted"""
    from pyhillfit_amd.sampler import SingleLevelSampler
    start = [4.0, 1.0, 8.0] if model == 2 else [4.0, 8.0]
    acc = _check(packed, gpu, model, 65, (5, 95), 0, (2, 3), temps=(1.0, 0.5), moments=True, theta0=lambda q, c: start, cov_scale=0.0)
    assert (acc == 1.0).all()
    s = SingleLevelSampler(packed, model, [2], [1.0], 64, thinning=THIN, seed=SEED, adapt_start=0, device=gpu)
    s.init(start, cov_identity=False, cov_scale=0.0)
    s.advance(100)
    d = s.d
    cov = s.state[2 * d + 1:2 * d + 1 + d * (d + 1) // 2].cpu().numpy()
    assert (cov == 0.0).all() and (s.acceptance().cpu().numpy() == 1.0).all()


def test_zero_pivot_in_half_the_lanes_of_a_wavefront(gpu, packed):
    """per-chain starts: the odd lanes have Hill = 0, so their initial covariance 0.05 |theta| has a zero pivot the even lanes' has not"""
    start = lambda q, c: [5.0, 0.0, 9.0] if c % 2 else [5.0, 1.0, 9.0]
    _check(packed, gpu, 2, 65, (5, 145), 0, (2, 1, 3), theta0=start, lanes=[0, 1, 2, 31, 32, 63, 64])
    _check(packed, gpu, 2, 64, (7, 6, 87), 10, (2,), theta0=start, lanes=[0, 1, 62, 63])


@pytest.mark.parametrize("model", [2, 1])
def test_pairs_with_dose_zero_and_dose_1e_minus_30(model, gpu, packed):
    acc = _check(packed, gpu, model, 65, (7, 6, 1, 186), 10, (4, 5, 2), temps=(1.0, 1.0, 0.5), moments=True)
    assert (acc > 0.0).all()


CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from test_gpu_sl_lean import ON_BOUNDS, PAIRS, SEED, THIN
from pyhillfit_amd.doseresponse import PackedPoints
from pyhillfit_amd.sampler import SingleLevelSampler
out = []
for pairs, temps, theta0, identity, scale in (((0, 2, 3), [1.0, 0.5, 1.0], [5.0, 1.0, 9.0], False, 0.05),
                                              ((2, 2, 2, 2), [1.0, 1.0, 0.0, 1.0], ON_BOUNDS[2], True, 1.0),
                                              ((4, 5, 1), [1.0, 1.0, 1.0], [5.0, 0.0, 9.0], False, 0.0)):
    s = SingleLevelSampler(PackedPoints(PAIRS), 2, list(pairs), temps, 65, thinning=THIN, seed=SEED, adapt_start=10,
                           reset_mean_at_adapt_start=True, device="cuda:0")
    s.init(theta0, cov_identity=identity, cov_scale=scale)
    out += [s.advance(k).cpu().numpy().ravel() for k in (7, 6, 1, 186)] + [s.state.cpu().numpy().ravel()]
np.concatenate(out).tofile(sys.argv[2])
"""


def test_switch_off_in_the_environment_gives_the_same_bytes(gpu, tmp_path):
    """PHF_SL_STEADY=0 (read once per process, so two fresh processes): every launch on the fully guarded general path; same rows and state"""
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
    assert len(a) == 8 * 65 * (40 * 4 + 16) * (3 + 4 + 3) and a == b
