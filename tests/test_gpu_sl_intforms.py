"""The device's three-input bit forms of round 10 (phf_math.h: the mantissa's re-bias in phf_normal_u32 and phf_log_ndtr_tab, the normal's
sign transfer) on the GPU (-m gpu), with the functions next to them that round 10 tried other forms of and left as they were:
  - phf_debug_math functions 17 (phf_normal_u32), 10 (phf_log_fast), 18 (phf_log_ndtr_tab) and 9 (phf_exp_fast) on the edge sets of
    tests/test_sl_intforms_host.py plus 2^20 random arguments each, bit for bit against the host build (the twin);
  - chains against the twin, bit for bit — rows, final state with accept count and untempered log-likelihood, moments — on the six pairs of
    tests/test_gpu_sl_lean.py, models 1 and 2, 64 and 65 chains, launches (7, 6, 1, 286) around adapt_start = 10, temperatures 1, 0.5, 0;
    and one queued launch with a ragged last block;
  - one short hierarchical hipcc launch (Ne = 3, 64 chains) and one posterior-predictive call against their twins: they draw through the
    same phf_normal_u32."""
import numpy as np
import pytest

import test_gpu_sl_lean as lean
from test_sl_intforms_host import log_edge_args, log_random_args, logphi_y_args, normal_edge_words

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N_RANDOM = 1 << 20


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
    return PackedPoints(lean.PAIRS)


def _same_bits_nan_as_nan(got, want):
    """bit for bit, a zero's sign included; a NaN compares as "is NaN" (its payload and sign are the hardware's)"""
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64))


def test_normal_of_a_word(gpu):
    from oracle import c_oracle as co
    from pyhillfit_amd.sampler import debug_math
    w = np.concatenate([normal_edge_words().astype(np.uint64), np.random.default_rng(41).integers(0, 2 ** 32, N_RANDOM, dtype=np.uint64)])
    got, want = debug_math(17, w.astype(np.float64), gpu), co.normal_u32(w.astype(np.uint32))
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), [hex(int(v)) for v in w[got.view(np.uint64) != want.view(np.uint64)][:8]]


def test_logarithm(gpu):
    from oracle import c_oracle as co
    from pyhillfit_amd.sampler import debug_math
    x = np.concatenate([log_edge_args(), log_random_args(N_RANDOM, seed=43), [0.0, -0.0, 5e-324, 1e-310, -1.0, -0.5, -1e300]])
    got, want = debug_math(10, x, gpu), co.vec("log_fast", x)
    assert _same_bits_nan_as_nan(got, want), [float(v).hex() for v in x[got.view(np.uint64) != want.view(np.uint64)][:8]]


def test_log_phi_from_the_table(gpu):
    from oracle import c_oracle as co
    from pyhillfit_amd.sampler import debug_math
    rng = np.random.default_rng(47)
    sqrt2 = float(np.sqrt(2.0))
    y = logphi_y_args()
    # fn 18 takes x and forms y = -x / sqrt 2 itself: the grid's y, restated as x, and random x over the table's range and beyond
    with np.errstate(over="ignore"):
        x_grid = -y * sqrt2
    x = np.concatenate([x_grid, -np.exp(rng.uniform(-30, 12.2, N_RANDOM // 2)), rng.uniform(-40, 0, N_RANDOM // 2),
                        [0.0, -0.0, -1.85e5, -2e5, 3.0, 1e5, np.inf, -np.inf, np.nan]])
    got, want = debug_math(18, x, gpu), co.vec("log_ndtr_tab", x)
    assert _same_bits_nan_as_nan(got, want), [float(v).hex() for v in x[~((got.view(np.uint64) == want.view(np.uint64)) | np.isnan(want))][:8]]


def test_exponential(gpu):
    from oracle import c_oracle as co
    from pyhillfit_amd.sampler import debug_math
    rng = np.random.default_rng(53)
    x = np.concatenate([rng.uniform(-760, 720, N_RANDOM // 2), rng.uniform(-3, 3, N_RANDOM // 2), np.arange(-64, 65) * float(np.log(2.0)) / 64.0,
                        [0.0, -0.0, 709.782712893384, 710.0, -745.13, -746.0, 1e-300, -1e-300, np.inf, -np.inf, np.nan]])
    got, want = debug_math(9, x, gpu), co.vec("exp_fast", x)
    assert _same_bits_nan_as_nan(got, want), [float(v).hex() for v in x[~((got.view(np.uint64) == want.view(np.uint64)) | np.isnan(want))][:8]]


@pytest.mark.parametrize("chains", [64, 65])
@pytest.mark.parametrize("model", [2, 1])
def test_chains_of_the_six_pairs_at_three_temperatures(model, chains, gpu, packed):
    """every pair of tests/test_gpu_sl_lean.py (shared and plain straight-line bodies, the run-time loops, dose 0, dose 1e-30) at temperatures
    1, 0.5 and 0 in one sampler; 0 -> 7 before adapt_start = 10, 7 -> 13 across it, 13 -> 14 one steady iteration, 14 -> 300 steady; rows,
    state, accept count, ll1 and moments of six lanes per problem against the twin"""
    pairs = list(range(len(lean.PAIRS))) * 3
    temps = [1.0] * 6 + [0.5] * 6 + [0.0] * 6
    acc = lean._check(packed, gpu, model, chains, (7, 6, 1, 286), 10, pairs, temps=temps, moments=True, reset=True)
    assert (acc > 0.0).all() and (acc < 1.0).all(), acc


def test_queued_launch_with_a_ragged_last_block(gpu, packed):
    lean.test_queued_launch_with_steady_quanta(gpu, packed)


def test_hierarchical_hipcc_launch_draws_the_same_normals(gpu):
    """Ne = 3 with point counts no hand-allocated kernel exists for: a hipcc kernel, whose normals are phf_normal_u32's"""
    from oracle import c_oracle as co
    from pyhillfit_amd import hierarchical as H
    from pyhillfit_amd.sampler import gamma_table
    from test_gpu_waic import synthetic_pair
    rng = np.random.default_rng(59)
    expts, (pic50, hill, sigma) = synthetic_pair(rng, [4, 3, 2])
    theta0 = np.concatenate([[1.1, 4.5, pic50 + 0.1, 0.3], np.tile([pic50 - 0.1, 1.1 * hill], 3), [1.2 * sigma]])
    T, thin, adapt, seed, C = 120, 5, 40, 61, 64
    s = H.HierarchicalSampler(H.PackedHierPoints([expts]), [0], C, thinning=thin, seed=seed, adapt_start=adapt, device=gpu)
    s.set_kernel_hint(isa=False)
    s.init(theta0, cov_scale=0.01)
    chain = np.concatenate([s.advance(k).cpu().numpy() for k in (37, 83)])
    assert H.last_kernel() in (1, 2)                                       # a hipcc kernel, one or two lanes per chain
    state = s.state.cpu().numpy().reshape(s.S, 1, C)
    shapes, scales, locs = H.prior_params()
    pk = co.PackedHierPair(expts, shapes, scales, locs)
    gam = gamma_table(T)
    for c in (0, 31, 63):
        st = pk.init_state(theta0, 0.01)
        rows = pk.advance(st, 0, T, thin, adapt, gam, seed=seed, chain_id=c, problem_id=0)
        assert np.array_equal(chain[:, 0, :, c].view(np.uint64), np.ascontiguousarray(rows).view(np.uint64)), c
        assert np.array_equal(state[:, 0, c].view(np.uint64), np.ascontiguousarray(st).view(np.uint64)), c


def test_posterior_predictive_call_draws_the_same_normals(gpu):
    """single-level replicates y_rep = clamp(pred + sigma phf_normal_u32(word), 0, 100) against the restatement of tests/test_gpu_ppc.py
    (the twin's phf_normal_u32 of the twin's Philox words; its tolerance, 1e-9, is for the prediction restated in numpy)"""
    import test_gpu_ppc as tp
    from pyhillfit_amd import ppc as pp
    from test_gpu_waic import synthetic_points
    rng = np.random.default_rng(67)
    pts = synthetic_points(rng, [5, 9, 4])
    pi = np.repeat(np.arange(pts.num_problems), 4)
    m = len(pi)
    theta = tp._theta(rng, 2, m)
    ctr = np.column_stack([rng.integers(0, 5000, m), rng.integers(0, 2 ** 32, m), rng.integers(0, 2 ** 32, m)])
    seed = 25 + (1 << 40)
    y_rep, _ = pp.replicate(pts, 2, pi, theta, ctr, seed, gpu)
    for i in range(m):
        q, n = pi[i], pts.count[pi[i]]
        pred, sigma = tp.predictions(pts, 2, q, theta[i])
        want = tp.restated_y_rep(2, pred, sigma, tp.words(ctr[i], n, seed))
        np.testing.assert_allclose(y_rep[i, :n], want, rtol=0, atol=1e-9)
