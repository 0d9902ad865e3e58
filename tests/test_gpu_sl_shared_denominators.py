"""The advance kernel's shared-denominator bodies on the GPU (-m gpu): synthetic pairs with every share mask of every entry-count
shape up to 5 uncensored x 4 censored entries (dose-0 entries and y == 0 / y == 100 entries at one dose among them), advanced plain
and as a work queue, models 1 and 2, moments on and off, against the scalar CPU twin bit for bit."""
import numpy as np
import pytest

from test_sl_shared_denominators import share_map, synthetic_pairs

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from pyhillfit_amd import _lib
    _lib.load()
    return "cuda:0"


@pytest.mark.parametrize("model,moments", [(2, False), (2, True), (1, False), (1, True)])
def test_every_share_mask_bit_identical_to_cpu_twin_plain_and_queued(model, moments, gpu):
    from oracle import c_oracle as co
    from pyhillfit_amd.doseresponse import PackedPoints
    from pyhillfit_amd.sampler import SingleLevelSampler, gamma_table
    cases = synthetic_pairs()
    packed = PackedPoints([(c, y) for _, c, y in cases])
    Q, chains, T, thin, adapt = len(cases), 1024, 480, 2, 60      # the second advance (419 iterations) is long enough to be queued
    for p, ((ko, kc, mask, _), _, _) in enumerate(cases):
        src = share_map(packed.ln_conc[p, :ko + kc], ko, kc)
        assert sum(1 << m for m, s in enumerate(src) if s >= 0) == mask
    theta0 = [5.0, 1.0, 9.0] if model == 2 else [5.0, 9.0]
    temps = [1.0 if q % 3 else 0.5 for q in range(Q)]
    got = []
    for quanta in (0, 4):
        s = SingleLevelSampler(packed, model, list(range(Q)), temps, chains, thinning=thin, seed=77, adapt_start=adapt, device=gpu,
                               queue_quanta=quanta)
        s.init(theta0, cov_identity=False, cov_scale=0.05)
        if moments:
            s.enable_moments(after_iteration=adapt)
        rows = np.concatenate([s.advance(k).cpu().numpy() for k in (adapt + 1, T - adapt - 1)])
        assert (s._queue is not None) == (quanta > 0)
        if quanta:
            s.check_queue()
        got.append((rows, s.state.cpu().numpy().reshape(s.S, Q, chains),
                    None if not moments else [t.cpu().numpy() for t in s.posterior_moments()[:2]]))
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
    if moments:
        assert all(np.array_equal(a, b) for a, b in zip(got[0][2], got[1][2]))
    chain, state = got[1][0], got[1][1]
    assert np.isfinite(chain).all()
    gam = gamma_table(T)
    rng = np.random.default_rng(model)
    for q, (_, concs, y) in enumerate(cases):
        pk = co.PackedPair(concs, y, model, temps[q])
        for c in (0, chains - 1, int(rng.integers(1, chains - 1))):
            st = pk.init_state(theta0, False, 0.05)
            rows = pk.advance(st, 0, T, thin, adapt, False, gam, seed=77, chain_id=c, problem_id=q)
            assert np.array_equal(chain[:, q, :, c], rows), (cases[q][0], c)
            assert np.array_equal(state[:, q, c], st), (cases[q][0], c)
