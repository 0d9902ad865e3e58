"""The single-level sampler's accept test for d = 3 on the device (phf_mh_accept_u32, pyhillfit_amd/csrc/phf_model.h, through
phf_debug_math fn 22): it must give phf_log_pos_k((w + 1/2) / 2^32) < x for every pair tried — signed zeros, infinities, NaN, x next
to 0 and next to ln u_0, x equal to the logarithm of a word, random x — with every word around the threshold T = 2^32 e^x - 1/2 and
around both edges of the band in which the logarithm is evaluated (2^18 words either side of the fp32 estimate of T), a stride through
four band-widths, and random words.  Chains stay bit-identical to the twin only if this holds for every (x, w) an iteration can meet."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BAND = 2 ** 18
W_MAX = 2 ** 32 - 1


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return "cuda:0"


def _check(xs, ws, gpu):
    """xs, ws: equal-length arrays of pairs; returns how many pairs were checked"""
    from pyhillfit_amd.sampler import debug_math
    inp = np.empty(2 * len(xs))
    inp[0::2], inp[1::2] = xs, ws
    out = debug_math(22, inp, gpu)
    fast, exact = out[0::2], out[1::2]
    assert set(np.unique(out)) <= {0.0, 1.0}
    bad = np.flatnonzero(fast != exact)
    assert bad.size == 0, [(float(xs[i]), int(ws[i]), float(fast[i]), float(exact[i])) for i in bad[:8]]
    return len(xs)


def _words_around(x, rng):
    t = np.ldexp(np.exp(min(x, 1.0)), 32) - 0.5 if np.isfinite(x) else (0.0 if x < 0 else 2.0 ** 33)
    t = float(np.clip(t, -2.0 ** 20, 2.0 ** 33))
    parts = [np.arange(-2 ** 12, 2 ** 12) + np.floor(t),                                   # the threshold itself
             np.arange(-2 ** 15, 2 ** 15) + np.floor(t - BAND), np.arange(-2 ** 15, 2 ** 15) + np.floor(t + BAND),   # the band's edges
             np.arange(-4 * BAND, 4 * BAND, 97) + np.floor(t),                             # four band-widths either side
             rng.integers(0, 2 ** 32, 2048).astype(np.float64), np.array([0.0, 1.0, 2.0, W_MAX - 1, W_MAX])]
    w = np.unique(np.clip(np.concatenate(parts), 0, W_MAX))
    return w


def test_accept_u32_equals_the_logarithm_comparison(gpu):
    from pyhillfit_amd.sampler import debug_math
    rng = np.random.default_rng(20261016)
    ln_u0 = float(np.log(0.5 * 2.0 ** -32))
    ln_umax = float(np.log1p(-0.5 * 2.0 ** -32))
    near = [0.0, 1e-300, 1e-12, 2.0 ** -20, 1e-6, 1e-4, 1e-2]
    xs = [0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 1.0, 100.0, 1e300, -100.0, -1e300, ln_umax, ln_umax * (1 + 1e-9), ln_umax * (1 - 1e-9)]
    xs += [s * d for d in near for s in (1.0, -1.0)]
    xs += [ln_u0 + d for d in (0.0, 1e-15, -1e-15, 1e-12, -1e-12, 1e-9, -1e-9, 1e-6, -1e-6, 1e-3, -1e-3, 0.5, -0.5)]
    xs += [float(np.log(1.5 * 2.0 ** -32)), float(np.log(2.5 * 2.0 ** -32))]
    # x equal to the device logarithm of a word (ties: that word must reject, its neighbours decide by the logarithm)
    tie_w = np.concatenate([rng.integers(0, 2 ** 32, 24), [0, 1, 2, 2 ** 31, W_MAX]]).astype(np.float64)
    tie_x = debug_math(10, (tie_w + 0.5) * 2.0 ** -32, gpu)
    xs += list(tie_x)
    xs += list(rng.uniform(-25.0, 0.5, 80)) + list(-10.0 ** rng.uniform(-12, 1.4, 40))
    checked = 0
    batch_x, batch_w = [], []
    for x in xs:
        w = _words_around(float(x), rng)
        batch_x.append(np.full(len(w), x))
        batch_w.append(w)
        if sum(map(len, batch_w)) > 4_000_000:
            checked += _check(np.concatenate(batch_x), np.concatenate(batch_w), gpu)
            batch_x, batch_w = [], []
    checked += _check(np.concatenate(batch_x), np.concatenate(batch_w), gpu)
    assert checked > 20_000_000
    # many random x with random words and the words next to each threshold
    x = np.concatenate([rng.uniform(-26.0, 1.0, 40000), -10.0 ** rng.uniform(-14, 1.4, 20000)])
    t = np.floor(np.ldexp(np.exp(x), 32))
    off = np.concatenate([rng.integers(0, 2 ** 32, (len(x), 32)) - t[:, None], rng.integers(-64, 64, (len(x), 32)),
                          rng.integers(-BAND - 2 ** 14, -BAND + 2 ** 14, (len(x), 16)), rng.integers(BAND - 2 ** 14, BAND + 2 ** 14, (len(x), 16))], axis=1)
    w = np.clip(t[:, None] + off, 0, W_MAX)
    _check(np.repeat(x, w.shape[1]), w.ravel(), gpu)
