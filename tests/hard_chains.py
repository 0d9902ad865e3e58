"""Hard chains for the streaming accumulators, an exact reference of what their reduces return and the a-priori error bounds
(shared by tests/test_hard_chains_host.py and tests/test_gpu_hard_chains.py; not a test module).

Rows are the samplers' layout [rows][Q][stride][C], stride = columns + 1, the unread last column NaN.  One FAMILY per column
(columns_of): offset, outlying start, drift, constant, and plant() puts one non-finite value into a copy of the rows.

The reference.  A double is a dyadic rational, so x - x0 and every sum of products the kernels form are evaluated EXACTLY here in
Python integers (all values of a half-chain scaled by one power of two) and fractions.Fraction, and rounded once at the end.  The
log-sum-exp quantities use mpmath at 120 digits.  numpy double or longdouble appear nowhere in the reference values.

The bounds.  u = 2^-53, gamma(n) = n u / (1 - n u): a recursively accumulated sum of n terms t_i carries |error| <= gamma(n) sum |t_i|
(Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 3.1; an fma chain of n products counts n).  Every bound
below is gamma(count of the roundings on the path) times the sum of the ABSOLUTE values of the terms that were added, the magnitudes
taken from the exact reference, never from the code under test; SLACK = 4 covers the dropped second-order terms and is the only
slack.  Notation for a half-chain of h rows: y_m = x_m - x0 (one rounding each), a = sum |y_m| / h.

diagnostics (phf_diagnostics.hip), half-chain i, lag k, n_k = h - k products:
    Q_k     fma chain of n_k products of two rounded y:                    gamma(n_k + 2) sum |y_m y_(m-k)|
    S       h additions of rounded y:                                      gamma(h + 1) sum |y|;   ybar = S / h: gamma(h + 2) a
    A_k + B_k = (S - last_k) + (S - first_k), last and first sums of k rounded y:  gamma(h + 4) AB_k,
            AB_k = 2 sum |y| + sum_(first k) |y| + sum_(last k) |y|
    h acov(k) = Q_k - ybar (A_k + B_k) + (h - k) ybar^2, three more roundings, then / h:
    |error of acov(k)| <= [gamma(h + 5) sum |y_m y_(m-k)| + gamma(2 h + 11) a AB_k + gamma(2 h + 9) (h - k) a^2] / h
  The shorter form one is tempted to write, gamma(h + 4) (sum |y y| + |ybar| (|A_k| + |B_k|) + (h - k) ybar^2) / h, is reported
  beside it (`acov_bound_short`) but is NOT a bound (the MI355X exceeds 4 x it by 5.85 on the offset family, 65 chains x 37 rows): the computed ybar, A_k and B_k carry absolute errors proportional to
  sum |y|, not to their own size, which cancels (A_(h-1) = y_0 = 0 exactly, its computed value is a rounding residue of S), and the
  product of two computed sums carries the errors of both.  Hence a >= |ybar|, AB_k >= |A_k| + |B_k| and the doubled counts.
    mean_i = x0 + ybar:                                                    e_i = gamma(h + 2) a + u |mean_i|
  chain averages over the M = 2 C half-chains (lane sums, a butterfly, a division: nred(C) roundings per path):
    mean acov(k):     mean_i bound_i(k) + gamma(nred) sum_i |acov_i(k)| / M
    mean of means:    mean_i e_i + gamma(nred) sum_i |mean_i| / M  =: e_mean
    B/h = sum_i d_i^2 / (M - 1), d_i = mean_i - mean:  |error of d_i| <= eps_i = e_i + e_mean + u |d_i|,
                      [sum_i (2 |d_i| + eps_i) eps_i + gamma(nred + 2) sum_i d_i^2] / (M - 1)
                      (eps_i^2 is kept: it is all that is left where every d_i is exactly 0, a column constant everywhere)

batch means (phf_batch_means.h), half-chain i, level l, n = floor(h / 2^l) batches, each batch sum a pairwise tree of depth l over
rounded y (gamma(l + 1) sum_batch |y|), abs_b = sum_batch |y|:
    S1_l    n additions of batch sums:                                     gamma(n + l + 1) sum_b abs_b
    S2_l    n additions of squared batch sums:                             gamma(n + 2 l + 3) sum_b abs_b^2
    v = (S2 - S1 S1 / n) / ((n - 1) b^2):  [gamma(n + 2 l + 5) sum_b abs_b^2 + gamma(2 (n + l) + 6) (sum_b abs_b)^2 / n] / ((n - 1) b^2)
    mean_i = x0 + S1_0 / h, the chain averages and B/h exactly as for the diagnostics.

co-moments (phf_comoments.h), half-chain k, columns i <= j:
    S_i: gamma(h + 1) sum |y_i|;   P_ij: gamma(h + 2) sum |y_i y_j|
    cov_k,ij = (P - S_i S_j / h) / (h - 1):  [gamma(h + 4) sum |y_i y_j| + gamma(2 h + 7) sum |y_i| sum |y_j| / h] / (h - 1)
    W_ij = sum_k cov_k,ij / m:   mean_k bound_k + gamma(nred) sum_k |cov_k,ij| / m
    mean_k,i as above (e_k,i);  z_k,i = mean_k,i - ref_i:  eps_k,i = e_k,i + e_ref,i + u |z_k,i|
    T_i = sum_k z_k,i:  eT_i = sum_k eps_k,i + gamma(nred) sum_k |z_k,i|
    U_ij = sum_k z_k,i z_k,j:  eU = sum_k (|z_k,i| eps_k,j + |z_k,j| eps_k,i + eps_k,i eps_k,j) + gamma(nred + 1) sum_k |z_k,i z_k,j|
    (B/h)_ij = (U - T_i T_j / m) / (m - 1):
               [eU + (|T_i| eT_j + |T_j| eT_i + eT_i eT_j) / m + 4 u (sum_k |z_i z_j| + |T_i T_j| / m)] / (m - 1)
    mean_i = ref_i + T_i / m:  e_ref,i + eT_i / m + 2 u (|ref_i| + |T_i| / m)
    pooled = (m (h-1) W + h (m-1) B/h) / (m h - 1) (host, numpy): the same combination of the two bounds + 4 u of the two terms.

WAIC (phf_pointwise.hip), point p, chain c of N draws l, the C chains merged over `levels` = ceil(C/64) + 6 pairings:
    the weights: a draw's final weight exp(l - max) is a product of exponentials whose arguments add up to D = max - l; every
    exponential is good to 1 ulp = 2 u and its argument carries u |argument|, so the weight's relative error is at most
    u D + 3 u (factors), and its absolute one at most u / e + 3 u (factors) weight, because D exp(-D) <= 1/e.  Over a chain's N
    draws and the merges that is, relative to a sum >= 1, gamma(5 N + 5 levels); lse = max + log(sum) adds 3 u (|max| + |log sum|):
    |error of lse| <= gamma(5 N + 5 levels) + 3 u (|max l| + |lse - max l|)
    the variance: m2_c = B - A (A / N) with A = sum y, B = sum y^2 (y = l - the chain's first l):
        gamma(N + 2) sum y^2 + gamma(2 N + 5) (sum |y|)^2 / N;   mean_c = x0 + A / N: e_c = gamma(N + 1) sum |y| / N + u |mean_c|
    Chan's pairwise merges add delta^2 n_a n_b / n, all terms non-negative, 6 roundings a merge: gamma(6 levels) m2; a merged
    mean carries E = max_c e_c + 2 levels u max |mean|, and by Cauchy-Schwarz sum_merges |delta| n_a n_b / n <=
    sqrt(between N C levels) with between = N sum_c (mean_c - mean)^2:
    |error of var| <= [sum_c bound(m2_c) + gamma(6 levels) m2 + 4 E sqrt(between N C levels) + 4 E^2 N C levels] / (N C - 1)

stepping stone (phf_stepping_stone.hip), rung of step Delta, chain c of N draws l (the kernel evaluates l itself; the reference takes
the l of phf_single_level_log_target at the same parameters and allows 2 ulp between the two evaluations), x = Delta l (one rounding):
    the weights as for WAIC, and every argument x - m carries the roundings of x and of m, 2 u max |x|, and 4 u Delta max |l|:
    |error of log r_c| <= b_c = gamma(5 N) + 6 u max |x| + 4 u (|max x| + |log s1| + log N),   log r_c = max x + log s1 - log N
    sum of l: gamma(N) sum |l|
    pooled log r = LSE_c(log r_c) - log C over `levels` pairings: b = max_c b_c + gamma(5 levels) + 4 u (|max_c log r_c| + |log sum| + log C)
    between-chain variance of v_c = r_c / r = exp(log r_c - log r) (divisor C - 1; the reduce reports se = sqrt(var / C)):
    eps_c = v_c (b_c + b + 4 u) + the mean of these;  [sum_c (2 |v_c - mean| + eps_c) eps_c] / (C - 1) + gamma(6 levels + 6) var
    A draw with l = -inf has weight 0 and still counts in N; a chain with a NaN l is left out of the reference and counted."""
import math
from fractions import Fraction as F

import numpy as np

U = 2.0 ** -53
SLACK = 4.0
MUS = (0.0, 4.548, -40.0, -1e4, -4.7e10)
DISTANCES = (4.0, 1e2, 1e4, 1e6)
NONFINITE = (-np.inf, np.inf, np.nan)
SHAPES = ((1, 37, None), (3, 37, None), (65, 37, None))              # (chains, rows, lags: None = the default)
LONG_SHAPE = (65, 130, 40)                                            # crosses the 32-lag block; 1 problem x 3 columns


def gamma(n):
    return n * U / (1.0 - n * U)


def nred(C):
    """roundings on a path of the reduces' chain sums: two additions per 64-chain step of a lane, six of the butterfly, a division"""
    return 2 * ((C + 63) // 64) + 6 + 2


def cuts_of(N):
    """the rows at which the cut run ends its calls: both sides of the half boundary, where x0 changes"""
    return [1, 7, 8, N // 2, N // 2 + 1]


def segments(N, cuts=None):
    """(lo, hi) of the calls of a run cut at `cuts` (None: whole)"""
    ends = sorted(set(c for c in (cuts or []) if 0 < c < N)) + [N]
    return list(zip([0] + ends[:-1], ends))


def plant_rows(N):
    """the row positions of a planted value; 'dropped middle' exists for odd N only"""
    h = N // 2
    rows = {"first of half 0": 0, "middle of half 0": h // 2, "first of half 1": N - h, "last": N - 1}
    if N % 2:
        rows["dropped middle"] = h
    return rows


# ---- generators ------------------------------------------------------------------------------------------------------------------
def ar1(rng, N, C, phi=0.5):
    """[N][C]: stationary AR(1) of unit variance"""
    x = np.empty((N, C))
    x[0] = rng.standard_normal(C)
    e = rng.standard_normal((N, C)) * math.sqrt(1.0 - phi * phi)
    for t in range(1, N):
        x[t] = phi * x[t - 1] + e[t]
    return x


def _sds(mu):
    return (1.0, 2e-3, 1e-9 * max(1.0, abs(mu)))


def columns_of(N, C, seed, which="all"):
    """list of (name, family, kappa, data [N][C]); kappa = 1 + d^2 for an outlying start, None otherwise.
    which: 'all' | 'long' (three columns for the long shape) | 'pairs' (eight columns for the co-moments and WAIC)"""
    rng = np.random.default_rng(seed)
    h = N // 2
    t = np.arange(N, dtype=np.float64)[:, None]
    cols = []
    for mu in MUS:
        for sd in _sds(mu):
            cols.append(("offset mu=%g sd=%g" % (mu, sd), "offset", None, mu + sd * ar1(rng, N, C)))
    for mu, sd in ((4.548, 2e-3), (-40.0, 1.0)):
        for d in DISTANCES:
            x = mu + sd * ar1(rng, N, C)
            x[0] = mu + d * sd
            x[N - h] = mu + d * sd
            cols.append(("outlying mu=%g sd=%g d=%g" % (mu, sd, d), "outlying start", 1.0 + d * d, x))
    for a, rise in ((0.0, 1.0), (-4.7e10, 1e6)):
        cols.append(("drift from %g by %g" % (a, rise), "drift", None, a + rise * t / (N - 1) + 1e-3 * rise * rng.standard_normal((N, C))))
    cols.append(("constant everywhere", "constant", None, np.full((N, C), 4.548)))
    cols.append(("constant per chain", "constant", None, np.tile(4.548 + 0.37 * np.arange(C), (N, 1))))
    stuck = -40.0 + ar1(rng, N, C)
    stuck[:, 0] = -40.0
    cols.append(("one stuck chain", "constant", None, stuck))
    if which == "all":
        return cols
    by = {c[0]: c for c in cols}
    if which == "long":
        names = ["offset mu=-4.7e+10 sd=47", "outlying mu=4.548 sd=0.002 d=1e+06", "drift from -4.7e+10 by 1e+06"]
    else:
        names = ["offset mu=4.548 sd=0.002", "offset mu=-40 sd=1", "offset mu=-10000 sd=1e-05", "offset mu=-4.7e+10 sd=47",
                 "outlying mu=4.548 sd=0.002 d=100", "outlying mu=-40 sd=1 d=1e+06", "drift from 0 by 1", "constant per chain"]
    return [by[n] for n in names]


class Case(object):
    """rows [N][Q][stride][C] and what its columns are"""

    def __init__(self, C, N, Q, seed, which="all", lags=None):
        per = [columns_of(N, C, seed + 1000 * q, which) for q in range(Q)]
        self.C, self.N, self.Q, self.lags = C, N, Q, lags
        self.names = [c[0] for c in per[0]]
        self.families = [c[1] for c in per[0]]
        self.kappa = [c[2] for c in per[0]]
        self.cols = len(self.names)
        self.rows = np.full((N, Q, self.cols + 1, C), np.nan)
        for q in range(Q):
            for j, c in enumerate(per[q]):
                self.rows[:, q, j, :] = c[3]


def plant(rows, value, row, q, j, c):
    out = rows.copy()
    out[row, q, j, c] = value
    return out


# ---- exact arithmetic -------------------------------------------------------------------------------------------------------------
def shifted_ints(xs):
    """one half-chain's values -> (x0 as a Fraction, Y, s): y_m = x_m - x0 = Y[m] / s exactly, s a power of two"""
    fr = [F(float(v)) for v in xs]
    ys = [f - fr[0] for f in fr]
    s = max(y.denominator for y in ys)
    return fr[0], [y.numerator * (s // y.denominator) for y in ys], s


def halves_of(col):
    """col [N] -> the two half-chains (the middle row of an odd N dropped)"""
    N = len(col)
    h = N // 2
    return col[:h], col[N - h:]


def _fl(v):
    return float(v)                                          # Fraction -> double: int / int true division is correctly rounded


def _means_reduce(means, e, C):
    """(mean of means, its bound, B/h, its bound) from exact half-chain means [M] (Fractions) and their bounds e [M]"""
    M = len(means)
    g = sum(means) / M
    e_mean = sum(e) / M + gamma(nred(C)) * _fl(sum(abs(m) for m in means)) / M
    d = [m - g for m in means]
    if M < 2:
        return g, e_mean, F(0), float("nan")
    eps = [ei + e_mean + U * abs(_fl(di)) for ei, di in zip(e, d)]
    sq = sum(di * di for di in d)
    bound = (sum((2.0 * abs(_fl(di)) + ep) * ep for di, ep in zip(d, eps)) + gamma(nred(C) + 2) * _fl(sq)) / (M - 1)
    return g, e_mean, sq / (M - 1), bound


def _dsum(pairs):
    """the sum of num / den over (num, den) pairs whose denominators are one constant times powers of two: (numerator, denominator)"""
    D = max(d for _, d in pairs)
    return sum(n * (D // d) for n, d in pairs), D


def diag_half(xs, L):
    """one half-chain: (mean, e, acov [L+1] as (numerator, denominator) pairs, bound [L+1], the short form [L+1]).  Integers
    throughout: h^3 s^2 acov(k) = h^2 Q_k - h S (A_k + B_k) + (h - k) S^2; int / int is correctly rounded"""
    x0, Y, s = shifted_ints(xs)
    h = len(Y)
    aY = [abs(v) for v in Y]
    S, aS = sum(Y), sum(aY)
    s2 = s * s
    mean = x0 + F(S, h * s)
    e = gamma(h + 2) * (aS / (h * s)) + U * abs(_fl(mean))
    acov, bound, short = [], [], []
    for k in range(L + 1):
        Qk = sum(Y[m] * Y[m - k] for m in range(k, h))
        aQk = sum(aY[m] * aY[m - k] for m in range(k, h))
        A, B = S - sum(Y[h - k:]) if k else S, S - sum(Y[:k])
        AB = 2 * aS + sum(aY[:k]) + (sum(aY[h - k:]) if k else 0)
        acov.append((h * h * Qk - h * S * (A + B) + (h - k) * S * S, h * h * h * s2))
        t1, t2, t3 = aQk / s2, aS * AB / (h * s2), (h - k) * aS * aS / (h * h * s2)
        bound.append((gamma(h + 5) * t1 + gamma(2 * h + 11) * t2 + gamma(2 * h + 9) * t3) / h)
        short.append(gamma(h + 4) * (t1 + abs(S) * (abs(A) + abs(B)) / (h * s2) + (h - k) * S * S / (h * h * s2)) / h)
    return mean, e, acov, bound, short


def diag_exact(rows, cols, lags=None):
    """what phf_diagnostics_reduce returns and the workspace's per-half-chain acov and means, exactly, with their bounds.
    rows [N][Q][stride][C] -> dict of float arrays: acov, acov_bound, acov_bound_short [Q][cols][C][2][L+1]; mean, mean_bound
    [Q][cols][C][2]; red, red_bound [Q][cols][L+3]; rhat [Q][cols] (exact W and B/h; NaN where W = 0)"""
    N, Q, _, C = rows.shape
    h = N // 2
    L = min(256 if lags is None else lags, h - 1)
    o = {"acov": np.zeros((Q, cols, C, 2, L + 1)), "mean": np.zeros((Q, cols, C, 2)), "red": np.zeros((Q, cols, L + 3)),
         "rhat": np.full((Q, cols), np.nan)}
    for k in ("acov_bound", "acov_bound_short"):
        o[k] = np.zeros_like(o["acov"])
    o["mean_bound"], o["red_bound"] = np.zeros_like(o["mean"]), np.zeros_like(o["red"])
    M = 2 * C
    for q in range(Q):
        for j in range(cols):
            means, es, acs, bds = [], [], [], []
            for c in range(C):
                for half, xs in enumerate(halves_of(rows[:, q, j, c])):
                    mean, e, acov, bound, short = diag_half(xs, L)
                    means.append(mean); es.append(e); acs.append(acov); bds.append(bound)
                    o["acov"][q, j, c, half] = [n / d for n, d in acov]
                    o["acov_bound"][q, j, c, half] = bound
                    o["acov_bound_short"][q, j, c, half] = short
                    o["mean"][q, j, c, half], o["mean_bound"][q, j, c, half] = _fl(mean), e
            for k in range(L + 1):
                tot, D = _dsum([a[k] for a in acs])
                atot, _ = _dsum([(abs(a[k][0]), a[k][1]) for a in acs])
                o["red"][q, j, k] = tot / (D * M)
                o["red_bound"][q, j, k] = sum(b[k] for b in bds) / M + gamma(nred(C)) * (atot / (D * M))
            g, eg, bh, ebh = _means_reduce(means, es, C)
            o["red"][q, j, L + 1], o["red_bound"][q, j, L + 1] = _fl(g), eg
            o["red"][q, j, L + 2], o["red_bound"][q, j, L + 2] = _fl(bh), ebh
            tot, D = _dsum([a[0] for a in acs])
            W = F(tot, D * M) * F(h, h - 1)
            if W > 0:
                o["rhat"][q, j] = math.sqrt(_fl((F(h - 1, h) * W + bh) / W))
    return o


def bm_half(xs):
    """one half-chain: (mean, e, S1 [NL], S2 [NL] (floats, rounded once), their bounds, the exact v_l (l < NL - 1) as (numerator,
    denominator) pairs and its bounds)"""
    x0, Y, s = shifted_ints(xs)
    h = len(Y)
    nl = h.bit_length()
    ss = s * s
    S1, S2, b1, b2, v, bv = [], [], [], [], [], []
    sums, asums = list(Y), [abs(t) for t in Y]
    aS = sum(asums)
    mean = x0 + F(sum(Y), h * s)
    for l in range(nl):
        n = len(sums)
        s1, s2, a1, a2 = sum(sums), sum(t * t for t in sums), sum(asums), sum(t * t for t in asums)
        S1.append(s1 / s); S2.append(s2 / ss)
        b1.append(gamma(n + l + 1) * (a1 / s)); b2.append(gamma(n + 2 * l + 3) * (a2 / ss))
        if l < nl - 1:
            bb = (n - 1) * 4 ** l
            v.append((n * s2 - s1 * s1, n * bb * ss))
            bv.append((gamma(n + 2 * l + 5) * (a2 / ss) + gamma(2 * (n + l) + 6) * (a1 * a1 / (n * ss))) / bb)
        m2 = 2 * (n // 2)
        sums = [sums[i] + sums[i + 1] for i in range(0, m2, 2)]
        asums = [asums[i] + asums[i + 1] for i in range(0, m2, 2)]
    return mean, gamma(h + 2) * (aS / (h * s)) + U * abs(_fl(mean)), S1, S2, b1, b2, v, bv


def bm_exact(rows, cols):
    """phf_batch_means_reduce and the workspace's S1, S2, exactly: dict of float arrays S1, S2 (+ _bound) [Q][cols][C][2][NL];
    red, red_bound [Q][cols][NL+1]"""
    N, Q, _, C = rows.shape
    h = N // 2
    nl = h.bit_length()
    o = {k: np.zeros((Q, cols, C, 2, nl)) for k in ("S1", "S2", "S1_bound", "S2_bound")}
    o["red"], o["red_bound"] = np.zeros((Q, cols, nl + 1)), np.zeros((Q, cols, nl + 1))
    M = 2 * C
    for q in range(Q):
        for j in range(cols):
            means, es, vs, bvs = [], [], [], []
            for c in range(C):
                for half, xs in enumerate(halves_of(rows[:, q, j, c])):
                    mean, e, S1, S2, b1, b2, v, bv = bm_half(xs)
                    means.append(mean); es.append(e); vs.append(v); bvs.append(bv)
                    o["S1"][q, j, c, half], o["S2"][q, j, c, half] = S1, S2
                    o["S1_bound"][q, j, c, half], o["S2_bound"][q, j, c, half] = b1, b2
            for l in range(nl - 1):
                tot, D = _dsum([v[l] for v in vs])                      # every v_l >= 0 (Cauchy-Schwarz): the sum of |v| is the sum
                o["red"][q, j, l] = tot / (D * M)
                o["red_bound"][q, j, l] = sum(b[l] for b in bvs) / M + gamma(nred(C)) * (tot / (D * M))
            g, eg, bh, ebh = _means_reduce(means, es, C)
            o["red"][q, j, nl - 1], o["red_bound"][q, j, nl - 1] = _fl(g), eg
            o["red"][q, j, nl], o["red_bound"][q, j, nl] = _fl(bh), ebh
    return o


def cm_pair(d, i, j):
    return i * d - i * (i - 1) // 2 + (j - i)


def cm_exact(rows, d, dropped=()):
    """phf_comoments_reduce, exactly: dict of float arrays W, Bh, pooled (+ _bound) [Q][pairs]; mean (+ _bound) [Q][d]; m [Q].
    dropped: (q, chain, half) triples left out, as the reduce leaves out a flagged half-chain"""
    N, Q, _, C = rows.shape
    h = N // 2
    npairs = d * (d + 1) // 2
    o = {k: np.zeros((Q, npairs)) for k in ("W", "Bh", "pooled", "W_bound", "Bh_bound", "pooled_bound")}
    o["mean"], o["mean_bound"], o["m"] = np.zeros((Q, d)), np.zeros((Q, d)), np.zeros(Q, dtype=int)
    g = gamma(nred(C))
    for q in range(Q):
        used = [(c, half) for c in range(C) for half in (0, 1) if (q, c, half) not in dropped]
        m = len(used)
        o["m"][q] = m
        st = []                                                   # per used half-chain: per column (x0, Y, s, aS)
        for c, half in used:
            st.append([shifted_ints(halves_of(rows[:, q, i, c])[half]) for i in range(d)])
        mean = [[x0 + F(sum(Y), h * s) for x0, Y, s in hc] for hc in st]
        absy = [[F(sum(abs(v) for v in Y), s) for x0, Y, s in hc] for hc in st]
        e = [[gamma(h + 2) * _fl(absy[k][i]) / h + U * abs(_fl(mean[k][i])) for i in range(d)] for k in range(m)]
        z = [[mean[k][i] - mean[0][i] for i in range(d)] for k in range(m)]
        eps = [[e[k][i] + e[0][i] + U * abs(_fl(z[k][i])) for i in range(d)] for k in range(m)]
        T = [sum(z[k][i] for k in range(m)) for i in range(d)]
        eT = [sum(eps[k][i] for k in range(m)) + g * _fl(sum(abs(z[k][i]) for k in range(m))) for i in range(d)]
        for i in range(d):
            o["mean"][q, i] = _fl(mean[0][i] + T[i] / m)
            o["mean_bound"][q, i] = e[0][i] + eT[i] / m + 2 * U * (abs(_fl(mean[0][i])) + abs(_fl(T[i])) / m)
            for j in range(i, d):
                p = cm_pair(d, i, j)
                covs, bsum = [], 0.0
                for k in range(m):
                    (_, Yi, si), (_, Yj, sj) = st[k][i], st[k][j]
                    P = F(sum(a * b for a, b in zip(Yi, Yj)), si * sj)
                    aP = F(sum(abs(a * b) for a, b in zip(Yi, Yj)), si * sj)
                    covs.append((P - F(sum(Yi) * sum(Yj), h * si * sj)) / (h - 1))
                    bsum += (gamma(h + 4) * _fl(aP) + gamma(2 * h + 7) * _fl(absy[k][i] * absy[k][j]) / h) / (h - 1)
                W = sum(covs) / m
                o["W"][q, p], o["W_bound"][q, p] = _fl(W), bsum / m + g * _fl(sum(abs(v) for v in covs)) / m
                Uij = sum(z[k][i] * z[k][j] for k in range(m))
                aU = _fl(sum(abs(z[k][i] * z[k][j]) for k in range(m)))
                eU = (sum(abs(_fl(z[k][i])) * eps[k][j] + abs(_fl(z[k][j])) * eps[k][i] + eps[k][i] * eps[k][j] for k in range(m))
                      + gamma(nred(C) + 1) * aU)
                Bh = (Uij - T[i] * T[j] / m) / (m - 1)
                eB = (eU + (abs(_fl(T[i])) * eT[j] + abs(_fl(T[j])) * eT[i] + eT[i] * eT[j]) / m
                      + 4 * U * (aU + abs(_fl(T[i] * T[j])) / m)) / (m - 1)
                o["Bh"][q, p], o["Bh_bound"][q, p] = _fl(Bh), eB
                w1, w2 = F(m * (h - 1), m * h - 1), F(h * (m - 1), m * h - 1)
                o["pooled"][q, p] = _fl(w1 * W + w2 * Bh)
                o["pooled_bound"][q, p] = (_fl(w1) * o["W_bound"][q, p] + _fl(w2) * eB + 4 * U * (_fl(w1 * abs(W)) + _fl(w2 * abs(Bh))))
    return o


def waic_exact(rows, points):
    """phf_waic_reduce for the 'given' likelihood (column p of a row is l of point p), exactly: float arrays lse, var (+ _bound)
    [Q][points].  The log-sum-exp by mpmath at 120 digits, the variance in Fractions."""
    import mpmath
    N, Q, _, C = rows.shape
    levels = (C + 63) // 64 + 6
    o = {k: np.zeros((Q, points)) for k in ("lse", "var", "lse_bound", "var_bound")}
    with mpmath.workdps(120):
        for q in range(Q):
            for p in range(points):
                x = rows[:, q, p, :]
                mx = float(np.max(x))
                tot = mpmath.fsum(mpmath.exp(mpmath.mpf(float(v)) - mx) for v in x.ravel())
                lse = mpmath.mpf(mx) + mpmath.log(tot)
                o["lse"][q, p] = float(lse)
                o["lse_bound"][q, p] = gamma(5 * N + 5 * levels) + 3 * U * (abs(mx) + abs(float(mpmath.log(tot))))
                means, m2s, eb, ec = [], [], 0.0, []
                for c in range(C):
                    x0, Y, s = shifted_ints(x[:, c])
                    S, aS = sum(Y), sum(abs(v) for v in Y)
                    sq = sum(v * v for v in Y)
                    means.append(x0 + F(S, N * s))
                    m2s.append((F(sq) - F(S * S, N)) / (s * s))
                    eb += gamma(N + 2) * _fl(F(sq, s * s)) + gamma(2 * N + 5) * _fl(F(aS * aS, N * s * s))
                    ec.append(gamma(N + 1) * _fl(F(aS, N * s)) + U * abs(_fl(means[-1])))
                g = sum(means) / C
                between = N * sum((mc - g) ** 2 for mc in means)
                m2 = sum(m2s) + between
                E = max(ec) + 2 * levels * U * max(abs(_fl(mc)) for mc in means)
                o["var"][q, p] = _fl(m2 / (N * C - 1))
                o["var_bound"][q, p] = (eb + gamma(6 * levels) * _fl(m2) + 4 * E * math.sqrt(_fl(between) * N * C * levels)
                                       + 4 * E * E * N * C * levels) / (N * C - 1)
    return o


def ss_exact(l, delta):
    """phf_stepping_stone_reduce from the draws' log-likelihoods l [N][Q][C] and the rungs' steps delta [Q], by mpmath at 120 digits
    (sums of l in Fractions): float arrays log_r_chain, log_r_chain_bound, sum_ll, sum_ll_bound [Q][C] (NaN for a chain with a NaN l);
    log_r, log_r_bound, var, var_bound, nan_chains [Q] (log_r and var NaN where a chain is NaN: the reduce poisons them)"""
    import mpmath
    N, Q, C = l.shape
    levels = (C + 63) // 64 + 6
    o = {k: np.full((Q, C), np.nan) for k in ("log_r_chain", "log_r_chain_bound", "sum_ll", "sum_ll_bound")}
    for k in ("log_r", "log_r_bound", "var", "var_bound"):
        o[k] = np.full(Q, np.nan)
    o["nan_chains"] = np.zeros(Q)
    with mpmath.workdps(120):
        for q in range(Q):
            lr, b = [], []
            for c in range(C):
                col = l[:, q, c]
                if np.isnan(col).any():
                    o["nan_chains"][q] += 1
                    continue
                fin = col[np.isfinite(col)]
                o["sum_ll"][q, c] = float(sum(F(float(v)) for v in col)) if fin.size == N else float(np.sum(col))
                o["sum_ll_bound"][q, c] = gamma(N) * float(np.sum(np.abs(fin)))
                x = [mpmath.mpf(float(delta[q])) * mpmath.mpf(float(v)) for v in fin] if delta[q] != 0.0 else [mpmath.mpf(0)] * N
                mx = max(x)
                s1 = mpmath.fsum(mpmath.exp(v - mx) for v in x)
                val = mx + mpmath.log(s1) - mpmath.log(N)
                bound = (gamma(5 * N) + 6 * U * float(max(abs(v) for v in x))
                         + 4 * U * (abs(float(mx)) + abs(float(mpmath.log(s1))) + math.log(N)))
                o["log_r_chain"][q, c], o["log_r_chain_bound"][q, c] = float(val), bound
                lr.append(val); b.append(bound)
            if o["nan_chains"][q] or not lr:
                continue
            top = max(lr)
            tot = mpmath.fsum(mpmath.exp(v - top) for v in lr)
            pooled = top + mpmath.log(tot) - mpmath.log(C)
            bp = max(b) + gamma(5 * levels) + 4 * U * (abs(float(top)) + abs(float(mpmath.log(tot))) + math.log(C))
            o["log_r"][q], o["log_r_bound"][q] = float(pooled), bp
            if C > 1:
                v = [mpmath.exp(t - pooled) for t in lr]
                mean = mpmath.fsum(v) / C
                var = mpmath.fsum((t - mean) ** 2 for t in v) / (C - 1)
                eps = [float(t) * (bc + bp + 4 * U) for t, bc in zip(v, b)]
                E = sum(eps) / C
                o["var"][q] = float(var)
                o["var_bound"][q] = (sum((2 * abs(float(t - mean)) + e + E) * (e + E) for t, e in zip(v, eps)) / (C - 1)
                                     + gamma(6 * levels + 6) * float(var))
    return o


# ---- what the host and the GPU tests share ---------------------------------------------------------------------------------------
def bm_fields(ws, nl):
    """batch-means state [Q][cols][5 NL + 2][C] -> (x0 [Q][cols][C][2], S1, S2 [Q][cols][C][2][NL]) (phf_batch_means.h's field order:
    x0[half] | pend[l] | S1[0][l] | S2[0][l] | S1[1][l] | S2[1][l])"""
    x0 = np.stack([ws[:, :, 0], ws[:, :, 1]], axis=-1)
    S1 = np.stack([np.moveaxis(ws[:, :, 2 + nl + 2 * half * nl:2 + nl + (2 * half + 1) * nl], 2, -1) for half in (0, 1)], axis=-2)
    S2 = np.stack([np.moveaxis(ws[:, :, 2 + nl + (2 * half + 1) * nl:2 + nl + (2 * half + 2) * nl], 2, -1) for half in (0, 1)], axis=-2)
    return x0, S1, S2


def bm_levels_hit(N, row):
    """indices of phf_batch_means_reduce's outputs [NL + 1] that read row `row` of N: the levels l < NL - 1 whose floor(h / 2^l)
    whole batches reach the row's place in its half-chain, then the mean of the means and B/h (always)"""
    h = N // 2
    m = row if row < h else row - (N - h)
    nl = h.bit_length()
    return [l for l in range(nl - 1) if m < ((h >> l) << l)] + [nl - 1, nl]


def comoments_table(out, ex, d, h):
    """phf_comoments_reduce's output [Q][out doubles] (device or twin) against cm_exact: the Table"""
    npair = d * (d + 1) // 2
    t = Table()
    t.add("co-moments", "all", "W", out[:, :npair], ex["W"], ex["W_bound"])
    t.add("co-moments", "all", "B/h", out[:, npair:2 * npair], ex["Bh"], ex["Bh_bound"])
    t.add("co-moments", "all", "mean", out[:, 2 * npair:2 * npair + d], ex["mean"], ex["mean_bound"])
    m = ex["m"][:, None].astype(float)
    pooled = (m * (h - 1.0) * out[:, :npair] + h * (m - 1.0) * out[:, npair:2 * npair]) / (m * h - 1.0)      # correlations.finalize
    t.add("co-moments", "all", "pooled", pooled, ex["pooled"], ex["pooled_bound"])
    assert np.array_equal(out[:, 2 * npair + 2 * d], ex["m"])
    return t


def cm_touched(d, j):
    """fields of a half-chain's co-moment state (x0[d] | S[d] | P | rows | flag) that involve column j, and the flag"""
    return [2 * d + d * (d + 1) // 2 + 1, j, d + j] + [2 * d + cm_pair(d, min(i, j), max(i, j)) for i in range(d)]


# ---- the table -------------------------------------------------------------------------------------------------------------------
class Table(object):
    """worst |error| / bound per (kernel, family, output)"""

    def __init__(self):
        self.worst = {}

    def add(self, kernel, family, output, got, want, bound):
        """got, want, bound: arrays of one shape.  Returns the worst ratio (0 where got == want, also at bound 0)"""
        got, want, bound = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), np.asarray(bound, dtype=np.float64)
        err = np.abs(got - want)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0.0, 0.0, err / (SLACK * bound))
        ratio = np.where(np.isnan(ratio), np.inf, ratio)
        w = float(np.max(ratio)) if ratio.size else 0.0
        key = (kernel, family, output)
        self.worst[key] = max(self.worst.get(key, 0.0), w)
        return w

    def lines(self):
        out = ["%-14s %-15s %-22s %s" % ("kernel", "family", "output", "worst |error| / (4 bound)")]
        for (kernel, family, output), w in sorted(self.worst.items()):
            out.append("%-14s %-15s %-22s %.3g" % (kernel, family, output, w))
        return out
