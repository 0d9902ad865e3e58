"""Convergence diagnostics of many-chain runs: split-R-hat, multi-chain ESS and the Monte-Carlo standard error of the mean.

The estimators are those of the Stan reference manual (Gelman et al., BDA3 11.4-11.5; Vehtari et al. 2021) WITHOUT rank
normalisation, which would need every draw resident at once.  Per problem and column, over the post-burn-in rows of C chains:
each chain is split into two half-chains of h = floor(N/2) rows (the middle row of an odd N is dropped), M = 2C.  The device
accumulates every half-chain's mean and autocovariance acov(k), k = 0..L, L = min(K, h-1), while the sampler's rows stream past
(phf_diagnostics_accumulate, one segment at a time: nothing is kept) and averages them over the half-chains
(phf_diagnostics_reduce).  finalize() then applies, on the host:

    W = mean_i s_i^2 with s_i^2 = acov_i(0) h/(h-1),  B/h = var_i(mean_i) (divisor M-1),  var+ = (h-1)/h W + B/h,
    R-hat = sqrt(var+/W),  rho_0 = 1,  rho_k = 1 - (W - mean_i acov_i(k))/var+,  P_t = rho_2t + rho_2t+1,
    Geyer's initial positive sequence (t = 0..T, T+1 the first t > 0 with P_t <= 0), then the initial monotone one
    (P_t <- min(P_t, P_t-1)),  tau = max(-1 + 2 sum_t P_t, 1/log10(M h)),  ESS = M h / tau,  MCSE = sqrt(var+/ESS).

ESS and MCSE are NaN (null in JSON) when the sequence has not turned non-positive by lag L < h-1 (lag_limit_reached: a cut there
would overstate the ESS) and, with R-hat, when W = 0 (a column that never moved) or W is not finite (a value that is not finite in
the column); json_record() then names the cause per column under "reason".  When L = h-1 and the sequence never turns, every
available pair P_t (2t+1 <= L) is kept."""
import ctypes as C

import numpy as np
import torch

from . import _lib, accumulator
from ._lib import _num
from .sampler import _ptr, _stream_ptr

DEFAULT_LAGS = 256
RHAT_THRESHOLD = 1.01
METHOD = ("split-R-hat and multi-chain ESS (Stan reference manual; Geyer initial positive + monotone sequence) without rank "
          "normalisation; MCSE of the mean = sqrt(var+/ESS)")
UNDETERMINED = "W is not positive: the column never moved within a half-chain (0/0), or it holds a value that is not finite"


def effective_lags(total_rows, lags=DEFAULT_LAGS):
    """L = min(K, floor(total_rows/2) - 1)"""
    return min(int(lags), int(total_rows) // 2 - 1)


def workspace_bytes(num_problems, columns, chains, total_rows, lags=DEFAULT_LAGS):
    """device bytes ChainDiagnostics holds: num_problems * columns * chains * (4L + 6) doubles (raises on an invalid shape)"""
    return accumulator.workspace_bytes("phf_diagnostics_workspace_bytes", num_problems, columns, chains, total_rows, lags)


def finalize(mean_acov, xbar_var, h, num_half_chains):
    """R-hat, ESS, MCSE and lag_limit_reached from the reduced quantities (module docstring).
    mean_acov [..., L+1]: mean over the M half-chains of acov(k); xbar_var [...]: variance of the half-chain means (divisor M-1);
    h: rows per half-chain.  Returns four arrays of shape [...] (NaN where not determined)."""
    acov = np.asarray(mean_acov, dtype=np.float64)
    bh = np.asarray(xbar_var, dtype=np.float64)
    L = acov.shape[-1] - 1
    M = int(num_half_chains)
    h = int(h)
    if L < 1 or L > h - 1 or M < 2:
        raise ValueError("need 1 <= L <= h-1 and at least two half-chains (L = %d, h = %d, M = %d)" % (L, h, M))
    W = acov[..., 0] * h / (h - 1.0)
    varp = (h - 1.0) / h * W + bh
    moved = W > 0
    Ws = np.where(moved, W, 1.0)
    vs = np.where(moved, varp, 1.0)
    rhat = np.where(moved, np.sqrt(vs / Ws), np.nan)
    rho = 1.0 - (Ws[..., None] - acov) / vs[..., None]
    rho[..., 0] = 1.0
    n_pairs = (L + 1) // 2                                   # t = 0..(L-1)/2: both lags 2t and 2t+1 <= L
    P = rho[..., 0:2 * n_pairs:2] + rho[..., 1:2 * n_pairs:2]
    turned = P[..., 1:] <= 0
    cut = np.any(turned, axis=-1)
    kept = np.where(cut, np.argmax(turned, axis=-1) + 1, n_pairs)            # number of terms t = 0..T
    Pm = np.minimum.accumulate(P, axis=-1)
    mask = np.arange(n_pairs) < kept[..., None]
    tau = np.maximum(-1.0 + 2.0 * np.sum(np.where(mask, Pm, 0.0), axis=-1), 1.0 / np.log10(M * h))
    limit = ~cut & (L < h - 1)
    ok = moved & ~limit
    ess = np.where(ok, M * h / tau, np.nan)
    mcse = np.where(ok, np.sqrt(vs / np.where(ok, ess, 1.0)), np.nan)
    return rhat, ess, mcse, limit & moved


class ChainDiagnostics(accumulator.RowAccumulator):
    """Streaming diagnostics of num_problems x columns over `chains` chains and total_rows post-burn-in rows.
    accumulate() takes the rows in order, a segment at a time, as views of the sampler's row buffer [rows][Q][stride][chains]
    (asynchronous, on the current stream); result() reduces and finalizes."""

    def __init__(self, num_problems, chains, columns, total_rows, lags=DEFAULT_LAGS, device="cuda"):
        accumulator.RowAccumulator.__init__(self, device)
        self.Q, self.C, self.cols, self.N, self.K = int(num_problems), int(chains), int(columns), int(total_rows), int(lags)
        self.min_cols = self.cols
        self.L = effective_lags(self.N, self.K)
        self.h = self.N // 2
        self._init_workspace(workspace_bytes(self.Q, self.cols, self.C, self.N, self.K), "phf_diagnostics_init", self.Q, self.cols, self.C,
                             self.N, self.K)

    def _accumulate(self, rows, n):
        _lib.check(self.lib.phf_diagnostics_accumulate(_ptr(rows), n, self.Q, rows.shape[2], self.C, self.cols, self.rows_seen, self.N,
                                                       self.K, _ptr(self.ws), C.c_size_t(self.nbytes), _stream_ptr(self.device)),
                   "phf_diagnostics_accumulate")

    def reduced(self):
        """[Q][cols][L+3] numpy: mean acov(0..L), mean of the half-chain means, their variance (divisor M-1)"""
        self._check_complete()
        out = torch.empty((self.Q, self.cols, self.L + 3), dtype=torch.float64, device=self.device)
        _lib.check(self.lib.phf_diagnostics_reduce(self.Q, self.cols, self.C, self.N, self.K, _ptr(self.ws), C.c_size_t(self.nbytes),
                                                   _ptr(out), _stream_ptr(self.device)), "phf_diagnostics_reduce")
        return out.cpu().numpy()

    def result(self):
        """dict of numpy [Q][cols]: rhat, ess, mcse_mean (NaN where not determined), lag_limit_reached (bool)"""
        red = self.reduced()
        rhat, ess, mcse, limit = finalize(red[..., :self.L + 1], red[..., self.L + 2], self.h, 2 * self.C)
        return {"rhat": rhat, "ess": ess, "mcse_mean": mcse, "lag_limit_reached": limit}


def diagnose(chains, lags=DEFAULT_LAGS, device="cuda"):
    """chains: array [rows][cols][chains] already in memory (burn-in removed).  Returns the result() dict of its one problem,
    arrays [cols]."""
    x = np.asarray(chains, dtype=np.float64)
    if x.ndim == 2:
        x = x[:, :, None]
    n, cols, c = x.shape
    d = ChainDiagnostics(1, c, cols, n, lags, device)
    d.accumulate(torch.from_numpy(np.ascontiguousarray(x[:, None])).to(d.device))
    return {k: v[0] for k, v in d.result().items()}


def json_record(res, q, lags, total_rows, chains, columns=None):
    """the command lines' "diagnostics" object of problem q (NaN -> null)"""
    rec = {"rhat": [_num(v) for v in res["rhat"][q]], "ess": [_num(v) for v in res["ess"][q]],
           "mcse_mean": [_num(v) for v in res["mcse_mean"][q]], "lag_limit_reached": [bool(v) for v in res["lag_limit_reached"][q]],
           "lags": int(lags), "rows_per_half_chain": int(total_rows) // 2, "half_chains": 2 * int(chains), "method": METHOD}
    if columns is not None:
        rec["columns"] = list(columns)
    if any(v is None for v in rec["rhat"]):
        rec["reason"] = [UNDETERMINED if v is None else None for v in rec["rhat"]]
    return rec


def report_line(rank, names, rhat, ess):
    """one line per rank: how many problems have some R-hat > 1.01 (or undetermined) and the worst one.
    rhat, ess: one 1-d array of columns per problem (problems of different groups may have different columns)"""
    if len(names) == 0:
        return "diagnostics [rank %d]: no problems" % rank
    worst = np.array([np.max(np.where(np.isnan(r), np.inf, r)) for r in rhat])
    bad = int(np.sum(worst > RHAT_THRESHOLD))
    undetermined = sum(1 for e in ess if np.any(np.isnan(e)))
    w = int(np.argmax(worst))
    return ("diagnostics [rank {}]: {} of {} with R-hat > {} on some column, {} with an ESS not determined; worst: {} (R-hat {:.4f})"
            .format(rank, bad, len(names), RHAT_THRESHOLD, undetermined, names[w], float(worst[w])))
