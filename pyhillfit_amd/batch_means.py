"""ESS and MCSE beyond the lag limit: batch means on a dyadic ladder of batch sizes (the "blocking" method of Flyvbjerg & Petersen
1989; the estimator behind mcmcse; Vats & Flegal's lugsail combination as a second opinion).

diagnostics.py sums at most L autocovariances; a column whose autocorrelation time exceeds that is reported without ESS.  Here every
half-chain (h = floor(N/2) rows, split as in diagnostics.py, M = 2C of them) is cut into batches of b = 2^l rows, l = 0..floor(log2 h),
while the rows stream past (phf_batch_means_accumulate: O(log N) state per chain, nothing is kept); phf_batch_means_reduce gives, per
level with n_l = floor(h/b) >= 2 batches, the mean over the half-chains of the variance of the batch means.  finalize() then applies, on
the host:

    rung l:    sigma2_l = b * mean_i v_i(l),   nu_l = M (n_l - 1),   r_l = sqrt(2 / nu_l)      (relative standard error of sigma2_l)
    top rung:  sigma2_top = h * B/h  (B/h = the variance of the half-chain means, divisor M - 1),   nu = M - 1
    var+ = (h-1)/h W + B/h  with W = sigma2_0
    plateau:   walking the rungs upward, the top rung last, l* = the first rung k with sigma2_{k+1} - sigma2_k <= r_{k+1} sigma2_{k+1};
               sigma2 = sigma2_{l*+1},  tau = max(sigma2 / var+, 1/log10(M h)),  ESS = M h / tau,  MCSE = sqrt(var+ / ESS),
               tau_rel_se = r_{l*+1},  tau_lugsail = (2 sigma2_{l*+1} - sigma2_{l*}) / var+   (not used for the ESS)
    chains must agree:  sigma2_top > sigma2 (1 + 4 r_top)  means the within-chain ladder does not explain the spread of the chain
               means (chains that mix locally and sit apart): chains_agree false, ESS and MCSE NaN, and
               ess_upper_bound = M h var+ / max_l sigma2_l instead.  The same when no plateau is found (plateau_reached false).

W = 0 (a column that never moved): everything NaN.  NaN is null in the JSON."""
import ctypes as C

import numpy as np
import torch

from . import _lib, accumulator
from ._lib import _num
from .sampler import _ptr, _stream_ptr

METHOD = ("batch means on a dyadic ladder of batch sizes (Flyvbjerg & Petersen 1989) over split half-chains: sigma2 at the first rung "
          "whose successor is within one relative standard error sqrt(2/nu), the between-chain rung last; tau = sigma2/var+, "
          "ESS = draws/tau, MCSE of the mean = sqrt(var+/ESS); no ESS where the chain means spread beyond 1 + 4 sqrt(2/(M-1)) of "
          "the ladder's sigma2 or no plateau is found")
DE_NOTE = ("the top rung is a between-chain variance: with chains coupled by differential-evolution moves its standard error is "
           "optimistic (as for R-hat), so chains_agree is a weaker check here")
FIELDS = ("ess", "mcse_mean", "tau", "tau_rel_se", "tau_lugsail", "level", "batch_rows", "plateau_reached", "chains_agree",
          "ess_upper_bound")


def levels(total_rows):
    """NL = floor(log2 h) + 1, h = floor(total_rows / 2)"""
    return (int(total_rows) // 2).bit_length()


def workspace_bytes(num_problems, columns, chains, total_rows):
    """device bytes BatchMeans holds: num_problems * columns * chains * (5 NL + 2) doubles (raises on an invalid shape)"""
    return accumulator.workspace_bytes("phf_batch_means_workspace_bytes", num_problems, columns, chains, total_rows)


def finalize(reduced, h, num_half_chains):
    """The estimator of the module docstring.  reduced [..., NL + 1] as phf_batch_means_reduce writes it: the mean over the half-chains
    of the variance of the batch means for levels 0..NL-2, the mean of the half-chain means, their variance (divisor M - 1).
    Returns a dict of arrays [...]: the FIELDS (float NaN where not determined; level, batch_rows int, -1 / 0 where not)."""
    red = np.asarray(reduced, dtype=np.float64)
    h, M = int(h), int(num_half_chains)
    nl = h.bit_length()
    if h < 2 or M < 2 or red.shape[-1] != nl + 1:
        raise ValueError("need h >= 2, at least two half-chains and NL + 1 = %d reduced values (h = %d, M = %d, got %d)"
                         % (nl + 1, h, M, red.shape[-1]))
    b = np.array([float(1 << l) for l in range(nl - 1)] + [float(h)])
    n = np.array([float(h >> l) for l in range(nl - 1)])
    r = np.sqrt(2.0 / np.append(M * (n - 1.0), M - 1.0))                     # the rungs' relative standard errors, the top rung last
    sig = np.concatenate([red[..., :nl - 1], red[..., nl:nl + 1]], axis=-1) * b          # [..., K], K = NL rungs
    K = nl
    W = red[..., 0]
    varp = (h - 1.0) / h * W + red[..., nl]
    moved = W > 0
    vs = np.where(moved, varp, 1.0)
    flat = (sig[..., 1:] - sig[..., :-1]) <= r[1:] * sig[..., 1:]            # [..., K-1]: rung k against its successor
    found = np.any(flat, axis=-1) & moved
    kstar = np.where(found, np.argmax(flat, axis=-1), 0)
    up = kstar + 1
    s_lo = np.take_along_axis(sig, kstar[..., None], axis=-1)[..., 0]
    s_hat = np.take_along_axis(sig, up[..., None], axis=-1)[..., 0]
    agree = found & ~(sig[..., K - 1] > s_hat * (1.0 + 4.0 * r[K - 1]))
    ok = found & agree
    tau = np.where(ok, np.maximum(s_hat / vs, 1.0 / np.log10(M * h)), np.nan)
    ess = M * h / tau
    mcse = np.sqrt(vs / np.where(ok, ess, 1.0))
    bound = np.where(moved & ~ok, M * h * vs / np.where(moved, np.max(sig, axis=-1), 1.0), np.nan)
    return {"ess": ess, "mcse_mean": np.where(ok, mcse, np.nan), "tau": tau, "tau_rel_se": np.where(ok, r[up], np.nan),
            "tau_lugsail": np.where(ok, (2.0 * s_hat - s_lo) / vs, np.nan), "level": np.where(found, up, -1),
            "batch_rows": np.where(found, b[up].astype(np.int64), 0), "plateau_reached": found, "chains_agree": agree,
            "ess_upper_bound": bound}


class BatchMeans(accumulator.RowAccumulator):
    """Streaming batch means of num_problems x columns over `chains` chains and total_rows post-burn-in rows, used like
    diagnostics.ChainDiagnostics: accumulate() takes the rows in order, a segment at a time, as views of the sampler's row buffer
    [rows][Q][stride][chains] (asynchronous, on the current stream); result() reduces and finalizes."""

    def __init__(self, num_problems, chains, columns, total_rows, device="cuda"):
        accumulator.RowAccumulator.__init__(self, device)
        self.Q, self.C, self.cols, self.N = int(num_problems), int(chains), int(columns), int(total_rows)
        self.min_cols = self.cols
        self.h = self.N // 2
        self.nl = levels(self.N)
        self._init_workspace(workspace_bytes(self.Q, self.cols, self.C, self.N), "phf_batch_means_init", self.Q, self.cols, self.C, self.N)

    def _accumulate(self, rows, n):
        _lib.check(self.lib.phf_batch_means_accumulate(_ptr(rows), n, self.Q, rows.shape[2], self.C, self.cols, self.rows_seen, self.N,
                                                       _ptr(self.ws), C.c_size_t(self.nbytes), _stream_ptr(self.device)),
                   "phf_batch_means_accumulate")

    def workspace(self):
        """the device state as numpy [Q][cols][5 NL + 2][C] (include/pyhillfit_amd.h names the fields)"""
        return self.ws[:self.Q * self.cols * (5 * self.nl + 2) * self.C].reshape(self.Q, self.cols, 5 * self.nl + 2, self.C).cpu().numpy()

    def reduced(self):
        """[Q][cols][NL+1] numpy: what phf_batch_means_reduce writes"""
        self._check_complete()
        out = torch.empty((self.Q, self.cols, self.nl + 1), dtype=torch.float64, device=self.device)
        _lib.check(self.lib.phf_batch_means_reduce(self.Q, self.cols, self.C, self.N, _ptr(self.ws), C.c_size_t(self.nbytes), _ptr(out),
                                                   _stream_ptr(self.device)), "phf_batch_means_reduce")
        return out.cpu().numpy()

    def result(self):
        """finalize()'s dict, arrays [Q][cols]"""
        return finalize(self.reduced(), self.h, 2 * self.C)


def diagnose(chains, device="cuda"):
    """chains: array [rows][cols][chains] already in memory (burn-in removed).  Returns the result() dict of its one problem,
    arrays [cols]."""
    x = np.asarray(chains, dtype=np.float64)
    if x.ndim == 2:
        x = x[:, :, None]
    n, cols, c = x.shape
    d = BatchMeans(1, c, cols, n, device)
    d.accumulate(torch.from_numpy(np.ascontiguousarray(x[:, None])).to(d.device))
    return {k: v[0] for k, v in d.result().items()}


def json_record(res, q, de_coupled=False):
    """the "batch_means" object inside the command lines' "diagnostics" object of problem q (NaN -> null)"""
    rec = {}
    for k in FIELDS:
        v = res[k][q]
        if k in ("plateau_reached", "chains_agree"):
            rec[k] = [bool(x) for x in v]
        elif k in ("level", "batch_rows"):
            rec[k] = [int(x) if x > 0 else None for x in v]
        else:
            rec[k] = [_num(x) for x in v]
    rec["method"] = METHOD
    if de_coupled:
        rec["note"] = DE_NOTE
    return rec


def report_line(rank, names, ess_geyer, ess_ladder, tau, thinning):
    """one line per rank: how many problems still have a column with no ESS from either estimator, and the largest tau in iterations.
    ess_geyer, ess_ladder, tau: one 1-d array of columns per problem"""
    if len(names) == 0:
        return "batch means [rank %d]: no problems" % rank
    neither = sum(1 for g, l in zip(ess_geyer, ess_ladder) if np.any(np.isnan(np.asarray(g, dtype=float)) & np.isnan(l)))
    worst = np.array([np.max(np.where(np.isnan(t), -np.inf, t)) for t in tau])
    w = int(np.argmax(worst))
    largest = ("largest tau {:.0f} iterations ({})".format(float(worst[w]) * thinning, names[w]) if np.isfinite(worst[w])
               else "no tau determined")
    return "batch means [rank {}]: {} of {} with an ESS determined by neither estimator on some column; {}".format(
        rank, neither, len(names), largest)
