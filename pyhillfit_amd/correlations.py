"""Posterior correlations of the parameter columns and the multivariate R-hat: the one analysis that looks across columns.

Per problem, over the post-burn-in rows of C chains and the d parameter columns of a row (the log-target is left out): every chain is
split into two half-chains of h = floor(N/2) rows exactly as pyhillfit_amd/diagnostics.py splits it (the middle row of an odd N is
dropped, h >= 4).  The device accumulates every half-chain's co-moments while the sampler's rows stream past (phf_comoments_accumulate,
one segment at a time: nothing is kept) and reduces them (phf_comoments_reduce) to

    W    the mean over the m used half-chains of their sample covariance matrices (divisor h - 1),
    B/h  the sample covariance matrix of the m half-chain means (divisor m - 1),

a half-chain with a non-finite parameter in any row being dropped whole (half_chains_dropped), so that all used ones have the same
length.  finalize() then gives, on the host:

    the pooled covariance  (m (h-1) W + h (m-1) B/h) / (m h - 1)  of all used draws, its sd and its correlation matrix;
    the within correlation matrix, from W alone: the shape of the posterior as ONE chain sees it, not inflated by chains that sit apart;
    rhat_from_moments_j = sqrt((h-1)/h + (B/h)_jj / W_jj): the split-R-hat of --diagnostics from the diagonals;
    lambda_max = the largest eigenvalue of W^-1 (B/h)  and  rhat_multivariate = sqrt((h-1)/h + lambda_max).

rhat_multivariate is the multivariate potential scale reduction factor of Brooks & Gelman (1998, eq. 4.1) written in the convention of
this project's split-R-hat: WITHOUT their (m+1)/m factor on lambda_max, as the split-R-hat of the Stan reference manual carries no such
factor either.  It is then exactly the largest split-R-hat that any linear combination of the columns can have (the Rayleigh quotient
of B/h against W), so rhat_multivariate >= max_j rhat_from_moments_j, with equality at d = 1.  `apart_direction` is the eigenvector
of lambda_max as loadings on the columns in units of their within-chain standard deviations, scaled to unit norm, its
largest-magnitude loading positive: the linear combination along which the chains disagree most.  `principal_axes` are the eigenvalues
of the within correlation matrix in descending order, their condition number and the loadings of the longest axis: the flat direction
inside a chain.  The eigenproblem is solved in those units: a Cholesky factor L of the within correlation matrix (W scaled by its
diagonal), then the symmetric eigenproblem of L^-1 (B/h scaled) L^-T.

Where W is singular (a column that never moved) or fewer than two half-chains remain, the affected entries are NaN (null in JSON) and
`reason` says why."""
import ctypes as C

import numpy as np
import torch

from . import _lib, accumulator
from ._lib import _num
from .sampler import _ptr, _stream_ptr

RHAT_THRESHOLD = 1.01
MIN_HALF = 4
METHOD = ("pooled and within-chain correlation of the parameter columns from per-half-chain co-moments; multivariate R-hat = "
          "sqrt((h-1)/h + lambda_max(W^-1 B/h)) (Brooks & Gelman 1998 in the split-R-hat convention, without their (m+1)/m factor), "
          "apart_direction = its eigenvector in units of the within-chain sd")


def pairs(d):
    return d * (d + 1) // 2


def fields(d):
    """doubles of one half-chain's state: x0[d] | S[d] | P[d (d+1) / 2] | rows | flag (phf_comoments.h)"""
    return 2 * d + pairs(d) + 2


def out_doubles(d):
    return 2 * pairs(d) + 2 * d + 4


def workspace_bytes(num_problems, columns, chains, total_rows):
    """device bytes PosteriorCorrelations holds: num_problems * 2 * chains * fields(columns) doubles (raises on an invalid shape)"""
    return accumulator.workspace_bytes("phf_comoments_workspace_bytes", num_problems, columns, chains, total_rows)


def unpack(reduced, d):
    """one problem's reduced output [out_doubles(d)] -> (W [d][d], B/h [d][d], mean [d], m, dropped, h)"""
    r = np.asarray(reduced, dtype=np.float64)
    n = pairs(d)
    iu = np.triu_indices(d)
    W, Bh = np.zeros((d, d)), np.zeros((d, d))
    W[iu], Bh[iu] = r[:n], r[n:2 * n]
    W, Bh = W + np.triu(W, 1).T, Bh + np.triu(Bh, 1).T
    return W, Bh, r[2 * n:2 * n + d].copy(), int(r[2 * n + 2 * d]), int(r[2 * n + 2 * d + 1]), int(r[2 * n + 2 * d + 2])


def _signed(v):
    """unit norm, the largest-magnitude loading positive"""
    v = v / np.linalg.norm(v)
    return -v if v[np.argmax(np.abs(v))] < 0 else v


def _scaled(M, s):
    """M / (s s^T) with an exact unit diagonal; NaN where a scale is not positive"""
    ok = s > 0
    safe = np.where(ok, s, 1.0)
    R = M / np.outer(safe, safe)
    R[~ok, :] = np.nan
    R[:, ~ok] = np.nan
    R[np.diag_indices_from(R)] = np.where(ok, 1.0, np.nan)
    return R


def finalize(W, Bh, mean, m, h, dropped=0, columns=None):
    """The result of one problem (module docstring) from W [d][d], B/h [d][d], the grand mean [d], the m half-chains used and their
    length h.  A dict of numpy arrays and numbers, NaN / None where not determined, `reason` then says why."""
    W, Bh, mean = np.asarray(W, dtype=np.float64), np.asarray(Bh, dtype=np.float64), np.asarray(mean, dtype=np.float64)
    d, m, h = len(mean), int(m), int(h)
    nan_v, nan_m = np.full(d, np.nan), np.full((d, d), np.nan)
    res = {"columns": list(columns) if columns is not None else ["column_%d" % i for i in range(d)], "rows_per_half_chain": h,
           "half_chains": m, "half_chains_dropped": int(dropped), "mean": nan_v, "sd": nan_v, "correlation": nan_m,
           "within_correlation": nan_m, "W": nan_m, "B_over_h": nan_m, "rhat_from_moments": nan_v, "rhat_multivariate": np.nan,
           "lambda_max": np.nan, "apart_direction": nan_v, "principal_axes": None, "strongest_pair": None, "reason": None}
    if m < 2:
        res["reason"] = "fewer than two half-chains without a non-finite row (%d left, %d dropped)" % (m, dropped)
        return res
    pooled = (m * (h - 1.0) * W + h * (m - 1.0) * Bh) / (m * h - 1.0)
    sd = np.sqrt(np.maximum(np.diag(pooled), 0.0))
    w = np.diag(W).copy()
    moved = w > 0
    sw = np.sqrt(np.where(moved, w, 0.0))
    Wc = _scaled(W, sw)
    res.update(mean=mean, sd=sd, correlation=_scaled(pooled, sd), within_correlation=Wc, W=W, B_over_h=Bh,
               rhat_from_moments=np.where(moved, np.sqrt((h - 1.0) / h + np.diag(Bh) / np.where(moved, w, 1.0)), np.nan))
    if not np.all(moved):
        res["reason"] = "W is singular: %s never moved within a half-chain" % ", ".join(res["columns"][i] for i in np.flatnonzero(~moved))
        return res
    try:
        L = np.linalg.cholesky(Wc)
    except np.linalg.LinAlgError:
        res["reason"] = "W is singular: the within correlation matrix is not positive definite"
        return res
    Bc = Bh / np.outer(sw, sw)
    A = np.linalg.solve(L, np.linalg.solve(L, Bc).T)                       # L^-1 Bc L^-T
    ev, evec = np.linalg.eigh(0.5 * (A + A.T))
    # lambda_max is at least every Rayleigh quotient of B/h against W; at the unit vectors those are Bc_jj (rhat_from_moments)
    lam = max(float(ev[-1]), float(np.max(np.diag(Bc))))
    res.update(lambda_max=lam, rhat_multivariate=float(np.sqrt((h - 1.0) / h + lam)),
               apart_direction=_signed(np.linalg.solve(L.T, evec[:, -1])))
    pev, pvec = np.linalg.eigh(Wc)
    res["principal_axes"] = {"eigenvalues": pev[::-1].copy(), "condition_number": float(pev[-1] / pev[0]) if pev[0] > 0 else np.nan,
                             "longest_axis": _signed(pvec[:, -1])}
    if d >= 2:
        off = np.abs(np.triu(Wc, 1))
        i, j = np.unravel_index(np.argmax(off), off.shape)
        res["strongest_pair"] = (int(i), int(j), float(Wc[i, j]))
    return res


class PosteriorCorrelations(accumulator.RowAccumulator):
    """Streaming co-moments of num_problems problems over `chains` chains, the d = len(columns) leading columns of a row and
    total_rows post-burn-in rows.  accumulate() takes the rows in order, a segment at a time, as views of the sampler's row buffer
    [rows][Q][stride][chains] (asynchronous, on the current stream); result() reduces and finalizes, per problem."""

    def __init__(self, num_problems, chains, columns, total_rows, device="cuda"):
        accumulator.RowAccumulator.__init__(self, device)
        self.columns = ["column_%d" % i for i in range(columns)] if isinstance(columns, int) else list(columns)
        self.Q, self.C, self.d, self.N = int(num_problems), int(chains), len(self.columns), int(total_rows)
        self.min_cols = self.d
        self.h = self.N // 2
        self._init_workspace(workspace_bytes(self.Q, self.d, self.C, self.N), "phf_comoments_init", self.Q, self.d, self.C, self.N)

    def _accumulate(self, rows, n):
        _lib.check(self.lib.phf_comoments_accumulate(_ptr(rows), n, self.Q, rows.shape[2], self.C, self.d, self.rows_seen, self.N,
                                                     _ptr(self.ws), C.c_size_t(self.nbytes), _stream_ptr(self.device)),
                   "phf_comoments_accumulate")

    def workspace(self):
        """the state as numpy [Q][2][fields(d)][C] (phf_comoments.h)"""
        return self.ws.cpu().numpy().reshape(self.Q, 2, fields(self.d), self.C)

    def reduced(self):
        """[Q][out_doubles(d)] numpy: W | B/h (upper triangles) | grand mean | shifted sums of means | m | dropped | h | 0"""
        self._check_complete()
        out = torch.empty((self.Q, out_doubles(self.d)), dtype=torch.float64, device=self.device)
        _lib.check(self.lib.phf_comoments_reduce(self.Q, self.d, self.C, self.N, _ptr(self.ws), C.c_size_t(self.nbytes), _ptr(out),
                                                 _stream_ptr(self.device)), "phf_comoments_reduce")
        return out.cpu().numpy()

    def result(self):
        """per problem, finalize()'s dict"""
        return [finalize_reduced(r, self.d, self.columns) for r in self.reduced()]


def finalize_reduced(reduced, d, columns=None):
    W, Bh, mean, m, dropped, h = unpack(reduced, d)
    return finalize(W, Bh, mean, m, h, dropped, columns)


def correlations_of_draws(draws, columns=None, device="cuda"):
    """draws: array [rows][d][chains] already in memory (burn-in and the log-target column removed).  Returns finalize()'s dict of
    its one problem; the accumulation runs on the GPU, so the result is that of a run fed the same rows, bit for bit."""
    x = np.asarray(draws, dtype=np.float64)
    if x.ndim == 2:
        x = x[:, :, None]
    n, d, c = x.shape
    acc = PosteriorCorrelations(1, c, d if columns is None else columns, n, device)
    if acc.d != d:
        raise ValueError("%d column names for %d columns" % (acc.d, d))
    acc.accumulate(torch.from_numpy(np.ascontiguousarray(x[:, None])).to(acc.device))
    res = acc.result()[0]
    acc.free()
    return res


def _vec(v):
    return [_num(x) for x in np.asarray(v).ravel()]


def _mat(M):
    return [[_num(x) for x in row] for row in np.asarray(M)]


def json_record(res):
    """the command lines' "correlations" object of one problem (NaN -> null)"""
    cols = res["columns"]
    rec = {"columns": list(cols), "rows_per_half_chain": res["rows_per_half_chain"], "half_chains": res["half_chains"],
           "half_chains_dropped": res["half_chains_dropped"], "mean": _vec(res["mean"]), "sd": _vec(res["sd"]),
           "correlation": _mat(res["correlation"]), "within_correlation": _mat(res["within_correlation"]),
           "rhat_from_moments": _vec(res["rhat_from_moments"]), "rhat_multivariate": _num(res["rhat_multivariate"]),
           "lambda_max": _num(res["lambda_max"])}
    determined = res["principal_axes"] is not None
    rec["apart_direction"] = {c: _num(v) for c, v in zip(cols, res["apart_direction"])} if determined else None
    if determined:
        pa = res["principal_axes"]
        rec["principal_axes"] = {"eigenvalues": _vec(pa["eigenvalues"]), "condition_number": _num(pa["condition_number"]),
                                 "longest_axis": {c: _num(v) for c, v in zip(cols, pa["longest_axis"])}}
    else:
        rec["principal_axes"] = None
    sp = res["strongest_pair"]
    rec["strongest_pair"] = {"columns": [cols[sp[0]], cols[sp[1]]], "within_correlation": _num(sp[2])} if sp is not None else None
    if res["reason"] is not None:
        rec["reason"] = res["reason"]
    rec["method"] = METHOD
    return rec


def _is(name, what):
    return name.lower().startswith(what)


def report_line(rank, names, results):
    """one line per rank: how many problems have a multivariate R-hat > 1.01 (or none determined), the worst with the two largest
    loadings of its apart_direction, and the largest |within correlation| between a pIC50 column and a Hill column"""
    if len(names) == 0:
        return "correlations [rank %d]: no problems" % rank
    worst = np.array([np.inf if np.isnan(r["rhat_multivariate"]) else r["rhat_multivariate"] for r in results])
    finite = np.where(np.isinf(worst), -np.inf, worst)
    bad, undetermined = int(np.sum(finite > RHAT_THRESHOLD)), int(np.sum(np.isinf(worst)))
    line = "correlations [rank {}]: {} of {} with a multivariate R-hat > {}, {} not determined".format(
        rank, bad, len(names), RHAT_THRESHOLD, undetermined)
    if np.any(np.isfinite(finite)):
        w = int(np.argmax(finite))
        r = results[w]
        top = np.argsort(-np.abs(r["apart_direction"]))[:2]
        line += "; worst: {} (R-hat {:.4f} along {})".format(
            names[w], float(worst[w]), " ".join("{:+.2f} {}".format(float(r["apart_direction"][i]), r["columns"][i]) for i in top))
    best = None
    for name, r in zip(names, results):
        Wc, cols = r["within_correlation"], r["columns"]
        for i, ci in enumerate(cols):
            for j, cj in enumerate(cols):
                if _is(ci, "pic50") and _is(cj, "hill") and np.isfinite(Wc[i, j]) and (best is None or abs(Wc[i, j]) > abs(best[3])):
                    best = (name, ci, cj, float(Wc[i, j]))
    if best is not None:
        line += "; strongest pIC50-Hill within correlation: {} ({}, {}: {:+.3f})".format(*best)
    return line
