"""PSIS-LOO: Pareto-smoothed importance-sampling leave-one-out cross-validation of the t = 1 posterior, with Pareto k-hat diagnostics
(Vehtari, Gelman & Gabry 2017; Vehtari, Simpson, Gelman, Yao & Gabry, JMLR 2024; r_eff = 1).

Per data point i, over the S = rows x chains post-burn-in draws with l_s = the point's log-likelihood (the same l as WAIC's,
include/pyhillfit_amd.h, "pointwise log-likelihood") and log ratios r_s = -l_s:

    M = ceil(min(S/5, 3 sqrt S)) largest r (the M smallest l) form the tail, the (M+1)-th smallest l is the cutoff;
    a generalised Pareto fit (Zhang & Stephens 2009) to the tail's exceedances exp(r) - exp(r_cutoff) gives k-hat_i and sigma-hat_i
    (k-hat <- (M k-hat + 5)/(M + 10)); the tail's ratios are replaced by rank with GPD quantiles at (j - 1/2)/M, capped at the largest
    raw ratio; every weight is truncated at S^(3/4) x the mean weight;
    elpd_loo_i = ln sum_s w_s exp(l_s) - ln sum_s w_s,   p_loo_i = lppd_i - elpd_loo_i,
    elpd_loo = sum_i elpd_loo_i,  se = sqrt(n var_i(elpd_loo_i)),  looic = -2 elpd_loo.

k-hat_i above min(1 - 1/log10 S, 0.7) says the estimate of point i is unreliable; above 1, that the ratios have no finite mean.

The device keeps, per point and chain, a bounded heap of the chain's smallest l and online sums of everything else while the sampler's
rows stream past (phf_psis_accumulate: no draw is kept), then selects the exact tail, fits and smooths on the device (phf_psis_reduce);
finalize() does the totals on the host.  By default a heap can hold the whole tail (M + 1 values) while the workspace fits 32 GiB, and every point is exact.  With a
smaller capacity, a point whose tail cannot be proved exact from the kept values (some chain's full heap tops out below the cutoff:
raise --loo-tail-per-chain) is NOT DETERMINED: its fields are null and the problem's elpd_loo is null."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib, accumulator
from .sampler import _ptr, _stream_ptr
from ._lib import _num
from .waic import GIVEN, DevicePoints, _likelihood, columns_read

HIERARCHICAL = 3
METHOD = ("PSIS-LOO (Vehtari, Simpson, Gelman, Yao & Gabry 2024; r_eff = 1): log ratios r = -log p(y_i | theta_s) over all chains' "
          "post-burn-in draws; tail M = ceil(min(S/5, 3 sqrt S)); generalised Pareto fit of Zhang & Stephens (2009) with "
          "k <- (M k + 5)/(M + 10); tail smoothed by rank, capped at the largest raw ratio; weights truncated at S^(3/4) x mean; "
          "elpd_loo_i = log sum w exp(l) - log sum w; se = sqrt(n var(elpd_loo_i))")


def khat_threshold(S):
    """min(1 - 1/log10 S, 0.7): above it, k-hat says S draws are too few for a reliable estimate (Vehtari et al. 2024)"""
    return min(1.0 - 1.0 / math.log10(S), 0.7) if S > 1 else -math.inf


def tail_length(chains, total_rows):
    """M = ceil(min(S/5, 3 sqrt S)) for S = chains x total_rows (raises on an invalid shape)"""
    lib = _lib.load()
    m = lib.phf_psis_tail_length(int(chains), int(total_rows))
    if m == 0:
        raise ValueError(lib.phf_last_error().decode())
    return int(m)


def tail_capacity(num_problems, stride, chains, total_rows, requested=0):
    """the heap capacity per (point, chain) in use, at most min(M + 1, total_rows): `requested`, or with 0 the default — that whole
    cap (every point exact) while the workspace fits 32 GiB, else 2 ceil((M + 1)/chains) + 32"""
    lib = _lib.load()
    k = lib.phf_psis_tail_per_chain(int(num_problems), int(stride), int(chains), int(total_rows), int(requested))
    if k == 0:
        raise ValueError(lib.phf_last_error().decode())
    return int(k)


def workspace_bytes(num_problems, stride, chains, total_rows, tail_per_chain=0):
    """device bytes PointwiseLOO holds (raises on an invalid shape)"""
    return accumulator.workspace_bytes("phf_psis_workspace_bytes", num_problems, stride, chains, total_rows, tail_per_chain)


def finalize(elpd_loo_i, lppd_i, khat_i, sigma_i, determined_i, S):
    """one problem's points (the reduce's fields), S draws -> dict of the pointwise arrays and totals; totals are NaN if any point
    is not determined"""
    elpd = np.asarray(elpd_loo_i, dtype=np.float64)
    lppd = np.asarray(lppd_i, dtype=np.float64)
    khat = np.asarray(khat_i, dtype=np.float64)
    det = np.asarray(determined_i, dtype=np.float64) == 1.0
    S = int(S)
    n = elpd.size
    thr = khat_threshold(S)
    undetermined = int(n - np.sum(det))
    p = lppd - elpd
    if undetermined or n == 0:
        tot = se = p_tot = float("nan")
    else:
        tot, p_tot = float(np.sum(elpd)), float(np.sum(p))
        se = float(np.sqrt(n * np.var(elpd, ddof=1))) if n > 1 and np.all(np.isfinite(elpd)) else float("nan")
    kd = khat[det]
    return {"elpd_loo_i": elpd, "lppd_i": lppd, "p_loo_i": p, "khat_i": khat, "sigma_i": np.asarray(sigma_i, dtype=np.float64),
            "determined_i": det, "elpd_loo": tot, "se_elpd_loo": se, "p_loo": p_tot, "lppd": float(np.sum(lppd)), "looic": -2.0 * tot,
            "se_looic": 2.0 * se, "n_points": int(n), "khat_threshold": thr, "n_khat_above_threshold": int(np.sum(kd > thr)),
            "n_khat_above_1": int(np.sum(kd > 1.0)), "max_khat": float(np.max(kd)) if kd.size else float("nan"),
            "n_undetermined": undetermined, "draws": S}


class PointwiseLOO(accumulator.RowAccumulator):
    """Streaming PSIS-LOO of num_problems problems over `chains` chains and total_rows post-burn-in rows.  accumulate() takes the rows
    in order, a segment at a time, as views of the sampler's row buffer [rows][Q][stride >= columns][chains] (asynchronous, on the
    current stream); result() reduces and finalizes.  kind: 1 | 2 (single-level model), "hierarchical" or "given" (waic.Points.given:
    column p of a row is the log-likelihood of point p); tail_per_chain: the heap
    capacity per (point, chain), 0 for the default rule."""

    tensors = ("ws", "dp")

    def __init__(self, points, kind, num_problems, chains, total_rows, device="cuda", tail_per_chain=0):
        accumulator.RowAccumulator.__init__(self, device)
        if points.num_problems != int(num_problems):
            raise ValueError("the points have %d problems, not %d" % (points.num_problems, num_problems))
        self.lik, self.ne = _likelihood(kind, points)
        self.cols = self.min_cols = columns_read(kind, points)
        self.points = points
        self.Q, self.C, self.N = int(num_problems), int(chains), int(total_rows)
        self.requested = int(tail_per_chain)
        nbytes = workspace_bytes(self.Q, points.stride, self.C, self.N, self.requested)
        self.M = tail_length(self.C, self.N)
        self.k = tail_capacity(self.Q, points.stride, self.C, self.N, self.requested)
        self.dp = DevicePoints(points, self.device)
        self._init_workspace(nbytes, "phf_psis_init", self.Q, points.stride, self.C, self.N, self.requested)

    def _accumulate(self, rows, n):
        if self.lik == GIVEN:
            _lib.check(self.lib.phf_psis_accumulate_given(C.byref(self.dp.struct), _ptr(rows), n, self.Q, rows.shape[2], self.C, self.rows_seen,
                                                          self.N, self.requested, _ptr(self.ws), C.c_size_t(self.nbytes),
                                                          _stream_ptr(self.device)), "phf_psis_accumulate_given")
        else:
            _lib.check(self.lib.phf_psis_accumulate(C.byref(self.dp.struct), self.lik, self.ne, _ptr(rows), n, self.Q, rows.shape[2], self.C,
                                                    self.rows_seen, self.N, self.requested, _ptr(self.ws), C.c_size_t(self.nbytes),
                                                    _stream_ptr(self.device)), "phf_psis_accumulate")

    def reduced(self, tail=False):
        """dict of numpy [Q][stride] arrays elpd_loo, lppd, khat, sigma, determined (NaN / 0 beyond a problem's count); with tail=True
        also "tail": [Q][stride][M + 1], the M + 1 smallest log-likelihoods of every point, ascending"""
        self._check_complete()
        ps = self.points.stride
        out = torch.empty((5, self.Q, ps), dtype=torch.float64, device=self.device)
        t = torch.empty((self.Q, ps, self.M + 1), dtype=torch.float64, device=self.device) if tail else None
        _lib.check(self.lib.phf_psis_reduce(C.byref(self.dp.struct), self.Q, self.C, self.N, self.requested, _ptr(self.ws),
                                            C.c_size_t(self.nbytes), _ptr(out), _ptr(t) if tail else None, _stream_ptr(self.device)),
                   "phf_psis_reduce")
        o = out.cpu().numpy()
        res = {k: o[i] for i, k in enumerate(("elpd_loo", "lppd", "khat", "sigma", "determined"))}
        if tail:
            res["tail"] = t.cpu().numpy()
        return res

    def insertions(self):
        """heap insertions so far (fill-ups and evictions), numpy [Q][stride][chains] (meaningless beyond a problem's count)"""
        f = self.ws[: self.Q * self.points.stride * 6 * self.C].view(self.Q, self.points.stride, 6, self.C)
        return f[:, :, 5].cpu().numpy()

    def result(self):
        """one finalize() dict per problem"""
        r = self.reduced()
        ins = self.insertions()
        S = self.N * self.C
        out = []
        for q, n in enumerate(self.points.count):
            res = finalize(r["elpd_loo"][q, :n], r["lppd"][q, :n], r["khat"][q, :n], r["sigma"][q, :n], r["determined"][q, :n], S)
            res["insertions_per_draw"] = float(ins[q, :n].sum() / max(1, n * S))
            out.append(res)
        return out


def loo_of_draws(points, kind, draws, device="cuda", tail_per_chain=0):
    """draws: array [rows][columns][chains] of one problem already in memory (burn-in removed) -> its finalize() dict"""
    x = np.asarray(draws, dtype=np.float64)
    if x.ndim == 2:
        x = x[:, :, None]
    n, cols, c = x.shape
    w = PointwiseLOO(points, kind, 1, c, n, device, tail_per_chain)
    w.accumulate(torch.from_numpy(np.ascontiguousarray(x[:, None])).to(w.device))
    res = w.result()[0]
    res["tail_length"], res["tail_per_chain"] = w.M, w.k
    return res


def json_record(res, points, q, tail_length=None, tail_per_chain=None):
    """the summary's "loo" object of problem q (NaN and infinities -> null); pointwise arrays in data-file order"""
    rec = {k: (_num(res[k]) if isinstance(res[k], float) else res[k]) for k in
           ("elpd_loo", "se_elpd_loo", "p_loo", "lppd", "looic", "se_looic", "n_points", "khat_threshold", "n_khat_above_threshold",
            "n_khat_above_1", "max_khat", "n_undetermined", "draws")}
    if tail_length is not None:
        rec["tail_length"], rec["tail_per_chain"] = int(tail_length), int(tail_per_chain)
    if "insertions_per_draw" in res:
        rec["insertions_per_draw"] = res["insertions_per_draw"]
    rec["pointwise"] = {k: [_num(v) for v in res[k + "_i"]] for k in ("elpd_loo", "lppd", "p_loo", "khat", "sigma")}
    rec["pointwise"]["determined"] = [bool(v) for v in res["determined_i"]]
    rec["points"] = {"experiment": [p[0] for p in points.info[q]], "dose": [p[1] for p in points.info[q]],
                     "response": [p[2] for p in points.info[q]], "kind": [p[3] for p in points.info[q]]}
    rec["method"] = METHOD
    return rec


def report_line(rank, names, results):
    """one line per rank: problems with some k-hat above the threshold, the worst k-hat, the undetermined points"""
    if len(names) == 0:
        return "loo [rank %d]: no problems" % rank
    flagged = sum(1 for r in results if r["n_khat_above_threshold"] > 0)
    worst = [-np.inf if np.isnan(r["max_khat"]) else r["max_khat"] for r in results]
    w = int(np.argmax(worst))
    und = [r["n_undetermined"] for r in results]
    return ("loo [rank {}]: {} problems, {} with some k-hat > threshold ({:.2f}); worst k-hat {:.3f} ({}); {} undetermined points in "
            "{} problems".format(rank, len(names), flagged, results[0]["khat_threshold"], worst[w], names[w], sum(und),
                                 sum(1 for u in und if u)))
