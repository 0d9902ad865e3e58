"""Stepping-stone evidence of the tempered ladder (Xie, Lewis, Fan, Kuo & Chen 2011, Syst. Biol. 60:150).

The ladder t_0 = 0 < ... < t_R-1 = 1 that PyHillTemp samples gives, besides thermodynamic integration, an unbiased estimate of each
rung ratio r_k = Z(t_k+1) / Z(t_k) = E_t_k[L^Delta_k], Delta_k = t_k+1 - t_k.  With l = log L(theta; t = 1) (the sampler's untempered
log-likelihood, pi_bit included) over chain c's n post-burn-in rows of rung k:

    log r_kc = LSE_j(Delta_k l_kcj) - ln n,     log r_k = LSE_c(log r_kc) - ln C,     se_k = sd_c(r_kc / r_k) / sqrt(C)  (divisor C - 1),
    ESS_k = (sum w)^2 / sum w^2 over all C n draws, w = exp(Delta_k l - max),
    log Z = sum_k<R-1 log r_k,     se = sqrt(sum_k se_k^2),     log B12 = log Z_1 - log Z_2,  se = sqrt(se_1^2 + se_2^2).

The chains are independent, so the spread of their ratios carries the autocorrelation within a chain.  It carries nothing else: se
is the between-chain Monte Carlo error of this run, and a bias every chain shares (draws that do not yet represent a rung's power
posterior, e.g. a region of it no chain has reached) is outside it.  On the G6 setup the pooled estimate misses log Z by far more than
se ("phf_stepping_stone.hip").  The device keeps, per rung and
chain, an online log-sum-exp of the weights and of their squares and the sum of l while the sampler's rows stream past
(phf_stepping_stone_accumulate) and merges the chains in a fixed order (phf_stepping_stone_reduce).  finalize() is the same
arithmetic in numpy on per-chain accumulators (chain_accumulators() builds them from draws): the CPU tests and the chain-file path of
compute_bayes_factors use it."""
import ctypes as C

import numpy as np
import torch

from . import _lib, accumulator
from .sampler import DevicePoints, _ptr, _stream_ptr

FIELDS = ("m", "s1", "s2", "sum_ll", "n")
OUT = ("log_r", "se", "log_r_chain0", "ess", "n", "mean_ll", "nan_chains")
METHOD = ("stepping stone (Xie, Lewis, Fan, Kuo & Chen 2011): log r_k = LSE over chains of [LSE_j(Delta_k l) - ln n] - ln C, l = log L(theta; t=1) "
          "of rung k's post-burn-in rows; se_k = sd over chains of r_kc / r_k / sqrt(C); ESS_k = (sum w)^2 / sum w^2; log Z = sum_k log r_k, "
          "se = sqrt(sum_k se_k^2); ti_minus_ss = trapezium TI (pooled) - log Z")


def deltas(temperatures):
    """Delta_k = t_k+1 - t_k of every rung, 0 for the last (its ratio is 1: log r = 0 exactly)"""
    t = np.asarray(temperatures, dtype=np.float64)
    return np.append(np.diff(t), 0.0)


def workspace_bytes(num_problems, chains, total_rows):
    """device bytes SteppingStone holds: num_problems * 5 * chains doubles (raises on an invalid shape)"""
    return accumulator.workspace_bytes("phf_stepping_stone_workspace_bytes", num_problems, chains, total_rows)


def chain_accumulators(ll, delta):
    """numpy image of the device accumulators: ll [C][n] draws of l per chain -> dict of [C] arrays m, s1, s2, sum_ll, n"""
    ll = np.atleast_2d(np.asarray(ll, dtype=np.float64))
    with np.errstate(invalid="ignore", over="ignore"):
        if delta == 0.0:
            x = np.where(np.isnan(ll), ll, 0.0)
        else:
            x = delta * ll
        m = np.max(np.where(np.isnan(x), -np.inf, x), axis=1)
        fin = np.isfinite(m)
        z = np.where(fin[:, None], x - np.where(fin, m, 0.0)[:, None], -np.inf)
        z = np.where(np.isnan(x), np.nan, z)
        s1, s2 = np.exp(z).sum(axis=1), np.exp(2.0 * z).sum(axis=1)
    return {"m": m, "s1": s1, "s2": s2, "sum_ll": ll.sum(axis=1), "n": np.full(ll.shape[0], float(ll.shape[1]))}


def _lse(v):
    v = np.asarray(v, dtype=np.float64)
    if np.isnan(v).any():
        return np.nan
    mx = np.max(v)
    if mx == -np.inf:
        return -np.inf
    return mx + np.log(np.sum(np.exp(v - mx)))


def finalize(acc):
    """one rung's per-chain accumulators (dict of [C] arrays, FIELDS) -> dict: pooled log r, its se (NaN for one chain), chain 0's
    log r, ESS, rows per chain, mean l over all draws, the per-chain log r and the number of chains whose log r is NaN"""
    m, s1, s2, sl, n = (np.asarray(acc[k], dtype=np.float64) for k in FIELDS)
    Cn = m.size
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        lr_c = np.where((m == -np.inf) & (s1 == 0.0), -np.inf, m + np.log(s1) - np.log(n))
        pooled = _lse(lr_c) - np.log(Cn) if _lse(lr_c) != -np.inf else -np.inf
        se = float(np.std(np.exp(lr_c - pooled), ddof=1) / np.sqrt(Cn)) if Cn > 1 else np.nan
        M = np.max(m)                                     # (sum w)^2 / sum w^2 with both sums relative to the one max
        if np.isnan(s1).any() or np.isnan(s2).any():
            ess = np.nan
        elif M == -np.inf:
            ess = 0.0
        else:
            ess = float(np.sum(s1 * np.exp(m - M)) ** 2 / np.sum(s2 * np.exp(2.0 * (m - M))))
    return {"log_r": float(pooled), "se": se, "log_r_chain0": float(lr_c[0]), "ess": ess, "n": float(n[0]),
            "mean_ll": float(np.sum(sl) / (Cn * n[0])), "nan_chains": float(np.sum(np.isnan(lr_c))), "log_r_chains": lr_c}


class SteppingStone(accumulator.RowAccumulator):
    """Streaming stepping-stone accumulation of Q rungs (problems) over `chains` chains and total_rows post-burn-in rows.
    packed: the sampler's PackedPoints (or DevicePoints); pair_index[q], delta[q]: problem q's row of the points and its Delta.
    accumulate() takes the rows in order, a segment at a time, as views of the sampler's row buffer [rows][Q][>= d+1][chains]
    (asynchronous, on the current stream); reduced() / result() merge the chains."""

    tensors = ("ws", "points")

    def __init__(self, packed, model, pair_index, delta, chains, total_rows, device="cuda"):
        accumulator.RowAccumulator.__init__(self, device)
        if int(model) not in (1, 2):
            raise ValueError("model must be 1 or 2")
        self.model = int(model)
        self.min_cols = self.model + 1
        self.points = packed if isinstance(packed, DevicePoints) else DevicePoints(packed, self.device)
        pi = np.asarray(pair_index, dtype=np.int32)
        dl = np.asarray(delta, dtype=np.float64)
        if pi.shape != dl.shape or pi.ndim != 1:
            raise ValueError("pair_index and delta must be 1-D of one length")
        self.Q, self.C, self.N = len(pi), int(chains), int(total_rows)
        self.pair_index = torch.from_numpy(pi).to(self.device)
        self.delta = torch.from_numpy(dl).to(self.device)
        self._init_workspace(workspace_bytes(self.Q, self.C, self.N), "phf_stepping_stone_init", self.Q, self.C, self.N)

    def _accumulate(self, rows, n):
        _lib.check(self.lib.phf_stepping_stone_accumulate(C.byref(self.points.struct), self.model, _ptr(self.pair_index), _ptr(self.delta),
                                                          _ptr(rows), n, self.Q, rows.shape[2], self.C, self.rows_seen, self.N,
                                                          _ptr(self.ws), C.c_size_t(self.nbytes), _stream_ptr(self.device)),
                   "phf_stepping_stone_accumulate")

    def reduced(self):
        """numpy [Q][7]: the columns of OUT"""
        self._check_complete()
        out = torch.empty((self.Q, len(OUT)), dtype=torch.float64, device=self.device)
        _lib.check(self.lib.phf_stepping_stone_reduce(self.Q, self.C, self.N, _ptr(self.ws), C.c_size_t(self.nbytes), _ptr(out),
                                                      _stream_ptr(self.device)), "phf_stepping_stone_reduce")
        return out.cpu().numpy()

    def accumulators(self):
        """the per-chain accumulators: dict of numpy [Q][C] arrays (FIELDS)"""
        self._check_complete()
        w = self.ws[:self.Q * len(FIELDS) * self.C].view(self.Q, len(FIELDS), self.C).cpu().numpy()
        return {k: w[:, i] for i, k in enumerate(FIELDS)}

    def result(self):
        """one dict per problem (the keys of OUT)"""
        red = self.reduced()
        return [dict(zip(OUT, (float(v) for v in row))) for row in red]


def _num(v):
    if v is None:
        return None
    v = float(v)
    return None if not np.isfinite(v) else v


def _log_num(v):
    """a log-ratio: -inf is a value (zero evidence) JSON cannot hold, written as the string; NaN -> null"""
    v = float(v)
    return "-inf" if v == -np.inf else _num(v)


def rung_record(values, temperature, delta, chains):
    """one rung's "stepping_stone" object from its OUT values"""
    v = dict(zip(OUT, (float(x) for x in values)))
    draws = chains * v["n"]
    return {"t": float(temperature), "delta": float(delta), "log_r": _log_num(v["log_r"]), "se": _num(v["se"]) if chains > 1 else None,
            "log_r_chain0": _log_num(v["log_r_chain0"]), "ess": _num(v["ess"]),
            "ess_fraction": _num(v["ess"] / draws) if draws > 0 else None, "mean_ll": _num(v["mean_ll"]),
            "nan_chains": int(v["nan_chains"]) if np.isfinite(v["nan_chains"]) else None}


def json_record(unit_values, temperatures, chains, ti_pooled):
    """one pair's "stepping_stone" object: unit_values [R][7] (OUT columns) in rung order; ti_pooled: the pair's pooled TI estimate"""
    v = np.asarray(unit_values, dtype=np.float64)
    t = np.asarray(temperatures, dtype=np.float64)
    dl = deltas(t)
    R = len(t)
    lr, se, lr0 = v[:R - 1, 0], v[:R - 1, 1], v[:R - 1, 2]
    log_z = float(np.sum(lr))
    log_z0 = float(np.sum(lr0))
    se_z = float(np.sqrt(np.sum(se ** 2))) if chains > 1 else None
    rungs = [rung_record(v[k], t[k], dl[k], chains) for k in range(R)]
    frac = [r["ess_fraction"] if r["ess_fraction"] is not None else np.nan for r in rungs[:R - 1]]
    worst = int(np.nanargmin(frac)) if R > 1 and not np.all(np.isnan(frac)) else None
    return {"log_z": _log_num(log_z), "se": _num(se_z), "log_z_chain0": _log_num(log_z0),
            "ti_minus_ss": _num(ti_pooled - log_z), "ti_pooled": _num(ti_pooled),
            "nan_rungs": int(np.sum(v[:R - 1, 6] != 0)), "lowest_ess_rung": worst, "chains": int(chains), "rungs": rungs, "method": METHOD}


def report_line(drug, channel, model, rec):
    """one line per pair: log Z_SS +- se (between-chain Monte Carlo error only), TI, the rung with the lowest ESS fraction"""
    se = "n/a" if rec["se"] is None else "{:.4f}".format(rec["se"])
    lz = rec["log_z"] if isinstance(rec["log_z"], str) or rec["log_z"] is None else "{:.4f}".format(rec["log_z"])
    ti = "n/a" if rec["ti_pooled"] is None else "{:.4f}".format(rec["ti_pooled"])
    w = rec["lowest_ess_rung"]
    low = "n/a" if w is None else "rung {} (t = {:g}, ESS fraction {:.3g})".format(w, rec["rungs"][w]["t"], rec["rungs"][w]["ess_fraction"])
    nan = "" if rec["nan_rungs"] == 0 else "; {} rung(s) with NaN log-likelihoods".format(rec["nan_rungs"])
    return ("stepping stone {} + {} model {}: log Z = {} +- {} (se: between-chain Monte Carlo error only, blind to a bias all chains "
            "share) (TI {}); lowest ESS: {}{}".format(drug, channel, model, lz, se, ti, low, nan))
