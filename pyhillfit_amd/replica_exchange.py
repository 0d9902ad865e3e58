"""Replica exchange (parallel tempering) between the rungs of PyHillTemp's ladder ("phf_replica_exchange.hip").

A SingleLevelSampler whose Q = P * R problems are P pairs x R rungs, pair-major and in temperature order (as PyHillTemp builds them),
advances in sub-advances that end at multiples of K; after the one that reaches iteration t (t % K == 0) round s = t / K proposes the
adjacent rung pairs (k, k+1) with k = s (mod 2) (deterministic even-odd scheme, Syed, Bouchard-Cote, Deligiannidis & Doucet 2022),
chain c of rung k with chain c of rung k+1, accepted iff log u < (t_k+1 - t_k)(l_k - l_k+1) with the states' untempered
log-likelihoods.  Rounds are numbered by absolute iteration, so a run gives the same bits however it is cut into advance() calls.
The C chain indices stay independent replica sets; what is exchanged is theta and l, the adaptation (mean, covariance, scale) stays
with the rung.  Labels that travel with the states count round trips rung 0 -> R-1 -> 0 per replica set."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import _num
from .sampler import _ptr, _stream_ptr

METHOD = ("replica exchange between adjacent rungs (deterministic even-odd scheme, Syed et al. 2022): after every K iterations round "
          "s = t/K proposes (k, k+1) with k = s mod 2, chain c with chain c; accept iff log u < (t_k+1 - t_k)(l_k - l_k+1)")
# the swap interval K the documentation recommends for PyHillTemp --swap-every (profiles/replica_exchange/results.txt)
RECOMMENDED_EVERY = 2
# label bits (phf_replica_exchange.hip)
REPLICA_MASK = (1 << 28) - 1
SEEN_BOTTOM = 1 << 30
HEADING_DOWN = 1 << 29


def stats_bytes(num_pairs, rungs, chains):
    lib = _lib.load()
    n = lib.phf_replica_exchange_stats_bytes(int(num_pairs), int(rungs), int(chains))
    if n == 0:
        raise ValueError(lib.phf_last_error().decode())
    return int(n)


class ReplicaExchange(object):
    """Swaps between the rungs of `sampler` (a SingleLevelSampler of P pairs x rungs_per_pair rungs).  advance(n, every=K) replaces
    sampler.advance(n); every call of one run must use the same K."""

    def __init__(self, sampler, rungs_per_pair):
        self.lib = _lib.load()
        self.s = sampler
        self.R = int(rungs_per_pair)
        if self.R < 2 or sampler.Q % self.R:
            raise ValueError("the sampler's %d problems are not a whole number of pairs of %d >= 2 rungs" % (sampler.Q, self.R))
        self.P, self.C = sampler.Q // self.R, sampler.C
        t = sampler.temperature.cpu().numpy().reshape(self.P, self.R)
        if np.any(np.diff(t, axis=1) < 0):
            raise ValueError("each pair's rungs must be in increasing temperature order")
        self.device = sampler.device
        self.nbytes = stats_bytes(self.P, self.R, self.C)
        self.stats = torch.empty((self.nbytes + 7) // 8, dtype=torch.int64, device=self.device)
        self.labels = torch.empty(sampler.Q * self.C, dtype=torch.int32, device=self.device)
        self.every = None
        self.rounds = 0
        self.reset_statistics()
        _lib.check(self.lib.phf_replica_exchange_labels_init(self.P, self.R, self.C, _ptr(self.labels), _stream_ptr(self.device)),
                   "phf_replica_exchange_labels_init")

    def reset_statistics(self):
        _lib.check(self.lib.phf_replica_exchange_stats_init(self.P, self.R, self.C, _ptr(self.stats), C.c_size_t(self.nbytes),
                                                            _stream_ptr(self.device)), "phf_replica_exchange_stats_init")
        self.rounds = 0

    def swap_round(self, s, trace=None):
        """round s (>= 1) on the sampler's current state; trace: None or a float64 device tensor [P][R-1][C][3] that receives
        (u, log u, log alpha) of every proposed (pair, rung pair, chain)"""
        if trace is not None and (tuple(trace.shape) != (self.P, self.R - 1, self.C, 3) or trace.dtype != torch.float64
                                  or not trace.is_contiguous()):
            raise ValueError("trace must be a contiguous float64 tensor [%d][%d][%d][3]" % (self.P, self.R - 1, self.C))
        _lib.check(self.lib.phf_replica_exchange_round(C.byref(self.s.prob), self.s.model, self.R, int(s), self.s.seed & (2 ** 64 - 1),
                                                       _ptr(self.s.state), _ptr(self.labels), _ptr(self.stats), C.c_size_t(self.nbytes),
                                                       _ptr(trace), _stream_ptr(self.device)), "phf_replica_exchange_round")
        self.rounds += 1

    def advance(self, n_iterations, every, out=None, save=True):
        """sampler.advance(n_iterations) with a swap round after every iteration t = s K; returns the saved rows [rows][Q][d+1][C]
        (None if save=False)"""
        K = int(every)
        if K < 1:
            raise ValueError("every must be a positive number of iterations")
        if self.every is not None and self.every != K:
            raise ValueError("this run swaps every %d iterations, not %d" % (self.every, K))
        self.every = K
        s = self.s
        t, t_end = s.t, s.t + int(n_iterations)
        rows = None
        if save:
            shape = (s.rows_between(t, t_end), s.Q, s.d + 1, s.C)
            if out is None:
                rows = torch.empty(shape, dtype=torch.float64, device=self.device)
            else:
                if tuple(out.shape) != shape or not out.is_contiguous():
                    raise ValueError("out must be contiguous with shape %s" % (shape,))
                rows = out
        r = 0
        while t < t_end:
            nxt = min((t // K + 1) * K, t_end)
            nr = s.rows_between(t, nxt)
            s.advance(nxt - t, out=rows[r:r + nr] if save else None, save=save)
            r += nr
            t = nxt
            if t % K == 0:
                self.swap_round(t // K)
        return rows

    def statistics(self):
        """dict of numpy int64: attempts [P][R-1], accepts [P][R-1] (rung pair (k, k+1)), round_trips [P][C] (per replica set)"""
        P, R, Cn = self.P, self.R, self.C
        out = torch.empty(2 * P * (R - 1) + P * Cn, dtype=torch.int64, device=self.device)
        _lib.check(self.lib.phf_replica_exchange_stats_read(P, R, Cn, _ptr(self.stats), C.c_size_t(self.nbytes), _ptr(out),
                                                            _stream_ptr(self.device)), "phf_replica_exchange_stats_read")
        v = out.cpu().numpy()
        a = P * (R - 1)
        return {"attempts": v[:a].reshape(P, R - 1), "accepts": v[a:2 * a].reshape(P, R - 1), "round_trips": v[2 * a:].reshape(P, Cn)}

    def replicas(self):
        """numpy int32 [Q][C]: the starting rung of the replica each slot holds now"""
        return (self.labels.cpu().numpy() & REPLICA_MASK).reshape(self.s.Q, self.C)

    def record(self):
        """the JSON object of this sampler's pairs: K, rounds, per pair the accept rate of every adjacent rung pair and the round trips"""
        st = self.statistics()
        pairs = []
        for p in range(self.P):
            att, acc = st["attempts"][p], st["accepts"][p]
            rate = [float(a) / float(n) if n else None for a, n in zip(acc, att)]
            pairs.append({"attempts": att.tolist(), "accepts": acc.tolist(), "accept_rate": rate,
                          "round_trips": int(st["round_trips"][p].sum()), "round_trips_per_replica_set": st["round_trips"][p].tolist()})
        return {"every": self.every, "rounds": self.rounds, "pairs": pairs, "method": METHOD}

    def state_dict(self):
        return {"labels": self.labels.clone(), "stats": self.stats.clone(), "rounds": self.rounds, "every": self.every,
                "rungs_per_pair": self.R}

    def load_state_dict(self, sd):
        if int(sd["rungs_per_pair"]) != self.R or sd["labels"].numel() != self.labels.numel() or sd["stats"].numel() != self.stats.numel():
            raise ValueError("replica-exchange checkpoint of another shape")
        self.labels.copy_(sd["labels"]); self.stats.copy_(sd["stats"])
        self.rounds = int(sd["rounds"]); self.every = sd["every"]


def joint_se(stepping_stone, num_pairs, rungs):
    """se of each pair's stepping-stone log Z over its replica sets (phf_stepping_stone_reduce_joint): numpy [num_pairs]; the
    SteppingStone's problems must be the pairs' rungs, pair-major"""
    st = stepping_stone
    st._check_complete()
    if st.Q != num_pairs * rungs:
        raise ValueError("%d problems are not %d pairs x %d rungs" % (st.Q, num_pairs, rungs))
    from . import stepping_stone as ss
    red = torch.empty((st.Q, len(ss.OUT)), dtype=torch.float64, device=st.device)
    _lib.check(st.lib.phf_stepping_stone_reduce(st.Q, st.C, st.N, _ptr(st.ws), C.c_size_t(st.nbytes), _ptr(red), _stream_ptr(st.device)),
               "phf_stepping_stone_reduce")
    out = torch.empty(num_pairs, dtype=torch.float64, device=st.device)
    _lib.check(st.lib.phf_stepping_stone_reduce_joint(num_pairs, rungs, st.C, st.N, _ptr(st.ws), C.c_size_t(st.nbytes), _ptr(red), _ptr(out),
                                                      _stream_ptr(st.device)), "phf_stepping_stone_reduce_joint")
    return out.cpu().numpy()


def joint_se_numpy(acc, reduced_log_r, num_pairs, rungs):
    """the same from SteppingStone.accumulators() ([Q][C] arrays) and the pooled log r of every rung: the test oracle"""
    m, s1, n = (np.asarray(acc[k], dtype=np.float64) for k in ("m", "s1", "n"))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        lr = np.where((m == -np.inf) & (s1 == 0.0), -np.inf, m + np.log(s1) - np.log(n))
        out = np.empty(num_pairs)
        for p in range(num_pairs):
            u = slice(p * rungs, p * rungs + rungs - 1)
            v = np.exp(lr[u] - np.asarray(reduced_log_r)[u][:, None]).sum(axis=0)
            out[p] = np.std(v, ddof=1) / np.sqrt(v.size) if v.size > 1 else np.nan
    return out


def replica_set_ti_se(ll1, temperatures, num_pairs):
    """se of each pair's pooled TI estimate over the replica sets: ll1 [P*R][C] per-chain <log L(t=1)> (mean_log_likelihood_t1),
    the sd over chains of each chain's trapezium (doseresponse.trapezium_rule), / sqrt(C)"""
    ll1 = np.asarray(ll1, dtype=np.float64)
    t = np.asarray(temperatures, dtype=np.float64)[:, None]
    R = len(t)
    out = np.empty(num_pairs)
    for p in range(num_pairs):
        y = ll1[p * R:(p + 1) * R]
        per_chain = 0.5 * np.sum((t[1:] - t[:-1]) * (y[1:] + y[:-1]), axis=0)
        out[p] = np.std(per_chain, ddof=1) / np.sqrt(per_chain.size) if per_chain.size > 1 else np.nan
    return out


# per-unit columns PyHillTemp gathers under --swap-every (unit = (pair, rung)): the rung's swaps with the next rung, and its pair's
# totals (the same on every rung of the pair)
UNIT_COLUMNS = ("attempts_next", "accepts_next", "round_trips", "rounds", "se_joint", "ti_se_replica_sets")


def unit_columns(stats, rounds, num_pairs, rungs, se_joint=None, ti_se=None):
    """numpy [P*R][len(UNIT_COLUMNS)] in unit order (pair-major, rungs in order)"""
    v = np.zeros((num_pairs * rungs, len(UNIT_COLUMNS)))
    for p in range(num_pairs):
        u = slice(p * rungs, (p + 1) * rungs)
        v[u, 0] = np.append(stats["attempts"][p], 0)
        v[u, 1] = np.append(stats["accepts"][p], 0)
        v[u, 2] = stats["round_trips"][p].sum()
        v[u, 3] = rounds
        v[u, 4] = np.nan if se_joint is None else se_joint[p]
        v[u, 5] = np.nan if ti_se is None else ti_se[p]
    return v


def json_record(unit_values, temperatures, chains, every):
    """one pair's "replica_exchange" object from its R rows of UNIT_COLUMNS"""
    v = np.asarray(unit_values, dtype=np.float64)
    R = len(temperatures)
    att, acc = v[:R - 1, 0], v[:R - 1, 1]
    rate = [float(a / n) if n > 0 else None for a, n in zip(acc, att)]
    known = [(r, k) for k, r in enumerate(rate) if r is not None]
    low = min(known) if known else None
    return {"every": int(every), "rounds": int(v[0, 3]), "accept_rate": rate, "attempts": [int(x) for x in att],
            "accepts": [int(x) for x in acc], "lowest_accept_rate": None if low is None else low[0],
            "lowest_accept_rung_pair": None if low is None else [low[1], low[1] + 1], "round_trips": int(v[0, 2]),
            "round_trips_per_replica_set": float(v[0, 2]) / chains, "chains": int(chains), "method": METHOD}


def report_line(drug, channel, model, rec, temperatures):
    """one line per pair: the lowest accept rate and where it sits, and the round trips per replica set"""
    k = rec["lowest_accept_rung_pair"]
    low = "n/a" if k is None else "{:.3f} between rungs {} and {} (t = {:.4g} and {:.4g})".format(
        rec["lowest_accept_rate"], k[0], k[1], temperatures[k[0]], temperatures[k[1]])
    return ("replica exchange {} + {} model {}: every {} iterations, {} rounds; lowest accept rate {}; round trips per replica set {:.2f}"
            .format(drug, channel, model, rec["every"], rec["rounds"], low, rec["round_trips_per_replica_set"]))
