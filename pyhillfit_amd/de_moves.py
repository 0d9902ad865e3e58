"""Differential-evolution moves between the chains of one pair of the hierarchical sampler (ter Braak 2006, DE-MC; DESIGN.md §3,
"Differential-evolution moves"; pyhillfit_amd/csrc/phf_hier_de.hip, phf_hier_de.h).

The chains of a pair form populations of G consecutive chains by global chain number.  A HierarchicalSampler with moves enabled
(enable_de_moves) advances in sub-advances that end at multiples of K; after the one that reaches iteration t (t % K == 0) round
r = t / K updates every chain once, in two sub-rounds: the chains of one parity within the population move by
x' = x + (sign gamma)(x_a - x_b), a and b two chains of the other parity, accepted iff log u < L(x') - L(x).  Every J-th round uses
gamma = 1 (a jump between modes).  Rounds are numbered by absolute iteration, so a run gives the same bits however it is cut into
advance() calls or continued from a state_dict; nothing of the move is part of the checkpoint but the statistics.

Off by default everywhere.  With moves on, the chains of one population are coupled: R-hat stays a valid check, a standard error from
between-chain spread is optimistic unless it is taken over populations."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .sampler import _ptr, _stream_ptr

METHOD = ("differential-evolution moves within populations of G consecutive chains (ter Braak 2006): after every K iterations each chain "
          "proposes x + (sign gamma)(x_a - x_b) from two chains of the other parity of its population, accepted iff "
          "log u < L(x') - L(x); every J-th round gamma = 1; chains of one population are coupled, populations independent")
POPULATIONS = (4, 8, 16, 32, 64)
DEFAULT_POPULATION = 64
DEFAULT_JUMP_EVERY = 10
# the interval K the documentation names for PyHillFit --hierarchical --de-every: the setting whose effect and cost are measured
# (profiles/de_moves/results.txt — which supports no K as a remedy for the pairs that do not mix)
RECOMMENDED_EVERY = 100
DOMAIN = 0x20000000                  # PHF_DE_DOMAIN: counter word 3 of a move's Philox block is DOMAIN | sub-round


def default_gamma(dim):
    """ter Braak's 2.38 / sqrt(2 dim)"""
    return 2.38 / math.sqrt(2.0 * dim)


def check_settings(every, thinning, population, chains, gamma=None, jump_every=DEFAULT_JUMP_EVERY):
    """ValueError unless the settings describe a run the kernel accepts"""
    if int(every) < 1:
        raise ValueError("the interval K of the differential-evolution moves must be a positive number of iterations")
    if int(every) % int(thinning):
        raise ValueError("the interval K = %d of the differential-evolution moves must be a multiple of the thinning %d" % (every, thinning))
    if int(population) not in POPULATIONS:
        raise ValueError("the population G must be one of %s (got %s)" % (", ".join(str(g) for g in POPULATIONS), population))
    if int(chains) % int(population):
        raise ValueError("the %d chains per pair are not a multiple of the population G = %d" % (chains, population))
    if gamma is not None and not (gamma > 0.0 and math.isfinite(gamma)):
        raise ValueError("gamma must be positive and finite")
    if int(jump_every) < 0:
        raise ValueError("the interval J of the gamma = 1 rounds must be >= 0 (0 = never)")


class DEMoves(object):
    """The moves of one HierarchicalSampler: owns the proposal workspace and the statistics, runs round r on the sampler's state."""

    def __init__(self, sampler, every, population=DEFAULT_POPULATION, gamma=None, jump_every=DEFAULT_JUMP_EVERY):
        s = sampler
        gamma = default_gamma(s.d) if gamma is None else float(gamma)
        check_settings(every, s.thinning, population, s.C, gamma, jump_every)
        self.lib = _lib.load()
        self.s = s
        self.every, self.G, self.gamma, self.jump_every = int(every), int(population), gamma, int(jump_every)
        self.Q, self.C, self.device = s.Q, s.C, s.device
        self.work_bytes = int(self.lib.phf_hier_de_workspace_bytes(s.n_expts, self.Q, self.C))
        self.nbytes = int(self.lib.phf_hier_de_stats_bytes(self.Q, self.C))
        if self.work_bytes == 0 or self.nbytes == 0:
            raise ValueError(self.lib.phf_last_error().decode())
        self.work = torch.empty(self.work_bytes // 8, dtype=torch.float64, device=self.device)
        self.stats = torch.empty(self.nbytes // 8, dtype=torch.int64, device=self.device)
        self.rounds = 0
        self.reset_statistics()

    def reset_statistics(self):
        _lib.check(self.lib.phf_hier_de_stats_init(self.Q, self.C, _ptr(self.stats), C.c_size_t(self.nbytes), _stream_ptr(self.device)),
                   "phf_hier_de_stats_init")
        self.rounds = 0

    def gamma_of(self, r):
        """gamma of round r: 1 in every J-th round"""
        return 1.0 if self.jump_every and r % self.jump_every == 0 else self.gamma

    def round(self, r, trace=None, gamma=None):
        """round r (>= 1) on the sampler's current state, on the current stream; trace: None or a float64 device tensor [Q][C][6] that
        receives (donor chain a, donor chain b, sign gamma, log u, L(x'), accepted) of every chain"""
        if trace is not None and (tuple(trace.shape) != (self.Q, self.C, 6) or trace.dtype != torch.float64 or not trace.is_contiguous()):
            raise ValueError("trace must be a contiguous float64 tensor [%d][%d][6]" % (self.Q, self.C))
        s = self.s
        _lib.check(self.lib.phf_hier_de_round(C.byref(s.points.struct), C.byref(s.prob), C.byref(s.prior), int(r), s.seed & (2 ** 64 - 1),
                                              self.G, float(self.gamma_of(r) if gamma is None else gamma), _ptr(s.state), _ptr(self.work),
                                              C.c_size_t(self.work_bytes), _ptr(self.stats), C.c_size_t(self.nbytes), _ptr(trace),
                                              _stream_ptr(self.device)), "phf_hier_de_round")
        self.rounds += 1

    def statistics(self):
        """dict of numpy int64 [Q]: attempts and accepts of the ordinary rounds, jump_attempts and jump_accepts of the gamma = 1 rounds"""
        out = torch.empty(4 * self.Q, dtype=torch.int64, device=self.device)
        _lib.check(self.lib.phf_hier_de_stats_read(self.Q, self.C, _ptr(self.stats), C.c_size_t(self.nbytes), _ptr(out),
                                                   _stream_ptr(self.device)), "phf_hier_de_stats_read")
        v = out.cpu().numpy().reshape(2, 2, self.Q)
        return {"attempts": v[0, 0], "accepts": v[0, 1], "jump_attempts": v[1, 0], "jump_accepts": v[1, 1]}

    def records(self):
        """the "de_moves" object of every problem of the sampler"""
        st = self.statistics()
        return [json_record(self.every, self.G, self.gamma, self.jump_every, self.rounds, st["attempts"][q], st["accepts"][q],
                            st["jump_attempts"][q], st["jump_accepts"][q]) for q in range(self.Q)]

    def state_dict(self):
        return {"stats": self.stats.clone(), "rounds": self.rounds, "every": self.every, "population": self.G, "gamma": self.gamma,
                "jump_every": self.jump_every}

    def load_state_dict(self, sd):
        if (int(sd["every"]), int(sd["population"]), float(sd["gamma"]), int(sd["jump_every"])) != (self.every, self.G, self.gamma, self.jump_every) \
                or sd["stats"].numel() != self.stats.numel():
            raise ValueError("checkpoint of other differential-evolution settings")
        self.stats.copy_(sd["stats"]); self.rounds = int(sd["rounds"])


def cut_points(t, t_end, every):
    """the ends of the sub-advances of an advance from t to t_end: every multiple of `every` on the way, then t_end"""
    out = []
    while t < t_end:
        t = min((t // every + 1) * every, t_end)
        out.append(t)
    return out


def _rate(acc, att):
    return float(acc) / float(att) if att else None


def json_record(every, population, gamma, jump_every, rounds, attempts, accepts, jump_attempts, jump_accepts):
    return {"every": int(every), "population": int(population), "gamma": float(gamma), "jump_every": int(jump_every), "rounds": int(rounds),
            "attempts": int(attempts), "accepts": int(accepts), "accept_rate": _rate(accepts, attempts),
            "jump_attempts": int(jump_attempts), "jump_accepts": int(jump_accepts), "jump_accept_rate": _rate(jump_accepts, jump_attempts),
            "method": METHOD}


COUPLING_NOTE = ("chains are coupled within populations of {G} consecutive chains (--de-every): R-hat remains a valid check; standard errors "
                 "from between-chain spread (MCSE, se of pooled means) are optimistic unless taken over populations")


def report_line(rank, names, records):
    """one line per rank: the lowest accept rate of the ordinary rounds and its pair"""
    known = [(r["accept_rate"], n) for n, r in zip(names, records) if r["accept_rate"] is not None]
    if not records:
        return "de-moves [rank %d]: no problems" % rank
    r0 = records[0]
    head = "de-moves [rank %d]: every %d iterations, populations of %d, %d rounds" % (rank, r0["every"], r0["population"], r0["rounds"])
    if not known:
        return head + "; no ordinary round yet"
    low = min(known)
    jumps = [r["jump_accept_rate"] for r in records if r["jump_accept_rate"] is not None]
    tail = "" if not jumps else "; lowest accept rate of the gamma = 1 rounds %.4f" % min(jumps)
    return head + "; lowest accept rate %.4f (%s)%s" % (low[0], low[1], tail)
