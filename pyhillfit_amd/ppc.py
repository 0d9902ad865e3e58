"""Posterior predictive checks of the t = 1 posterior (Gelman et al., BDA3 ch. 6; Gabry et al. 2019): does data replicated from the
fitted model look like the data?

Per problem, over its n data points (waic.Points: the single-level fits drop responses outside [0, 100]) and the S valid draws theta_s
of all chains' post-burn-in rows, one replicate y_rep of every point per draw (include/pyhillfit_amd.h, "posterior predictive checks":
a censored normal for single-level fits, the truncated normal on [0, 100] for the hierarchical model), and five test quantities T,
each of y and of y_rep under the same theta:

    deviance  -2 sum_i l_i(. | theta)       mean     mean of the responses          sd   their sd (divisor n - 1)
    zeros     #{responses == 0}              hundreds #{responses == 100}

    p_T = (#{T(y_rep) > T(y)} + #{T(y_rep) = T(y)} / 2) / S     (the mid-p value; p near 0 or 1 says the model misses T)

and the predictive PIT of every point, u_i = mean_s P(y_rep < y_i | theta_s) + P(y_rep = y_i | theta_s) / 2 (analytic, no replicate),
flagged outside [0.005, 0.995].  The PIT is the POSTERIOR predictive one: the point was used in the fit, so u_i is pulled towards
1/2 (it is not LOO-PIT) and a flagged point is a strong misfit.

The device accumulates while the sampler's rows stream past (phf_ppc_accumulate, one segment at a time: no draw is kept), merges
the chains in a fixed order (phf_ppc_reduce); finalize() does the rest on the host.  A draw with sigma <= 1e-3 is counted as
invalid and left out of S."""
import ctypes as C

import numpy as np
import torch

from . import _lib, accumulator
from ._lib import _num
from . import waic as wc
from .sampler import _ptr, _stream_ptr

STATS = ("deviance", "mean", "sd", "zeros", "hundreds")
HEAD = 4 * len(STATS) + 1               # reduce fields before the per-point PIT sums (include/pyhillfit_amd.h)
P_LO, P_HI = 0.01, 0.99                 # a statistic's p outside [P_LO, P_HI] is reported
PIT_LO, PIT_HI = 0.005, 0.995           # a point's PIT outside [PIT_LO, PIT_HI] is flagged
METHOD = ("posterior predictive check (BDA3 ch. 6): per draw one replicate of every point (single-level: clamp(pred + sigma z, 0, 100); "
          "hierarchical: the truncated normal on [0, 100]); p = (#{T(y_rep) > T(y)} + #{T(y_rep) = T(y)}/2) / S for T = deviance, mean, "
          "sd, zeros, hundreds; pit_i = mean_s P(y_rep < y_i) + P(y_rep = y_i)/2 (posterior-predictive, pulled towards 1/2; not LOO-PIT), "
          "flagged outside [0.005, 0.995]")


def workspace_bytes(num_problems, stride, chains, total_rows):
    """device bytes PosteriorPredictiveCheck holds: num_problems * (21 + stride) * chains doubles (raises on an invalid shape)"""
    return accumulator.workspace_bytes("phf_ppc_workspace_bytes", num_problems, stride, chains, total_rows)


def finalize(sums, n_points, draws):
    """one problem's reduced sums (a row of phf_ppc_reduce's out: [21 + stride]), its number of points and the number of draws
    (rows x chains, the invalid ones included) -> dict of the p values, counts, means and the per-point PIT"""
    v = np.asarray(sums, dtype=np.float64)
    invalid = int(v[HEAD - 1])
    S = int(draws) - invalid
    stats = {}
    for s, name in enumerate(STATS):
        gt, eq, srep, sobs = v[4 * s:4 * s + 4]
        stats[name] = {"p": (gt + 0.5 * eq) / S if S > 0 else float("nan"), "n_greater": int(gt), "n_equal": int(eq),
                       "mean_rep": srep / S if S > 0 else float("nan"), "mean_obs": sobs / S if S > 0 else float("nan")}
    pit = v[HEAD:HEAD + int(n_points)] / S if S > 0 else np.full(int(n_points), np.nan)
    flagged = (pit < PIT_LO) | (pit > PIT_HI)
    extreme = [k for k in STATS if not P_LO <= stats[k]["p"] <= P_HI]
    return {"statistics": stats, "pit": pit, "flagged": flagged, "n_flagged": int(np.sum(flagged)), "extreme": extreme,
            "draws": S, "invalid": invalid, "n_points": int(n_points)}


class PosteriorPredictiveCheck(accumulator.RowAccumulator):
    """Streaming posterior predictive check of num_problems problems over `chains` chains and total_rows post-burn-in rows.
    accumulate() takes the rows in order, a segment at a time, as views of the sampler's row buffer [rows][Q][stride >= columns][chains]
    (asynchronous, on the current stream); result() reduces and finalizes.  kind: 1 | 2 (single-level model) or "hierarchical".
    seed, problem_ids (one per problem) and chain_id_base address the random stream: the replicates of a draw depend on them and
    on the draw's (chain, row) alone."""

    tensors = ("ws", "dp")

    def __init__(self, points, kind, num_problems, chains, total_rows, seed=25, problem_ids=None, chain_id_base=0, device="cuda"):
        accumulator.RowAccumulator.__init__(self, device)
        if points.num_problems != int(num_problems):
            raise ValueError("the points have %d problems, not %d" % (points.num_problems, num_problems))
        self.lik, self.ne = wc._likelihood(kind, points)
        self.cols = self.min_cols = wc.columns_read(kind, points)
        self.points = points
        self.Q, self.C, self.N = int(num_problems), int(chains), int(total_rows)
        self.seed, self.chain_id_base = int(seed) & 0xFFFFFFFFFFFFFFFF, int(chain_id_base) & 0xFFFFFFFF
        ids = np.arange(self.Q) if problem_ids is None else np.asarray(problem_ids, dtype=np.int64)
        if ids.shape != (self.Q,):
            raise ValueError("one problem id per problem: %d expected, got %s" % (self.Q, ids.shape))
        self.problem_ids = ids
        nbytes = workspace_bytes(self.Q, points.stride, self.C, self.N)
        self.dp = wc.DevicePoints(points, self.device)
        self.pid = torch.from_numpy((ids & 0xFFFFFFFF).astype(np.uint32).view(np.int32)).to(self.device)
        self._init_workspace(nbytes, "phf_ppc_init", self.Q, points.stride, self.C, self.N)

    def _accumulate(self, rows, n):
        _lib.check(self.lib.phf_ppc_accumulate(C.byref(self.dp.struct), self.lik, self.ne, _ptr(rows), n, self.Q, rows.shape[2], self.C,
                                               self.rows_seen, self.N, _ptr(self.pid), self.chain_id_base, self.seed, _ptr(self.ws),
                                               C.c_size_t(self.nbytes), _stream_ptr(self.device)), "phf_ppc_accumulate")

    def reduced(self):
        """numpy [Q][21 + stride]: the sums over all chains (include/pyhillfit_amd.h)"""
        self._check_complete()
        out = torch.empty((self.Q, HEAD + self.points.stride), dtype=torch.float64, device=self.device)
        _lib.check(self.lib.phf_ppc_reduce(self.Q, self.points.stride, self.C, self.N, _ptr(self.ws), C.c_size_t(self.nbytes), _ptr(out),
                                           _stream_ptr(self.device)), "phf_ppc_reduce")
        return out.cpu().numpy()

    def result(self):
        """one finalize() dict per problem"""
        red = self.reduced()
        return [finalize(red[q], n, self.N * self.C) for q, n in enumerate(self.points.count)]


def replicate(points, kind, problem_index, theta, counters, seed=25, device="cuda"):
    """batch evaluator: theta [m][d] (d = model + 1, or 5 + 2 Ne), problem_index [m], counters [m][3] = (chain id, problem id, row)
    -> (y_rep [m][stride] (NaN beyond a problem's points), stats [m][2][5]: T(y) then T(y_rep) in the order of STATS)"""
    lib = _lib.load()
    lik, ne = wc._likelihood(kind, points)
    theta = np.atleast_2d(np.asarray(theta, dtype=np.float64))
    if theta.shape[1] != wc.columns_read(kind, points):
        raise ValueError("theta must have %d columns, got %d" % (wc.columns_read(kind, points), theta.shape[1]))
    m = theta.shape[0]
    ctr = np.ascontiguousarray(np.asarray(counters, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint32)
    if ctr.shape != (m, 3):
        raise ValueError("counters must be [%d][3], got %s" % (m, ctr.shape))
    dp = wc.DevicePoints(points, device)
    th = torch.from_numpy(np.ascontiguousarray(theta.T)).to(dp.device)
    pi = torch.from_numpy(np.asarray(problem_index, dtype=np.int32)).to(dp.device)
    ct = torch.from_numpy(ctr.view(np.int32)).to(dp.device)
    y_rep = torch.empty((m, points.stride), dtype=torch.float64, device=dp.device)
    stats = torch.empty((m, 2, len(STATS)), dtype=torch.float64, device=dp.device)
    _lib.check(lib.phf_ppc_replicate(C.byref(dp.struct), lik, ne, m, _ptr(pi), _ptr(th), _ptr(ct), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                     _ptr(y_rep), _ptr(stats), _stream_ptr(dp.device)), "phf_ppc_replicate")
    return y_rep.cpu().numpy(), stats.cpu().numpy()


def ppc_of_draws(points, kind, draws, seed=25, problem_id=0, chain_id_base=0, device="cuda"):
    """draws: array [rows][columns][chains] of one problem already in memory (burn-in removed) -> its finalize() dict"""
    x = np.asarray(draws, dtype=np.float64)
    if x.ndim == 2:
        x = x[:, :, None]
    n, cols, c = x.shape
    p = PosteriorPredictiveCheck(points, kind, 1, c, n, seed, [problem_id], chain_id_base, device)
    p.accumulate(torch.from_numpy(np.ascontiguousarray(x[:, None])).to(p.device))
    return p.result()[0]


def json_record(res, points, q):
    """the summary's "ppc" object of problem q (NaN -> null); per-point arrays in data-file order"""
    info = points.info[q]
    return {"draws": res["draws"], "invalid": res["invalid"], "n_points": res["n_points"],
            "statistics": {k: {f: (_num(v) if isinstance(v, float) else v) for f, v in res["statistics"][k].items()} for k in STATS},
            "extreme_statistics": list(res["extreme"]), "n_flagged": res["n_flagged"],
            "points": {"experiment": [p[0] for p in info], "dose": [p[1] for p in info], "response": [p[2] for p in info],
                       "pit": [_num(v) for v in res["pit"]], "flagged": [bool(f) for f in res["flagged"]]},
            "method": METHOD}


def report_line(rank, names, results):
    """one line per rank: how many problems have some p outside [0.01, 0.99], the most extreme of them, how many points are flagged"""
    if len(names) == 0:
        return "ppc [rank %d]: no problems" % rank
    worst, dist = None, -1.0
    for name, r in zip(names, results):
        for k in STATS:
            p = r["statistics"][k]["p"]
            if np.isfinite(p) and abs(p - 0.5) > dist:
                worst, dist = (name, k, p), abs(p - 0.5)
    bad = sum(1 for r in results if r["extreme"])
    line = "ppc [rank {}]: {} problems, {} with some p outside [{}, {}]".format(rank, len(names), bad, P_LO, P_HI)
    if worst is not None:
        line += "; most extreme: {} ({} p = {:.4g})".format(*worst)
    return line + "; {} of {} points with PIT outside [{}, {}]".format(sum(r["n_flagged"] for r in results), sum(r["n_points"] for r in results),
                                                                  PIT_LO, PIT_HI)
