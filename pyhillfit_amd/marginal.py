"""Integrated (marginal) leave-one-experiment-out cross-validation of the hierarchical model (Merkle, Furr & Rabe-Hesketh 2019;
Vehtari et al. 2016 on hierarchical models).

The conditional pointwise LOO of a hierarchical fit keeps the left-out point's own (Hill_i, pIC50_i) in the condition: it predicts a
new point in an old experiment and its Pareto k is above 0.7 almost everywhere.  Here a WHOLE experiment i is left out and its
(Hill_i, pIC50_i) are integrated out against the population distribution of each draw phi = (alpha, beta, mu, s, sigma):

    m_i(phi) = ln INT INT prod_j TN(y_ij | pred(c_ij; H, P), sigma) loglogistic(H; alpha, beta) logistic(P; mu, s) 1[P >= -2] dH dP

(the density on P is the factor the sampled joint carries, not renormalised for the bound at -2) by a fixed Q x Q tensor rule on the
standard-logistic variables a, b of H = alpha exp(a / beta), P = mu + s b (pyhillfit_amd/csrc/phf_hier_marginal.h): nodes
x_k = -16 + 32 k / Q, weights proportional to the logistic density at the nodes.  g_i = |m_i - m_i of the even-even nodes| is the
rule's own error estimate.  The experiments then are the "points" of the streaming WAIC and PSIS accumulators, fed the m_i as a
"given" log-likelihood:

    elpd_i = ln( sum_s w_s exp(m_i(phi_s)) / sum_s w_s ),  w_s the Pareto-smoothed 1 / exp(m_i(phi_s));   elpd_logo = sum_i elpd_i."""
import ctypes as C

import numpy as np
import torch

from . import _lib, accumulator
from . import loo as loo_mod
from . import waic as waic_mod
from .sampler import _ptr, _stream_ptr

HALF_WIDTH = 16.0                       # L of phf_hier_marginal.h
NODE_CHOICES = (32, 64, 128, 256)
DEFAULT_NODES = 128
DEFAULT_EVERY = 178                     # --marginal-every: measured, the densest thinning whose cost stays within the sampling time
                                        # of a default `--hierarchical -a` Crumb run ("Integrated leave-one-experiment-out")
GAP_WARN = 0.01
MAX_EXPTS = 64
MAX_POINTS = 512                        # points per problem the kernel's LDS slices hold (phf_hier_marginal.hip: kMaxStride)
METHOD = ("integrated leave-one-experiment-out (Merkle, Furr & Rabe-Hesketh 2019): per draw (alpha, beta, mu, s, sigma) the experiment's "
          "(Hill_i, pIC50_i) integrated out against log-logistic(alpha, beta) x logistic(mu, s) on pIC50 >= -2 (not renormalised for the "
          "bound) by a fixed Q x Q rule on the standard-logistic variables, nodes -16 + 32 k / Q, weights proportional to the logistic "
          "density; quadrature_gap_max = max over the draws of |m_i - m_i of the even-even nodes|; PSIS (Vehtari et al. 2024, r_eff = 1) "
          "and WAIC over the experiments' marginal log-likelihoods of every T-th post-burn-in row of all chains")


def log_logistic_density(x):
    """ln lambda(x), lambda(x) = e^-x / (1 + e^-x)^2 (symmetric: written with |x|, no overflow)"""
    ax = np.abs(np.asarray(x, dtype=np.float64))
    return -ax - 2.0 * np.log1p(np.exp(-ax))


def _lse(v):
    m = np.max(v)
    return m + np.log(np.sum(np.exp(v - m)))


def node_table(nodes=DEFAULT_NODES, half_width=HALF_WIDTH):
    """[3][Q] float64: x_k = -L + k h (h = 2 L / Q), ln w_k = ln lambda(x_k) - ln sum lambda, and ln w_k renormalised over the even
    nodes (-inf at odd k, never read there).  Made once, in fp64; the host twin and the kernel read these same doubles."""
    Q = int(nodes)
    if half_width == HALF_WIDTH and Q not in NODE_CHOICES:
        raise ValueError("the number of nodes must be one of %s, got %r" % (NODE_CHOICES, nodes))
    h = 2.0 * half_width / Q
    x = -half_width + np.arange(Q, dtype=np.float64) * h
    ll = log_logistic_density(x)
    t = np.empty((3, Q))
    t[0] = x
    t[1] = ll - _lse(ll)
    t[2] = -np.inf
    t[2, ::2] = ll[::2] - _lse(ll[::2])
    return t


def check_nodes(nodes):
    if int(nodes) not in NODE_CHOICES:
        raise ValueError("--marginal-nodes must be one of %s, got %r" % (", ".join(map(str, NODE_CHOICES)), nodes))
    return int(nodes)


def _check_points(points):
    if points.num_expts is None:
        raise ValueError("the marginal likelihood needs hierarchical points")
    if not 1 <= points.num_expts <= MAX_EXPTS:
        raise ValueError("the number of experiments must be in 1..%d, got %d" % (MAX_EXPTS, points.num_expts))
    if points.stride > MAX_POINTS:
        raise ValueError("the marginal likelihood takes at most %d points per pair, got %d" % (MAX_POINTS, points.stride))


class MarginalLogLik(object):
    """batch evaluator: (m_i, g_i) of every experiment of problem problem_index[v] at the hierarchical vectors theta [m][5 + 2 Ne]"""

    def __init__(self, points, nodes=DEFAULT_NODES, device="cuda"):
        self.lib = _lib.load()
        _check_points(points)
        self.nodes = check_nodes(nodes)
        self.points = points
        self.ne = points.num_expts
        self.dp = waic_mod.DevicePoints(points, device)
        self.device = self.dp.device
        if self.device.type != "cuda":
            raise ValueError("MarginalLogLik runs on a GPU device, not %s" % self.device)
        self.table = torch.from_numpy(node_table(self.nodes)).to(self.device)

    def __call__(self, problem_index, theta):
        """-> (m, g): numpy [m][Ne] each"""
        theta = np.atleast_2d(np.asarray(theta, dtype=np.float64))
        if theta.shape[1] != 5 + 2 * self.ne:
            raise ValueError("theta must have %d columns, got %d" % (5 + 2 * self.ne, theta.shape[1]))
        m = theta.shape[0]
        pi = np.asarray(problem_index, dtype=np.int32).reshape(-1)
        if pi.size != m:
            raise ValueError("problem_index must have one entry per vector")
        th = torch.from_numpy(np.ascontiguousarray(theta.T)).to(self.device)
        pid = torch.from_numpy(pi).to(self.device)
        out = torch.empty((2, m, self.ne), dtype=torch.float64, device=self.device)
        _lib.check(self.lib.phf_hier_marginal_loglik(C.byref(self.dp.struct), self.ne, _ptr(self.table), self.nodes, m, _ptr(pid), _ptr(th),
                                                     _ptr(out), _stream_ptr(self.device)), "phf_hier_marginal_loglik")
        o = out.cpu().numpy()
        return o[0], o[1]


def rows_used(first_row, num_rows, every):
    """the number of global rows r in [first_row, first_row + num_rows) with r mod every == 0"""
    if first_row < 0 or num_rows < 0 or every < 1:
        raise ValueError("first_row and num_rows must be >= 0 and every >= 1")
    end = first_row + num_rows
    return (end + every - 1) // every - (first_row + every - 1) // every


class MarginalRows(object):
    """streams the sampler's rows [n][Q][stride][chains] through the marginal kernel: exactly the global post-burn-in rows r with
    r mod every == 0 are used, however the calls cut the rows; keeps the per-chain running maximum of the gap"""

    def __init__(self, points, num_problems, chains, nodes=DEFAULT_NODES, every=1, device="cuda"):
        self.lib = _lib.load()
        _check_points(points)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("MarginalRows runs on a GPU device, not %s" % self.device)
        if points.num_problems != int(num_problems):
            raise ValueError("the points have %d problems, not %d" % (points.num_problems, num_problems))
        if int(every) < 1:
            raise ValueError("every must be >= 1, got %r" % (every,))
        self.nodes, self.every = check_nodes(nodes), int(every)
        self.points, self.ne = points, points.num_expts
        self.Q, self.C = int(num_problems), int(chains)
        self.dp = waic_mod.DevicePoints(points, self.device)
        self.table = torch.from_numpy(node_table(self.nodes)).to(self.device)
        self.gap_max = torch.zeros((self.Q, self.ne, self.C), dtype=torch.float64, device=self.device)
        self.rows_seen = 0

    def __call__(self, rows):
        """the next n post-burn-in rows -> (loglik, gap): device tensors [used][Q][Ne][chains] of the rows used among them"""
        accumulator.check_rows(rows, self.Q, self.C, 5 + 2 * self.ne, self.device)
        n = rows.shape[0]
        used = rows_used(self.rows_seen, n, self.every)
        ll = torch.empty((used, self.Q, self.ne, self.C), dtype=torch.float64, device=self.device)
        gap = torch.empty_like(ll)
        if used:
            _lib.check(self.lib.phf_hier_marginal_rows(C.byref(self.dp.struct), self.ne, _ptr(self.table), self.nodes, _ptr(rows), n, self.Q,
                                                       rows.shape[2], self.C, self.rows_seen, self.every, _ptr(ll), _ptr(gap),
                                                       _ptr(self.gap_max), _stream_ptr(self.device)), "phf_hier_marginal_rows")
        self.rows_seen += n
        return ll, gap

    def gap_maxima(self):
        """numpy [Q][Ne]: the largest gap over the used rows and all chains (a maximum: the order of the chains cannot matter)"""
        return self.gap_max.amax(dim=2).cpu().numpy()


def experiment_points(points):
    """the "points" of the accumulators: one per experiment, labelled with the experiment's label in the data file"""
    labels = []
    for q in range(points.num_problems):
        seen = {}
        for tag, info in zip(points.tag[q, :points.count[q]], points.info[q]):
            seen.setdefault(int(tag), info[0])
        labels.append([seen.get(e, e + 1) for e in range(points.num_expts)])
    return waic_mod.Points.given(labels)


def workspace_bytes(num_problems, num_expts, chains, total_rows, every, rows_per_call=0):
    """device bytes ExperimentLOO holds: the WAIC and PSIS workspaces over the used rows, the gap maxima, and the two
    [used rows of a call][Q][Ne][chains] buffers of the marginal kernel"""
    used = rows_used(0, int(total_rows), int(every))
    if used * int(chains) < 2:
        raise ValueError("--marginal-every %d leaves %d draws of %d rows x %d chains: too few" % (every, used * chains, total_rows, chains))
    call = rows_used(0, int(rows_per_call), int(every)) + 1 if rows_per_call else used
    return (waic_mod.workspace_bytes(num_problems, num_expts, chains, used) + loo_mod.workspace_bytes(num_problems, num_expts, chains, used)
            + 8 * num_problems * num_expts * chains * (1 + 2 * min(call, used)))


class ExperimentLOO(accumulator.RowAccumulator):
    """Streaming integrated leave-one-experiment-out of num_problems hierarchical problems (all with Ne experiments) over `chains`
    chains and total_rows post-burn-in rows: accumulate() takes the rows in order, a segment at a time, as views of the sampler's row
    buffer; every `every`-th global row goes through the marginal kernel and its [used][Q][Ne][chains] output, the experiments being
    the points and Ne the stride, into the WAIC and PSIS accumulators as a given log-likelihood.  result() reduces and finalizes."""

    def __init__(self, points, num_problems, chains, total_rows, nodes=DEFAULT_NODES, every=DEFAULT_EVERY, device="cuda"):
        self.marginal = MarginalRows(points, num_problems, chains, nodes, every, device)
        accumulator.RowAccumulator.__init__(self, device)
        self.points, self.ne = points, points.num_expts
        self.min_cols = 5 + 2 * self.ne
        self.nodes, self.every = self.marginal.nodes, self.marginal.every
        self.Q, self.C, self.N = int(num_problems), int(chains), int(total_rows)
        self.used = rows_used(0, self.N, self.every)
        if self.used * self.C < 2:
            raise ValueError("--marginal-every %d leaves %d draws of %d rows x %d chains: too few" % (self.every, self.used * self.C, self.N, self.C))
        self.epoints = experiment_points(points)
        self.waic = waic_mod.PointwiseWAIC(self.epoints, "given", self.Q, self.C, self.used, device)
        self.psis = loo_mod.PointwiseLOO(self.epoints, "given", self.Q, self.C, self.used, device)

    def _accumulate(self, rows, n):
        ll, _ = self.marginal(rows)
        if ll.shape[0]:
            self.waic.accumulate(ll)
            self.psis.accumulate(ll)
        return ll

    def result(self):
        """one dict per problem"""
        self._check_complete()
        lse, var = self.waic.reduced()
        r = self.psis.reduced()
        gaps = self.marginal.gap_maxima()
        S = self.used * self.C
        counts = [[int(np.sum(self.points.tag[q, :self.points.count[q]] == e)) for e in range(self.ne)] for q in range(self.Q)]
        return [finalize(r["elpd_loo"][q], r["lppd"][q], r["khat"][q], r["determined"][q], lse[q], var[q], gaps[q], counts[q], S)
                for q in range(self.Q)]

    def free(self):
        self.waic.free()
        self.psis.free()
        self.marginal = None


def finalize(elpd_i, lppd_i, khat_i, determined_i, lse_i, var_i, gap_max_i, n_i, S):
    """one problem's experiments, S draws -> the per-experiment arrays and the totals (NaN if an experiment is not determined)"""
    elpd, lppd, khat = [np.asarray(v, dtype=np.float64) for v in (elpd_i, lppd_i, khat_i)]
    det = np.asarray(determined_i, dtype=np.float64) == 1.0
    gap = np.asarray(gap_max_i, dtype=np.float64)
    S, n = int(S), elpd.size
    thr = loo_mod.khat_threshold(S)
    p_waic = np.asarray(var_i, dtype=np.float64)
    lppd_waic = np.asarray(lse_i, dtype=np.float64) - np.log(S)
    ok = bool(np.all(det))
    tot = float(np.sum(elpd)) if ok else float("nan")
    se = float(np.sqrt(n * np.var(elpd, ddof=1))) if ok and n > 1 and np.all(np.isfinite(elpd)) else float("nan")
    return {"elpd_i": elpd, "lppd_i": lppd, "khat_i": khat, "determined_i": det, "lppd_waic_i": lppd_waic, "p_waic_i": p_waic,
            "elpd_waic_i": lppd_waic - p_waic, "quadrature_gap_max_i": gap, "n_i": [int(v) for v in n_i], "elpd_logo": tot,
            "se_elpd_logo": se, "p_logo": float(np.sum(lppd - elpd)) if ok else float("nan"), "lppd": float(np.sum(lppd)),
            "elpd_waic": float(np.sum(lppd_waic - p_waic)), "n_experiments": int(n), "khat_threshold": thr,
            "n_khat_above_threshold": int(np.sum(khat[det] > thr)), "n_gap_above_0.01": int(np.sum(gap > GAP_WARN)),
            "max_khat": float(np.max(khat[det])) if np.any(det) else float("nan"), "n_undetermined": int(n - np.sum(det)), "draws": S}


def json_record(res, labels, nodes, every):
    """the summary's "loo_experiment" object of one problem (NaN and infinities -> null); labels: the experiments' labels in the data file"""
    num = _lib._num
    rec = {k: (num(res[k]) if isinstance(res[k], float) else res[k]) for k in
           ("elpd_logo", "se_elpd_logo", "p_logo", "lppd", "elpd_waic", "n_experiments", "khat_threshold", "n_khat_above_threshold",
            "n_gap_above_0.01", "max_khat", "n_undetermined", "draws")}
    rec["nodes"], rec["every"] = int(nodes), int(every)
    rec["experiments"] = [{"label": int(labels[e]), "n_i": res["n_i"][e], "elpd_i": num(res["elpd_i"][e]), "lppd_i": num(res["lppd_i"][e]),
                           "khat_i": num(res["khat_i"][e]), "determined": bool(res["determined_i"][e]),
                           "waic": {"lppd_i": num(res["lppd_waic_i"][e]), "p_waic_i": num(res["p_waic_i"][e]),
                                    "elpd_waic_i": num(res["elpd_waic_i"][e])},
                           "quadrature_gap_max": num(res["quadrature_gap_max_i"][e])} for e in range(res["n_experiments"])]
    rec["method"] = METHOD
    return rec


def report_line(rank, names, results, labels=None):
    """one line per rank: the flagged k-hat, and the experiments whose quadrature gap exceeds 0.01, by name"""
    if len(names) == 0:
        return "loo-experiment [rank %d]: no problems" % rank
    flagged = sum(r["n_khat_above_threshold"] for r in results)
    total = sum(r["n_experiments"] for r in results)
    wide = ["{} experiment {}".format(names[q], labels[q][e] if labels is not None else e + 1)
            for q, r in enumerate(results) for e in range(r["n_experiments"]) if r["quadrature_gap_max_i"][e] > GAP_WARN]
    elpd = np.array([r["elpd_logo"] for r in results], dtype=np.float64)
    line = ("loo-experiment [rank {}]: {} problems, {} experiments, {} with k-hat > threshold ({:.2f}) in {} problems; sum of the finite "
            "elpd_logo {:.2f}, {} problems without one"
            .format(rank, len(names), total, flagged, results[0]["khat_threshold"], sum(1 for r in results if r["n_khat_above_threshold"]),
                    float(np.sum(elpd[np.isfinite(elpd)])), int(np.sum(~np.isfinite(elpd)))))
    if wide:
        shown = ", ".join(wide[:8]) + (", ... (%d in all)" % len(wide) if len(wide) > 8 else "")
        line += "; quadrature gap above {} in {}: raise --marginal-nodes".format(GAP_WARN, shown)
    return line
