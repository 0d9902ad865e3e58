"""WAIC and pointwise predictive accuracy of the t = 1 posterior (Watanabe 2010; Vehtari, Gelman & Gabry 2017).

Per data point i, over the S = rows x chains post-burn-in draws theta_s, with l_i(theta) the point's log-likelihood
(include/pyhillfit_amd.h, "pointwise log-likelihood"):

    lppd_i = ln( (1/S) sum_s exp(l_i(theta_s)) ) = LSE_i - ln S,     p_i = var_s l_i(theta_s)  (divisor S - 1),
    elpd_i = lppd_i - p_i,     elpd_waic = sum_i elpd_i,     p_waic = sum_i p_i,     se = sqrt(n var_i(elpd_i)),  WAIC = -2 elpd_waic.

The device keeps, per point and chain, an online log-sum-exp and the sums for the variance while the sampler's rows stream past
(phf_waic_accumulate, one segment at a time: no draw is kept) and merges the chains in a fixed order (phf_waic_reduce); finalize()
does the rest on the host.  Points with p_i > 0.4 are counted: there WAIC's approximation is unreliable (Vehtari et al. 2017).

Points are those of the data file, in its order: single-level fits drop responses outside [0, 100] as the sampler does and
treat y == 0 and y == 100 as censored (a probability MASS); the hierarchical model gives every point a truncated-normal DENSITY.
So single-level and hierarchical elpd differ on the censored points by more than predictive accuracy: compare_models flags them."""
import ctypes as C

import numpy as np
import torch

from . import _lib, accumulator
from ._lib import _num
from .sampler import _ptr, _stream_ptr

P_WARN = 0.4
HIERARCHICAL = 3                        # phf_waic_accumulate's `likelihood` for the hierarchical layout (1 | 2: single-level model)
GIVEN = 4                               # phf_waic_accumulate_given: l of point p is column p of the row (kind "given")
KINDS = ("uncensored", "censored-0", "censored-100")
METHOD = ("WAIC (Watanabe 2010; Vehtari, Gelman & Gabry 2017): lppd_i = log mean_s p(y_i | theta_s), p_waic_i = var_s log p(y_i | theta_s) "
          "(divisor S - 1), elpd_i = lppd_i - p_waic_i, se = sqrt(n var(elpd_i)); per data point over all chains' post-burn-in draws")


class Points(object):
    """Data points of Q problems, one row each, in data-file order: the numpy image of `phf_pointwise_points` plus, per problem, the
    (experiment, dose, response, kind) of every point.  Build with single_level() or hierarchical()."""

    def __init__(self, per_problem, num_expts=None):
        """per_problem: list of lists of (experiment label, dose, response, tag, kind)"""
        self.num_problems = len(per_problem)
        self.num_expts = num_expts
        self.stride = max(1, max(len(p) for p in per_problem)) if per_problem else 1
        self.ln_conc = np.zeros((self.num_problems, self.stride))
        self.response = np.zeros((self.num_problems, self.stride))
        self.tag = np.zeros((self.num_problems, self.stride), dtype=np.int32)
        self.count = np.array([len(p) for p in per_problem], dtype=np.int32)
        self.info = []
        for q, pts in enumerate(per_problem):
            for j, (_, dose, y, tag, _) in enumerate(pts):
                with np.errstate(divide="ignore"):
                    self.ln_conc[q, j] = np.log(dose)
                self.response[q, j] = y
                self.tag[q, j] = tag
            self.info.append([(int(e), float(d), float(y), k) for e, d, y, _, k in pts])

    @classmethod
    def single_level(cls, experiments_per_problem, labels_per_problem=None):
        """experiments_per_problem: per problem, the list of [n_i, 2] (dose, response) arrays the sampler concatenates
        (doseresponse.concatenate_experiments); responses outside [0, 100] are dropped, as the sampler drops them"""
        out = []
        for q, expts in enumerate(experiments_per_problem):
            labels = labels_per_problem[q] if labels_per_problem is not None else range(1, len(expts) + 1)
            pts = []
            for lab, x in zip(labels, expts):
                for dose, y in np.asarray(x, dtype=np.float64):
                    tag = 1 if y == 0 else 2 if y == 100 else 0 if 0 < y < 100 else -1
                    if tag >= 0:
                        pts.append((lab, dose, y, tag, KINDS[tag]))
            out.append(pts)
        return cls(out)

    @classmethod
    def given(cls, labels_per_problem):
        """"points" whose log-likelihood is handed in (kind "given"): one per label, e.g. the experiments of a hierarchical pair"""
        return cls([[(lab, 1.0, 0.0, 0, "given") for lab in labels] for labels in labels_per_problem])

    @classmethod
    def hierarchical(cls, experiments_per_problem, labels_per_problem=None):
        """every problem with the same number Ne of experiments (one launch group); every point, truncated-normal"""
        ne = {len(e) for e in experiments_per_problem}
        if len(ne) != 1:
            raise ValueError("the problems of one hierarchical point set must all have the same number of experiments")
        out = []
        for q, expts in enumerate(experiments_per_problem):
            labels = labels_per_problem[q] if labels_per_problem is not None else range(1, len(expts) + 1)
            out.append([(lab, dose, y, i, "truncated") for i, (lab, x) in enumerate(zip(labels, expts))
                        for dose, y in np.asarray(x, dtype=np.float64)])
        return cls(out, num_expts=ne.pop())


class DevicePoints(object):
    def __init__(self, points, device):
        self.points = points
        self.device = torch.device(device)
        self.ln_conc = torch.from_numpy(points.ln_conc).to(self.device)
        self.response = torch.from_numpy(points.response).to(self.device)
        self.tag = torch.from_numpy(points.tag).to(self.device)
        self.count = torch.from_numpy(points.count).to(self.device)
        self.struct = _lib.PointwisePoints(points.num_problems, points.stride, self.ln_conc.data_ptr(), self.response.data_ptr(),
                                           self.tag.data_ptr(), self.count.data_ptr())


def _likelihood(kind, points):
    if kind in (1, 2):
        if points.num_expts is not None:
            raise ValueError("single-level model %d needs single-level points" % kind)
        return kind, 0
    if kind == "hierarchical":
        if points.num_expts is None:
            raise ValueError("the hierarchical likelihood needs hierarchical points")
        return HIERARCHICAL, points.num_expts
    if kind == "given":
        return GIVEN, 0
    raise ValueError("kind must be 1, 2 (single-level model) or 'hierarchical', got %r" % (kind,))


def columns_read(kind, points):
    lik, ne = _likelihood(kind, points)
    return points.stride if lik == GIVEN else 5 + 2 * ne if lik == HIERARCHICAL else lik + 1


def pointwise_loglik(points, kind, problem_index, theta, device="cuda"):
    """batch evaluator: theta [m][d] (d = model + 1, or 5 + 2 Ne), problem_index [m] -> [m][stride] (NaN beyond a problem's points)"""
    lib = _lib.load()
    lik, ne = _likelihood(kind, points)
    theta = np.atleast_2d(np.asarray(theta, dtype=np.float64))
    if theta.shape[1] != columns_read(kind, points):
        raise ValueError("theta must have %d columns, got %d" % (columns_read(kind, points), theta.shape[1]))
    m = theta.shape[0]
    dp = DevicePoints(points, device)
    th = torch.from_numpy(np.ascontiguousarray(theta.T)).to(dp.device)
    pi = torch.from_numpy(np.asarray(problem_index, dtype=np.int32)).to(dp.device)
    out = torch.empty((m, points.stride), dtype=torch.float64, device=dp.device)
    if lik == HIERARCHICAL:
        rc = lib.phf_pointwise_loglik_hierarchical(C.byref(dp.struct), ne, m, _ptr(pi), _ptr(th), _ptr(out), _stream_ptr(dp.device))
    else:
        rc = lib.phf_pointwise_loglik_single_level(C.byref(dp.struct), lik, m, _ptr(pi), _ptr(th), _ptr(out), _stream_ptr(dp.device))
    _lib.check(rc, "phf_pointwise_loglik")
    return out.cpu().numpy()


def workspace_bytes(num_problems, stride, chains, total_rows):
    """device bytes PointwiseWAIC holds: num_problems * stride * 5 * chains doubles (raises on an invalid shape)"""
    return accumulator.workspace_bytes("phf_waic_workspace_bytes", num_problems, stride, chains, total_rows)


def finalize(lppd_sum_lse, var, S):
    """one problem's points: LSE_i = ln sum_s exp(l_i), var_i (divisor S - 1), S draws -> dict of the pointwise arrays and totals"""
    lse = np.asarray(lppd_sum_lse, dtype=np.float64)
    p = np.asarray(var, dtype=np.float64)
    S = int(S)
    lppd = lse - np.log(S)
    elpd = lppd - p
    n = elpd.size
    se = float(np.sqrt(n * np.var(elpd, ddof=1))) if n > 1 else float("nan")
    return {"lppd_i": lppd, "p_waic_i": p, "elpd_i": elpd, "lppd": float(np.sum(lppd)), "p_waic": float(np.sum(p)),
            "elpd_waic": float(np.sum(elpd)), "se_elpd_waic": se, "waic": -2.0 * float(np.sum(elpd)), "se_waic": 2.0 * se,
            "n_points": int(n), "n_p_waic_above_0.4": int(np.sum(p > P_WARN)), "draws": S}


class PointwiseWAIC(accumulator.RowAccumulator):
    """Streaming WAIC of num_problems problems over `chains` chains and total_rows post-burn-in rows.  accumulate() takes the rows in
    order, a segment at a time, as views of the sampler's row buffer [rows][Q][stride >= columns][chains] (asynchronous, on the
    current stream); result() reduces and finalizes.  kind: 1 | 2 (single-level model), "hierarchical", or "given": column p of a
    row IS the log-likelihood of point p (Points.given)."""

    tensors = ("ws", "dp")

    def __init__(self, points, kind, num_problems, chains, total_rows, device="cuda"):
        accumulator.RowAccumulator.__init__(self, device)
        if points.num_problems != int(num_problems):
            raise ValueError("the points have %d problems, not %d" % (points.num_problems, num_problems))
        self.lik, self.ne = _likelihood(kind, points)
        self.cols = self.min_cols = columns_read(kind, points)
        self.points = points
        self.Q, self.C, self.N = int(num_problems), int(chains), int(total_rows)
        nbytes = workspace_bytes(self.Q, points.stride, self.C, self.N)
        self.dp = DevicePoints(points, self.device)
        self._init_workspace(nbytes, "phf_waic_init", self.Q, points.stride, self.C, self.N)

    def _accumulate(self, rows, n):
        if self.lik == GIVEN:
            _lib.check(self.lib.phf_waic_accumulate_given(C.byref(self.dp.struct), _ptr(rows), n, self.Q, rows.shape[2], self.C, self.rows_seen,
                                                          self.N, _ptr(self.ws), C.c_size_t(self.nbytes), _stream_ptr(self.device)),
                       "phf_waic_accumulate_given")
        else:
            _lib.check(self.lib.phf_waic_accumulate(C.byref(self.dp.struct), self.lik, self.ne, _ptr(rows), n, self.Q, rows.shape[2], self.C,
                                                    self.rows_seen, self.N, _ptr(self.ws), C.c_size_t(self.nbytes), _stream_ptr(self.device)),
                       "phf_waic_accumulate")

    def reduced(self):
        """(LSE, var): numpy [Q][stride] each (meaningless beyond a problem's count)"""
        self._check_complete()
        out = torch.empty((2, self.Q, self.points.stride), dtype=torch.float64, device=self.device)
        _lib.check(self.lib.phf_waic_reduce(self.Q, self.points.stride, self.C, self.N, _ptr(self.ws), C.c_size_t(self.nbytes), _ptr(out),
                                            _stream_ptr(self.device)), "phf_waic_reduce")
        o = out.cpu().numpy()
        return o[0], o[1]

    def result(self):
        """one finalize() dict per problem"""
        lse, var = self.reduced()
        S = self.N * self.C
        return [finalize(lse[q, :n], var[q, :n], S) for q, n in enumerate(self.points.count)]


def waic_of_draws(points, kind, draws, device="cuda"):
    """draws: array [rows][columns][chains] of one problem already in memory (burn-in removed) -> its finalize() dict"""
    x = np.asarray(draws, dtype=np.float64)
    if x.ndim == 2:
        x = x[:, :, None]
    n, cols, c = x.shape
    w = PointwiseWAIC(points, kind, 1, c, n, device)
    w.accumulate(torch.from_numpy(np.ascontiguousarray(x[:, None])).to(w.device))
    return w.result()[0]


def json_record(res, points, q):
    """the summary's "waic" object of problem q (NaN -> null); pointwise arrays in data-file order"""
    rec = {k: (_num(res[k]) if isinstance(res[k], float) else res[k]) for k in
           ("elpd_waic", "se_elpd_waic", "p_waic", "lppd", "waic", "se_waic", "n_points", "n_p_waic_above_0.4", "draws")}
    rec["pointwise"] = {k: [_num(v) for v in res[k + "_i"]] for k in ("elpd", "lppd", "p_waic")}
    rec["points"] = {"experiment": [p[0] for p in points.info[q]], "dose": [p[1] for p in points.info[q]],
                     "response": [p[2] for p in points.info[q]], "kind": [p[3] for p in points.info[q]]}
    rec["method"] = METHOD
    return rec


def report_line(rank, names, results):
    """one line per rank: the number of problems, the worst p_waic warning count, the total elpd"""
    if len(names) == 0:
        return "waic [rank %d]: no problems" % rank
    warn = [r["n_p_waic_above_0.4"] for r in results]
    w = int(np.argmax(warn))
    return ("waic [rank {}]: {} problems, {} with some p_waic_i > {}; sum of elpd_waic {:.2f}; most such points: {} ({})"
            .format(rank, len(names), sum(1 for v in warn if v > 0), P_WARN, sum(r["elpd_waic"] for r in results), names[w], warn[w]))
