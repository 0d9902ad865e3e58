"""Power-scaling sensitivity of prior and likelihood (Kallioinen, Paananen, Buerkner & Vehtari 2023; the method of R's priorsense).

Power-scaling a component c(theta) of the log-target by alpha gives p_alpha(theta) ~ p(theta | y) exp((alpha - 1) c(theta)); the draws
of the fit are re-weighted, never re-sampled.  The components are the log-prior and the log-likelihood (single-level: phf_sl_log_prior
and the untempered log-likelihood; hierarchical: the five Gamma hyper-priors and the truncated-normal data term, the population terms
belonging to neither; "given": two named columns of the rows), the directions alpha = 1/(1 + delta) and 1 + delta.

While the post-burn-in rows stream past the device keeps, per (problem, column) and on the quantiles' grid, the base counts and the
four weighted integer masses, and per chain the weights' and the columns' sums (csrc/phf_sensitivity.hip; no draw is kept).  Its
reduce returns per-slot scalars: the sums of the cumulative Jensen-Shannon divergence on the CDF and on the survival function.  Here:

    h = numerator / denominator,   CJS = sqrt(max(h(CDF), h(survival), 0)),   D = (CJS(down) + CJS(up)) / (2 log2(1 + delta))

and the weighted-mean shift in units of the base sd, the sd ratio, the between-chain standard error of the shift, the weights' ESS
fraction (sum w)^2 / (n sum w^2), and a diagnosis per column at a threshold on D (0.05, priorsense's default).  Not done: Pareto
smoothing of the weights (delta is bounded and the ESS fraction reported instead), per-hyper-prior components, derived quantities."""
import ctypes as C

import numpy as np

from . import _lib, accumulator
from ._lib import _num

DEFAULT_DELTA = 0.01
DEFAULT_BINS = 4096
DEFAULT_THRESHOLD = 0.05
MAX_DELTA = 0.25
MIN_BINS, MAX_BINS = 64, 4096
KINDS = {1: 1, 2: 2, "hierarchical": 3, "given": 4}
COMPONENTS = ("prior", "likelihood")
DIRECTIONS = ("down", "up")
SLOT_HEAD, PER_WEIGHT = 8, 5
MASS_ONE = 2.0 ** 20
CLAMP = 8.0
DIAGNOSES = ("prior-data conflict", "prior-dominated (weak likelihood)", "likelihood-dominated", "none")
METHOD = ("power-scaling sensitivity (Kallioinen et al. 2023): every post-burn-in draw of every chain re-weighted by exp((alpha - 1)(c - c_ref)) "
          "for c = log-prior | log-likelihood and alpha = 1/(1 + delta) | 1 + delta (exponent clamped to [-8, 8], no Pareto smoothing); D = the "
          "mean of the two directions' cumulative Jensen-Shannon distances (the larger of CDF and survival form) between the base and the "
          "weighted histogram of B bins, divided by log2(1 + delta)")


def check_delta(delta):
    d = float(delta)
    if not (0.0 < d <= MAX_DELTA):
        raise ValueError("--sensitivity-delta must satisfy 0 < delta <= %g, got %r" % (MAX_DELTA, delta))
    return d


def check_bins(bins):
    b = int(bins)
    if b < MIN_BINS or b > MAX_BINS or b & (b - 1):
        raise ValueError("--sensitivity-bins must be a power of two in [%d, %d], got %d" % (MIN_BINS, MAX_BINS, b))
    return b


def check_threshold(t):
    t = float(t)
    if not (t > 0.0 and np.isfinite(t)):
        raise ValueError("--sensitivity-threshold must be positive, got %r" % (t,))
    return t


def workspace_bytes(num_problems, columns, chains, total_rows, bins=DEFAULT_BINS):
    """device bytes PowerScaling holds (raises on an invalid shape)"""
    return accumulator.workspace_bytes("phf_sensitivity_workspace_bytes", num_problems, columns, chains, total_rows, bins)


class PowerScaling(accumulator.RowAccumulator):
    """Streaming power-scaling sensitivity of num_problems x columns over `chains` chains and total_rows post-burn-in rows.
    points: the sampler's device points (sampler.DevicePoints for kind 1 | 2, hierarchical.DeviceHierPoints — with prior, a
    hierarchical.HierPrior — for kind "hierarchical"), problem q <-> pair q; kind "given": None, and given = (prior column, likelihood
    column) of the rows.  accumulate() takes the rows in order, a segment at a time, as views of the sampler's row buffer
    [rows][Q][stride][chains] (asynchronous, on the current stream); result() reduces and finalizes."""

    def __init__(self, points, kind, num_problems, chains, columns, total_rows, delta=DEFAULT_DELTA, bins=DEFAULT_BINS, device="cuda",
                 prior=None, given=None, threshold=DEFAULT_THRESHOLD):
        from .sampler import _ptr, _stream_ptr
        self._ptr, self._stream_ptr = _ptr, _stream_ptr
        accumulator.RowAccumulator.__init__(self, device)
        if kind not in KINDS:
            raise ValueError("kind must be 1, 2, 'hierarchical' or 'given', got %r" % (kind,))
        self.kind, self.code = kind, KINDS[kind]
        self.Q, self.C, self.cols, self.N = int(num_problems), int(chains), int(columns), int(total_rows)
        self.delta, self.B, self.threshold = check_delta(delta), check_bins(bins), check_threshold(threshold)
        self.points, self.prior = points, prior
        self.given = (0, 0)
        if kind == "given":
            if given is None or len(given) != 2:
                raise ValueError("kind 'given' needs given = (prior column, likelihood column)")
            self.given = (int(given[0]), int(given[1]))
        elif points is None or (kind == "hierarchical" and prior is None):
            raise ValueError("kind %r needs the model's points%s" % (kind, " and prior" if kind == "hierarchical" else ""))
        self.min_cols = self.cols
        self._init_workspace(workspace_bytes(self.Q, self.cols, self.C, self.N, self.B), "phf_sensitivity_init", self.Q, self.cols, self.C,
                             self.N, self.B)

    def _struct_ptrs(self):
        sl = C.addressof(self.points.struct) if self.code in (1, 2) else None
        hp = C.addressof(self.points.struct) if self.code == 3 else None
        pr = C.addressof(self.prior) if self.code == 3 else None
        return sl, hp, pr

    def _accumulate(self, rows, n):
        sl, hp, pr = self._struct_ptrs()
        _lib.check(self.lib.phf_sensitivity_accumulate(self.code, sl, hp, pr, self.given[0], self.given[1], self._ptr(rows), n, self.Q,
                                                       rows.shape[2], self.C, self.cols, self.delta, self.B, self.rows_seen, self.N,
                                                       self._ptr(self.ws), C.c_size_t(self.nbytes), self._stream_ptr(self.device)),
                   "phf_sensitivity_accumulate")

    def counts(self):
        """the histograms: numpy uint64 [Q][columns][5][B] (base, prior down, prior up, likelihood down, likelihood up)"""
        import torch
        n = self.Q * self.cols * 5 * self.B
        return self.ws.view(torch.int64)[:n].cpu().numpy().view(np.uint64).reshape(self.Q, self.cols, 5, self.B)

    def reduced(self, per_chain=False):
        """the device's reduce: slots [Q][columns][28], weights [Q][4][4], columns [Q][columns][5][4] (include/pyhillfit_amd.h) and,
        with per_chain, the per-chain sums: weights [Q][4][4][chains], columns [Q][columns][5][3][chains]"""
        import torch
        S = self.Q * self.cols
        slots = torch.empty((S, SLOT_HEAD + 4 * PER_WEIGHT), dtype=torch.float64, device=self.device)
        weights = torch.empty((self.Q, 4, 4), dtype=torch.float64, device=self.device)
        cols = torch.empty((S, 5, 4), dtype=torch.float64, device=self.device)
        nw = self.Q * 16 * self.C
        pc = torch.empty(nw + S * 15 * self.C, dtype=torch.float64, device=self.device) if per_chain else None
        _lib.check(self.lib.phf_sensitivity_reduce(self.Q, self.cols, self.C, self.N, self.B, self._ptr(self.ws), C.c_size_t(self.nbytes),
                                                   self._ptr(slots), self._ptr(weights), self._ptr(cols),
                                                   self._ptr(pc) if per_chain else None, self._stream_ptr(self.device)),
                   "phf_sensitivity_reduce")
        out = (slots.cpu().numpy().reshape(self.Q, self.cols, -1), weights.cpu().numpy(), cols.cpu().numpy().reshape(self.Q, self.cols, 5, 4))
        if per_chain:
            p = pc.cpu().numpy()
            out += (p[:nw].reshape(self.Q, 4, 4, self.C), p[nw:].reshape(self.Q, self.cols, 5, 3, self.C))
        return out

    def result(self):
        slots, weights, cols = self.reduced()
        return finalize(slots, weights, cols, self.delta, self.threshold, self.rows_seen * self.C, self.B)


def components(points, kind, problem_index, theta, prior=None, device="cuda"):
    """(prior, likelihood, population term) [3][m] of m parameter vectors theta [m][d] of the problems problem_index [m], on the GPU
    (phf_sensitivity_components); kind 1 | 2 | "hierarchical" and points as for PowerScaling"""
    import torch
    from .sampler import _ptr, _stream_ptr
    lib = _lib.load()
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError("components runs on a GPU device, not %s" % dev)
    code = KINDS[kind]
    th = np.ascontiguousarray(np.asarray(theta, dtype=np.float64).T)
    m = th.shape[1]
    t_th = torch.from_numpy(th).to(dev)
    t_pi = torch.from_numpy(np.ascontiguousarray(problem_index, dtype=np.int32)).to(dev)
    out = torch.empty((3, m), dtype=torch.float64, device=dev)
    sl = C.addressof(points.struct) if code in (1, 2) else None
    hp = C.addressof(points.struct) if code == 3 else None
    pr = C.addressof(prior) if code == 3 else None
    _lib.check(lib.phf_sensitivity_components(code, sl, hp, pr, m, _ptr(t_pi), _ptr(t_th), _ptr(out), _stream_ptr(dev)),
               "phf_sensitivity_components")
    return out.cpu().numpy()


# ---- finalize (host, numpy) ----------------------------------------------------------------------------------------------------------
def cjs_from_sums(num_c, den_c, num_s, den_s):
    """CJS = sqrt(max(h on the CDF, h on the survival function, 0)), h = numerator / denominator (0 where the denominator is 0)"""
    num_c, den_c, num_s, den_s = (np.asarray(v, dtype=np.float64) for v in (num_c, den_c, num_s, den_s))
    with np.errstate(divide="ignore", invalid="ignore"):
        hc = np.where(den_c > 0, num_c / den_c, 0.0)
        hs = np.where(den_s > 0, num_s / den_s, 0.0)
    return np.sqrt(np.maximum(np.maximum(hc, hs), 0.0))


def _h(P, Q):
    with np.errstate(divide="ignore", invalid="ignore"):
        s = P + Q
        a = np.where(P > 0, P * np.log2(2.0 * P / s), 0.0)
        b = np.where(Q > 0, Q * np.log2(2.0 * Q / s), 0.0)
    den = np.sum(s)
    return (np.sum(a) + np.sum(b)) / den if den > 0 else 0.0


def cjs_numpy(base, mass):
    """numpy restatement of the cumulative Jensen-Shannon distance of a base histogram against a weighted one (the same bins): over
    the bins from the first to the last one holding a base draw; returns (CJS, h on the CDF, h on the survival function)"""
    base = np.asarray(base, dtype=np.float64)
    mass = np.asarray(mass, dtype=np.float64)
    nz = np.flatnonzero(base)
    if nz.size == 0 or mass.sum() == 0:
        return 0.0, 0.0, 0.0
    sl = slice(nz[0], nz[-1] + 1)
    P = np.cumsum(base[sl]) / base.sum()
    Q = np.cumsum(mass[sl]) / mass.sum()
    hc, hs = _h(P, Q), _h(1.0 - P, 1.0 - Q)
    return float(np.sqrt(max(hc, hs, 0.0))), hc, hs


def sensitivity_d(cjs_down, cjs_up, delta):
    return (np.asarray(cjs_down) + np.asarray(cjs_up)) / (2.0 * np.log2(1.0 + delta))


def diagnose(d_prior, d_lik, threshold=DEFAULT_THRESHOLD):
    p, l = d_prior > threshold, d_lik > threshold
    return DIAGNOSES[0] if p and l else DIAGNOSES[1] if p else DIAGNOSES[2] if l else DIAGNOSES[3]


def finalize(slots, weights, cols, delta, threshold=DEFAULT_THRESHOLD, draws=None, bins=None):
    """the device's reduce -> dict of numpy arrays.  Over [Q][columns][2 components]: D; over [Q][columns][2][2 directions]: cjs,
    mean_shift (units of the base sd), sd_ratio, mean_shift_se; over [Q][2][2]: ess_fraction, clamped; over [Q][2]: non_finite;
    over [Q][columns]: base_mean, base_sd, draws, non_finite_values, diagnosis"""
    slots, weights, cols = np.asarray(slots), np.asarray(weights), np.asarray(cols)
    Qn, nc = slots.shape[0], slots.shape[1]
    per = slots[..., SLOT_HEAD:].reshape(Qn, nc, 2, 2, PER_WEIGHT)
    cjs = cjs_from_sums(per[..., 0], per[..., 1], per[..., 2], per[..., 3])
    D = sensitivity_d(cjs[..., 0], cjs[..., 1], delta)
    anchor = slots[..., 6]
    with np.errstate(divide="ignore", invalid="ignore"):
        n0, sd0, sdd0 = cols[:, :, 0, 0], cols[:, :, 0, 1], cols[:, :, 0, 2]
        mb = sd0 / n0
        sb = np.sqrt(np.maximum(sdd0 / n0 - mb * mb, 0.0))
        w = cols[:, :, 1:, 0].reshape(Qn, nc, 2, 2)
        mw = cols[:, :, 1:, 1].reshape(Qn, nc, 2, 2) / w
        sw = np.sqrt(np.maximum(cols[:, :, 1:, 2].reshape(Qn, nc, 2, 2) / w - mw * mw, 0.0))
        shift = (mw - mb[..., None, None]) / sb[..., None, None]
        ratio = sw / sb[..., None, None]
        se = cols[:, :, 1:, 3].reshape(Qn, nc, 2, 2) / sb[..., None, None]
        wq = weights.reshape(Qn, 2, 2, 4)
        ess = wq[..., 1] ** 2 / (wq[..., 0] * wq[..., 2])
    res = {"D": D, "cjs": cjs, "mean_shift": shift, "sd_ratio": ratio, "mean_shift_se": se, "ess_fraction": ess,
           "clamped": wq[..., 3], "entered": wq[..., 0, 0], "base_mean": anchor + mb, "base_sd": sb, "draws": slots[..., 2],
           "non_finite_values": slots[..., 3], "delta": float(delta), "threshold": float(threshold), "bins": bins,
           "diagnosis": np.array([[diagnose(D[q, c, 0], D[q, c, 1], threshold) for c in range(nc)] for q in range(Qn)], dtype=object)}
    res["non_finite"] = (float(draws) - wq[..., 0, 0]) if draws is not None else np.full((Qn, 2), np.nan)
    return res


def json_record(res, q, columns):
    """the command lines' "sensitivity" object of problem q: per column name the two components' D, CJS, mean shift, sd ratio and the
    shift's between-chain standard error (each [down, up]) and the diagnosis; the weights' ESS fraction, clamped and non-finite counts"""
    rec = {"delta": res["delta"], "bins": res["bins"], "threshold": res["threshold"], "method": METHOD, "columns": {}, "weights": {}}
    for c, name in enumerate(columns):
        col = {"diagnosis": str(res["diagnosis"][q, c]), "draws": int(res["draws"][q, c]), "non_finite": int(res["non_finite_values"][q, c])}
        for k, comp in enumerate(COMPONENTS):
            col[comp] = {"D": _num(res["D"][q, c, k]), "cjs": [_num(v) for v in res["cjs"][q, c, k]],
                         "mean_shift": [_num(v) for v in res["mean_shift"][q, c, k]],
                         "sd_ratio": [_num(v) for v in res["sd_ratio"][q, c, k]],
                         "mean_shift_se": [_num(v) for v in res["mean_shift_se"][q, c, k]]}
        rec["columns"][name] = col
    for k, comp in enumerate(COMPONENTS):
        nf = res["non_finite"][q, k]
        rec["weights"][comp] = {"ess_fraction": [_num(v) for v in res["ess_fraction"][q, k]],
                                "clamped": [int(v) for v in res["clamped"][q, k]],
                                "non_finite": int(nf) if np.isfinite(nf) else None}
    flagged = [n for c, n in enumerate(columns) if res["diagnosis"][q, c] != DIAGNOSES[3]]
    rec["flagged_columns"] = flagged
    return rec


def summarise(parts):
    """parts: per problem (diagnosis [columns], D [columns][2], ess_fraction [2][2], clamped [2][2]) -> counts for the report"""
    pairs = {d: 0 for d in DIAGNOSES[:3]}
    cols = {d: 0 for d in DIAGNOSES[:3]}
    worst, low, clamped = 0.0, np.inf, 0
    for diag, D, ess, cl in parts:
        seen = set()
        for d in diag:
            if d != DIAGNOSES[3]:
                cols[d] += 1
                seen.add(d)
        for d in seen:
            pairs[d] += 1
        Df = np.asarray(D, dtype=np.float64)
        if np.any(np.isfinite(Df)):
            worst = max(worst, float(np.nanmax(Df)))
        e = np.asarray(ess, dtype=np.float64)
        if np.any(np.isfinite(e)):
            low = min(low, float(np.nanmin(e)))
        clamped += int(np.nansum(cl))
    return {"pairs": pairs, "columns": cols, "worst_D": worst, "lowest_ess_fraction": low if np.isfinite(low) else None, "clamped": clamped}


def report_line(rank, names, parts):
    """one line per rank: how many pairs have a flagged column, by diagnosis, and the worst D"""
    if len(names) == 0:
        return "sensitivity [rank %d]: no problems" % rank
    s = summarise(parts)
    flagged = "; ".join("{} pairs ({} columns) {}".format(s["pairs"][d], s["columns"][d], d) for d in DIAGNOSES[:3])
    return "sensitivity [rank {}]: {} pairs; {}; worst D {:.3g}; lowest ESS fraction {}; {} clamped draws".format(
        rank, len(names), flagged, s["worst_D"], "n/a" if s["lowest_ess_fraction"] is None else "%.3f" % s["lowest_ess_fraction"], s["clamped"])


def part_of(res, q):
    return (list(res["diagnosis"][q]), res["D"][q], res["ess_fraction"][q], res["clamped"][q])


def sensitivity_of_draws(points, kind, draws, delta=DEFAULT_DELTA, bins=DEFAULT_BINS, threshold=DEFAULT_THRESHOLD, device="cuda",
                         prior=None, given=None, columns=None):
    """draws: array [rows][cols][chains] already in memory (burn-in removed) of ONE problem -> result() of it; columns: how many
    leading columns are parameters (default: all the model reads)"""
    import torch
    x = np.ascontiguousarray(np.asarray(draws, dtype=np.float64)[:, None])
    n, _, stride, c = x.shape
    ps = PowerScaling(points, kind, 1, c, stride if columns is None else columns, n, delta, bins, device, prior=prior, given=given,
                      threshold=threshold)
    ps.accumulate(torch.from_numpy(x).to(ps.device))
    res = ps.result()
    ps.free()
    return res
