"""Posterior quantiles and credible intervals over all chains, and credible bands of the dose-response curve.

Per problem and column, over the S = rows x chains post-burn-in draws, the device keeps an exact-count histogram
(phf_quantiles_accumulate, one segment at a time: no draw is kept).  Its grid is fixed by an anchor a (the first finite draw),
a power-of-two base width w0 = 2^(floor(log2 max(|a|, 2^-30)) - 40) and a level k, the least whose B bins hold [min, max]:

    t = (x - a) * (1/w0),    j = floor(t * 2^-k) + B/2.

Raising k merges bins 2^dk-fold in place, and floor(floor(y)/2^m) = floor(y/2^m): the final counts are those of binning every draw
at the final grid, the same however the rows are cut into segments.  Unless k = 0, a bin is at most 4 (max - min)/B wide (2.4e-4
of the draws' range at B = 16 384).  For each p the reduce finds the bin of the rank r = ceil(p N) draw (clamped to [1, N]) —
the inverse empirical CDF, numpy's quantile(method="inverted_cdf") — and reports its edges [lo, hi], clamped to [min, max], which
hold the exact sample quantile, and a value interpolated linearly by rank inside the bin.  Non-finite draws are counted apart.

Curve bands (single-level model 1 or 2): per draw the Hill curve 100 (1 - 1/(1 + exp(Hill (ln c - ln IC50)))) at G doses of the
pair, binned as G more columns through the same histograms; the curve is never written to memory.

Hierarchical bands (band_ln_doses): per draw (alpha, beta, mu, s) of a hierarchical row and per dose, the curve of the inferred
underlying effect (Hill = alpha, pIC50 = mu) and of a predicted future experiment (Hill* ~ log-logistic(alpha, beta), pIC50* ~
logistic(mu, s), drawn by inversion from the draw's own Philox block: csrc/phf_hier_bands.h), binned as 2 D more columns."""
import ctypes as C

import numpy as np
import torch

from . import _lib, accumulator
from ._lib import _num
from .sampler import _ptr, _stream_ptr

DEFAULT_PROBS = (0.025, 0.05, 0.25, 0.5, 0.75, 0.95, 0.975)
DEFAULT_BINS = 16384
HEAD = 8                                # out: min, max, draws, non-finite, bin width, level, anchor, w0
PER_PROB = 4                            # out: value, lo, hi, bin
INTERVALS = {"ci90": (0.05, 0.95), "ci95": (0.025, 0.975)}
METHOD = ("inverse empirical CDF (numpy quantile method='inverted_cdf': the ceil(p N)-th smallest draw) over all chains' post-burn-in "
          "draws, from an exact-count histogram of B bins whose grid is anchored at the first draw and coarsened by powers of two to "
          "hold [min, max]: [lo, hi] is the bin holding that draw, value is linear in rank inside it")
BAND_METHOD = ("percent block 100 (1 - 1/(1 + exp(Hill (ln c - ln IC50)))) per post-burn-in draw (alpha, beta, mu, s) of every chain; "
               "underlying: Hill = alpha, pIC50 = mu; future_experiment: one replicate per draw by inversion, Hill* = alpha exp(logit(u_H) / "
               "beta) (log-logistic(scale alpha, shape beta)), pIC50* = mu + s logit(u_P) (logistic(mu, s)), u = (k + 1/2) 2^-52 with k = "
               "(w_a >> 6) 2^26 + (w_b >> 6) from words (0, 1) (Hill) and (2, 3) (pIC50) of the Philox4x32 block (the samplers' rounds) "
               "counter = (chain_id_base + chain, problem id, post-burn-in row index, 0xC0000000), key = seed; quantiles per dose: " + METHOD)
MAX_BAND_CONCS = 64


def parse_probs(text):
    """'0.025,0.5,...' -> tuple of floats in [0, 1] (raises ValueError)"""
    probs = tuple(float(v) for v in str(text).split(",") if v.strip())
    if not probs or len(probs) > 64 or not all(0.0 <= p <= 1.0 for p in probs):
        raise ValueError("quantile probabilities must be 1 to 64 numbers in [0, 1], got %r" % (text,))
    return probs


def check_bins(bins):
    b = int(bins)
    if b < 64 or b > 32768 or b & (b - 1):
        raise ValueError("--quantile-bins must be a power of two in [64, 32768], got %d" % b)
    return b


def workspace_bytes(num_problems, columns, curve_points=0, bins=DEFAULT_BINS):
    """device bytes PosteriorQuantiles holds: num_problems (columns + curve_points) (8 bins + 72) (raises on an invalid shape)"""
    return accumulator.workspace_bytes("phf_quantiles_workspace_bytes", num_problems, columns, curve_points, bins)


def curve_doses(concs, points):
    """G doses log-spaced from the pair's smallest dose / 10 to its largest x 10 (uM)"""
    c = np.asarray(concs, dtype=np.float64)
    c = c[c > 0]
    return np.logspace(np.log10(c.min() / 10.0), np.log10(c.max() * 10.0), int(points))


def parse_band_concs(text):
    """'0.1,10' -> tuple of concentrations in uM, all > 0 and finite, at most 64 (raises ValueError)"""
    concs = tuple(float(v) for v in str(text).split(",") if v.strip())
    if not concs or len(concs) > MAX_BAND_CONCS or not all(np.isfinite(c) and c > 0.0 for c in concs):
        raise ValueError("--band-concs must be 1 to %d concentrations in uM, all > 0, got %r" % (MAX_BAND_CONCS, text))
    return concs


def band_doses(concs, points, named=()):
    """the doses of a hierarchical band: the G grid doses of curve_doses, then the named concentrations"""
    return np.concatenate([curve_doses(concs, points), np.asarray(named, dtype=np.float64)])


def hill_curve(model, ln_dose, pic50, hill):
    """the curve the device bins, in numpy: 100 (1 - 1/(1 + exp(Hill (ln c - ln IC50)))), exp's argument capped at 40 as the
    targets cap it (model 1: Hill = 1)"""
    h = 1.0 if model == 1 else hill
    arg = np.minimum(h * (ln_dose - np.log(10.0) * (6.0 - pic50)), 40.0)
    return 100.0 * (1.0 - 1.0 / (1.0 + np.exp(arg)))


class PosteriorQuantiles(accumulator.RowAccumulator):
    """Streaming quantiles of num_problems x columns over `chains` chains and total_rows post-burn-in rows; with curve_ln_doses
    ([num_problems][G], natural log of the doses) and model 1 | 2 also the Hill curve at G doses per problem.
    accumulate() takes the rows in order, a segment at a time, as views of the sampler's row buffer [rows][Q][stride][chains]
    (asynchronous, on the current stream); result() reduces.
    Hierarchical bands: with band_ln_doses ([num_problems][D]) the rows are hierarchical ones and, per problem, D slots of the
    underlying effect and D of a future experiment follow the columns; the future experiment's stream is addressed by seed,
    problem_ids ([num_problems], the samplers' global problem ids) and chain_id_base."""

    tensors = ("ws", "ln_doses", "problem_id")

    def __init__(self, num_problems, chains, columns, total_rows, probs=DEFAULT_PROBS, bins=DEFAULT_BINS, device="cuda",
                 curve_ln_doses=None, model=None, band_ln_doses=None, seed=0, problem_ids=None, chain_id_base=0):
        accumulator.RowAccumulator.__init__(self, device)
        self.Q, self.C, self.cols, self.N, self.B = int(num_problems), int(chains), int(columns), int(total_rows), check_bins(bins)
        self.probs = tuple(float(p) for p in probs)
        parse_probs(",".join(repr(p) for p in self.probs))
        self.G, self.model, self.ln_doses = 0, None, None
        if curve_ln_doses is not None:
            if model not in (1, 2):
                raise ValueError("curve bands need the single-level model 1 or 2")
            ld = np.ascontiguousarray(curve_ln_doses, dtype=np.float64)
            if ld.ndim != 2 or ld.shape[0] != self.Q:
                raise ValueError("curve_ln_doses must be [num_problems][G]")
            self.G, self.model = ld.shape[1], int(model)
            self.ln_doses = torch.from_numpy(ld).to(self.device)
        self.D, self.problem_id = 0, None
        if band_ln_doses is not None:
            if curve_ln_doses is not None:
                raise ValueError("single-level curve bands and hierarchical bands do not share a workspace")
            ld = np.ascontiguousarray(band_ln_doses, dtype=np.float64)
            if ld.ndim != 2 or ld.shape[0] != self.Q or ld.shape[1] < 1:
                raise ValueError("band_ln_doses must be [num_problems][D], D >= 1")
            ids = np.arange(self.Q) if problem_ids is None else np.asarray(problem_ids, dtype=np.int64)
            if ids.shape != (self.Q,):
                raise ValueError("problem_ids must name every problem")
            self.D, self.G = ld.shape[1], 2 * ld.shape[1]
            self.seed, self.chain_id_base = int(seed) & 0xFFFFFFFFFFFFFFFF, int(chain_id_base) & 0xFFFFFFFF
            self.ln_doses = torch.from_numpy(ld).to(self.device)
            self.problem_id = torch.from_numpy((ids & 0xFFFFFFFF).astype(np.uint32).view(np.int32)).to(self.device)
        self.min_cols = max(self.cols, 4 if self.D else 0)
        self._init_workspace(workspace_bytes(self.Q, self.cols, self.G, self.B), "phf_quantiles_init", self.Q, self.cols, self.G, self.B)

    def _accumulate(self, rows, n):
        step = max(1, (2 ** 31 - 1) // self.C)                 # rows x chains < 2^31 per call
        for r0 in range(0, n, step):
            part = rows[r0:r0 + step]
            m, first = part.shape[0], self.rows_seen + r0
            if self.cols:
                _lib.check(self.lib.phf_quantiles_accumulate(_ptr(part), m, self.Q, rows.shape[2], self.C, self.cols, self.G, self.B,
                                                             first, self.N, _ptr(self.ws), C.c_size_t(self.nbytes),
                                                             _stream_ptr(self.device)), "phf_quantiles_accumulate")
            if self.D:
                _lib.check(self.lib.phf_quantiles_accumulate_hier_curves(_ptr(part), m, self.Q, rows.shape[2], self.C, _ptr(self.ln_doses),
                                                                         self.cols, self.D, self.B, first, self.N,
                                                                         _ptr(self.problem_id), self.chain_id_base, self.seed,
                                                                         _ptr(self.ws), C.c_size_t(self.nbytes),
                                                                         _stream_ptr(self.device)), "phf_quantiles_accumulate_hier_curves")
            elif self.G:
                _lib.check(self.lib.phf_quantiles_accumulate_curves(_ptr(part), m, self.Q, rows.shape[2], self.C, self.model,
                                                                    _ptr(self.ln_doses), self.cols, self.G, self.B, first,
                                                                    self.N, _ptr(self.ws), C.c_size_t(self.nbytes),
                                                                    _stream_ptr(self.device)), "phf_quantiles_accumulate_curves")

    def counts(self):
        """the histograms: numpy uint64 [Q][columns + G][B], and the non-finite counts [Q][columns + G]"""
        S = self.Q * (self.cols + self.G)
        raw = self.ws.view(torch.int64)
        counts = raw[:S * self.B].cpu().numpy().view(np.uint64).reshape(self.Q, self.cols + self.G, self.B)
        nf = raw[S * self.B + S * HEAD:S * self.B + S * HEAD + S].cpu().numpy().view(np.uint64).reshape(self.Q, self.cols + self.G)
        return counts, nf

    def reduced(self):
        """[Q][columns + G][8 + 4 P] numpy (include/pyhillfit_amd.h, phf_quantiles_reduce)"""
        S = self.Q * (self.cols + self.G)
        P = len(self.probs)
        out = torch.empty((S, HEAD + PER_PROB * P), dtype=torch.float64, device=self.device)
        probs = (C.c_double * P)(*self.probs)
        _lib.check(self.lib.phf_quantiles_reduce(self.Q, self.cols, self.G, self.B, probs, P, _ptr(self.ws), C.c_size_t(self.nbytes),
                                                 _ptr(out), _stream_ptr(self.device)), "phf_quantiles_reduce")
        return out.cpu().numpy().reshape(self.Q, self.cols + self.G, HEAD + PER_PROB * P)

    def result(self):
        """dict of numpy arrays over [Q][columns + G] (the curve points last): min, max, draws, non_finite, bin_width, level, and
        [Q][columns + G][P]: value, lo, hi, bin; probs"""
        red = self.reduced()
        P = len(self.probs)
        per = red[..., HEAD:].reshape(self.Q, self.cols + self.G, P, PER_PROB)
        res = {"min": red[..., 0], "max": red[..., 1], "draws": red[..., 2], "non_finite": red[..., 3], "bin_width": red[..., 4],
               "level": red[..., 5], "value": per[..., 0], "lo": per[..., 1], "hi": per[..., 2], "bin": per[..., 3],
               "probs": np.array(self.probs), "columns": self.cols, "curve_points": self.G}
        if self.D:
            res.update(band_doses=self.D, seed=self.seed)
        return res


def quantiles_of_draws(draws, probs=DEFAULT_PROBS, bins=DEFAULT_BINS, device="cuda"):
    """draws: array [rows][cols][chains] already in memory (burn-in removed), or [rows][cols].  Returns the result() dict of its
    one problem (arrays [cols] / [cols][P])."""
    x = np.asarray(draws, dtype=np.float64)
    if x.ndim == 2:
        x = x[:, :, None]
    n, cols, c = x.shape
    qs = PosteriorQuantiles(1, c, cols, n, probs, bins, device)
    qs.accumulate(torch.from_numpy(np.ascontiguousarray(x[:, None])).to(qs.device))
    res = qs.result()
    qs.free()
    return {k: (v[0] if isinstance(v, np.ndarray) and v.ndim >= 2 else v) for k, v in res.items()}


def exact_quantiles(draws, probs=DEFAULT_PROBS):
    """host ground truth: np.quantile(method="inverted_cdf") of every column's finite draws, [cols][P] (NaN where none)"""
    x = np.asarray(draws, dtype=np.float64)
    if x.ndim == 3:
        x = x.transpose(0, 2, 1).reshape(-1, x.shape[1])
    out = np.full((x.shape[1], len(probs)), np.nan)
    for c in range(x.shape[1]):
        v = x[:, c][np.isfinite(x[:, c])]
        if v.size:
            out[c] = np.quantile(v, probs, method="inverted_cdf")
    return out


def _intervals(probs, value, lo, hi):
    rec = {}
    for name, (pl, ph) in INTERVALS.items():
        if pl in probs and ph in probs:
            i, j = probs.index(pl), probs.index(ph)
            rec[name] = [_num(value[i]), _num(value[j])]
            rec[name + "_bracket"] = [_num(lo[i]), _num(hi[j])]
    return rec


def column_record(res, q, c):
    probs = [float(p) for p in res["probs"]]
    rec = {"value": [_num(v) for v in res["value"][q, c]], "lo": [_num(v) for v in res["lo"][q, c]],
           "hi": [_num(v) for v in res["hi"][q, c]], "min": _num(res["min"][q, c]), "max": _num(res["max"][q, c]),
           "draws": int(res["draws"][q, c]), "non_finite": int(res["non_finite"][q, c]), "bin_width": _num(res["bin_width"][q, c])}
    rec.update(_intervals(probs, res["value"][q, c], res["lo"][q, c], res["hi"][q, c]))
    return rec


def json_record(res, q, columns, bins):
    """the command lines' "quantiles" object of problem q: keyed by column name, plus probs, bins and the method"""
    rec = {name: column_record(res, q, c) for c, name in enumerate(columns)}
    rec["probs"] = [float(p) for p in res["probs"]]
    rec["bins"] = int(bins)
    rec["method"] = METHOD
    return rec


def curve_band_record(res, q, doses):
    """the "curve_band" object of problem q: the doses (uM) and, per dose, the curve's quantiles (percent block)"""
    c0 = int(res["columns"])
    per = [column_record(res, q, c0 + g) for g in range(int(res["curve_points"]))]
    rec = {"doses": [float(d) for d in doses], "probs": [float(p) for p in res["probs"]]}
    for k in ("value", "lo", "hi", "min", "max", "bin_width"):
        rec[k] = [p[k] for p in per]
    for k in INTERVALS:
        if k in per[0]:
            rec[k] = [p[k] for p in per]
    return rec


def _band_part(res, q, first, count):
    per = [column_record(res, q, first + g) for g in range(count)]
    rec = {}
    for k in ("value", "lo", "hi", "min", "max", "bin_width", "non_finite"):
        rec[k] = [p[k] for p in per]
    for k in INTERVALS:
        if k in per[0]:
            rec[k] = [p[k] for p in per]
    return rec


def hier_band_record(res, q, doses, n_grid):
    """the "hierarchical_bands" object of problem q: the doses (uM; n_grid grid doses, then the named concentrations) and, per dose,
    the quantiles (percent block) of the inferred underlying effect and of a predicted future experiment"""
    c0, D = int(res["columns"]), int(res["band_doses"])
    doses = [float(d) for d in doses]
    if len(doses) != D or not 0 <= int(n_grid) <= D:
        raise ValueError("%d doses, %d of them on the grid, for a band of %d" % (len(doses), n_grid, D))
    return {"doses": doses, "probs": [float(p) for p in res["probs"]], "grid_points": int(n_grid),
            "named_concentrations": doses[int(n_grid):], "seed": int(res["seed"]), "method": BAND_METHOD,
            "underlying": _band_part(res, q, c0, D), "future_experiment": _band_part(res, q, c0 + D, D)}


def hier_band_draws(theta, counters, seed, device="cuda"):
    """(Hill*, pIC50*) [m][2] of m draws: theta [m][4] = (alpha, beta, mu, s), counters [m][3] = (chain id, problem id, row) of the
    stream (phf_hier_band_draws); NaN where the parameters give no draw"""
    lib = _lib.load()
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError("hier_band_draws runs on a GPU device, not %s" % dev)
    th = np.ascontiguousarray(np.asarray(theta, dtype=np.float64).reshape(-1, 4).T)
    ct = np.ascontiguousarray(np.asarray(counters, dtype=np.int64).reshape(-1, 3) & 0xFFFFFFFF).astype(np.uint32)
    m = th.shape[1]
    if ct.shape[0] != m:
        raise ValueError("one counter per draw")
    t_th = torch.from_numpy(th).to(dev)
    t_ct = torch.from_numpy(ct.view(np.int32)).to(dev)
    out = torch.empty((m, 2), dtype=torch.float64, device=dev)
    _lib.check(lib.phf_hier_band_draws(m, _ptr(t_th), _ptr(t_ct), int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(out), _stream_ptr(dev)),
               "phf_hier_band_draws")
    return out.cpu().numpy()


def report_line(rank, names, parts, band_non_finite=None):
    """one line per rank: pairs, the widest bin relative to its column's range, non-finite draws (and, with hierarchical bands,
    band_non_finite: the non-finite band draws).
    parts: per problem (bin_width [cols], min [cols], max [cols], non_finite [cols])"""
    if len(names) == 0:
        return "quantiles [rank %d]: no problems" % rank
    rel, nf = 0.0, 0
    for w, lo, hi, n in parts:
        span = np.asarray(hi) - np.asarray(lo)
        ok = span > 0
        if np.any(ok):
            rel = max(rel, float(np.max(np.asarray(w)[ok] / span[ok])))
        nf += int(np.sum(n))
    line = "quantiles [rank {}]: {} pairs; widest bin {:.2e} of its column's range; {} non-finite draws".format(rank, len(names), rel, nf)
    if band_non_finite is not None:
        line += "; {} non-finite band draws".format(int(band_non_finite))
    return line
