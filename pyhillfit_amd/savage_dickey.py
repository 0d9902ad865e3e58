"""Savage-Dickey Bayes factor B12 of "Hill fixed at 1" (model 1) against "Hill free" (model 2) from the t = 1 draws of the model-2 fit
alone (Dickey 1971; Verdinelli & Wasserman 1995), the SAME number thermodynamic integration and the stepping stone reach through a
tempered ladder per pair and model.

Model 1 is model 2 at Hill = 1; the priors on pIC50 and sigma are the same independent factors in both models and Hill's prior is
uniform on [0, 10].  Then

    B12 = p(Hill = 1 | y, M2) / pi(Hill = 1 | M2) = 10 p(Hill = 1 | y, M2) = E_{(pIC50, sigma) | y, M2} [ r ],
    r   = L(pIC50, 1, sigma) / ( (1/10) INT_0^10 L(pIC50, h, sigma) dh )

(Rao-Blackwell: the conditional density of Hill at 1, normalised by quadrature at the draw's pIC50 and sigma; the draw's own Hill is
not used).  It is NOT valid once one model's prior on pIC50 or sigma, or Hill's uniform prior, is changed: the assertions below and
in pyhillfit_amd/csrc/phf_savage_dickey.h stand guard.

The GPU keeps, per (problem, chain), the sums of r over every T-th post-burn-in row while the rows stream past
(phf_savage_dickey_accumulate); the chains are merged here, in fp64.  `se` is the between-chain Monte Carlo error only."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib, accumulator
from . import doseresponse as dr
from .sampler import DevicePoints, _ptr, _stream_ptr

PANEL_CHOICES = (16, 32, 64)
DEFAULT_PANELS = 32
PANEL_NODES = 15
DEFAULT_EVERY = 11                      # --savage-dickey-every: measured, the densest thinning whose cost stays within the sampling time
                                        # of a default `-m 2 -a` Crumb run at P = 32 ("Savage-Dickey Bayes factor")
ACC_DOUBLES = 8                         # phf_savage_dickey.h
USED, SKIPPED, SUM_R, SUM_R2, MAX_R, SUM_RC, MAX_GAP = range(7)
HILL_NULL, HILL_LOWER, HILL_UPPER = 1.0, 0.0, 10.0
MAX_ENTRIES = 256                       # entries per pair the kernel's LDS slices hold (phf_savage_dickey.hip: kMaxStride)
MIN_ESS = 100.0                         # conventions, not measurements (like the stepping stone's lowest-ESS flag): below this many
GAP_FRACTION = 0.01                     # effective draws, or a fine-coarse gap above 1 % of max(|log B12|, se), `reliable` is false
METHOD = ("Savage-Dickey density ratio from the model-2 draws alone: B12 = p(Hill = 1 | y, M2) / pi(Hill = 1 | M2) = the mean over the "
          "draws' (pIC50, sigma) of r = L(pIC50, 1, sigma) / ((1/10) INT_0^10 L(pIC50, h, sigma) dh); the integral by the 15-point "
          "Gauss-Kronrod rule on each of P equal panels of [0, 10] (log_b12_coarse: the 7 embedded Gauss nodes; gap = |log_b12 - "
          "log_b12_coarse|; quadrature_gap_max: the largest |log r - log r_coarse| of a draw); over every T-th post-burn-in row of all "
          "chains; B12 is the mean over chains of the chains' means, log_b12_se the between-chain standard deviation / sqrt(chains) / "
          "B12: Monte Carlo error only; ess = (SUM r)^2 / SUM r^2 pooled, max_share the largest r over SUM r")
NOTE = ("the same B12 = Z1 / Z2 thermodynamic integration targets, valid only for the nested priors of models 1 and 2 (same priors on "
        "pIC50 and sigma, Hill uniform on [0, 10]).  When Hill = 1 lies far in the tail of the posterior, few draws carry the sum "
        "(small ess, max_share near 1): the number is then a bound on how strongly model 2 is favoured, not an estimate")

# 15-point Kronrod rule on [-1, 1] and its 7 embedded Gauss-Legendre nodes: abscissae xgk, weights wgk and wg of QUADPACK's qk15
# (Piessens, de Doncker-Kapenga, Ueberhuber & Kahaner 1983, "QUADPACK", Springer; netlib.org/quadpack/dqk15.f), the non-negative
# half, outermost first.  tests/test_savage_dickey_host.py holds them to polynomial exactness (degree 22 and 13).
_XGK = (0.991455371120812639206854697526329, 0.949107912342758524526189684047851, 0.864864423359769072789712788640926,
        0.741531185599394439863864773280788, 0.586087235467691130294144838258730, 0.405845151377397166906606412076961,
        0.207784955007898467600689403773245, 0.0)
_WGK = (0.022935322010529224963732008058970, 0.063092092629978553290700663189204, 0.104790010322250183839876322541518,
        0.140653259715525918745189590510238, 0.169004726639267902826583426598550, 0.190350578064785409913256402421014,
        0.204432940075298892414161999234649, 0.209482141084727828012999174891714)
_WG = (0.129484966168869693270611432679082, 0.279705391489276667901467771423780, 0.381830050505118944950369775488975,
       0.417959183673469387755102040816327)


def check_priors():
    """the nesting the density ratio rests on, against the constants the samplers' priors are built from"""
    if not (dr.hill_uniform_lower == HILL_LOWER and dr.hill_uniform_upper == HILL_UPPER and HILL_LOWER < HILL_NULL < HILL_UPPER):
        raise AssertionError("the Savage-Dickey ratio assumes Hill ~ uniform[0, 10] under model 2 and Hill = 1 under model 1")
    if dr.sigma_uniform_lower != dr.sigma_loc:
        raise AssertionError("the Savage-Dickey ratio assumes one sigma support for both models")


def check_panels(panels):
    if int(panels) not in PANEL_CHOICES:
        raise ValueError("--savage-dickey-panels must be one of %s, got %r" % (", ".join(map(str, PANEL_CHOICES)), panels))
    return int(panels)


def rows_used(first_row, num_rows, every):
    """the number of global rows r in [first_row, first_row + num_rows) with r mod every == 0"""
    if first_row < 0 or num_rows < 0 or every < 1:
        raise ValueError("first_row and num_rows must be >= 0 and every >= 1")
    end = first_row + num_rows
    return (end + every - 1) // every - (first_row + every - 1) // every


def unit_rule():
    """the 15 nodes on [-1, 1] in ascending order, the Kronrod weights and the Gauss weights (0 at the 8 nodes that are no Gauss nodes)"""
    xk, wk, wg = np.array(_XGK), np.array(_WGK), np.array(_WG)
    x = np.concatenate([-xk[:-1], xk[::-1]])
    w = np.concatenate([wk[:-1], wk[::-1]])
    g = np.zeros(PANEL_NODES)
    g[1::2] = np.concatenate([wg[:-1], wg[::-1]])
    return x, w, g


def node_table(panels=DEFAULT_PANELS):
    """[3][15 P] float64: h_k over [0, 10] in ascending order, ln w_k of the Kronrod rule (fine), ln w_k of the embedded Gauss rule
    (coarse; -inf where the node is no Gauss node).  Made once, in fp64; the host twin and the kernel read these same doubles."""
    P = check_panels(panels)
    x, w, g = unit_rule()
    edges = HILL_LOWER + (HILL_UPPER - HILL_LOWER) * np.arange(P + 1, dtype=np.float64) / P
    mid, half = 0.5 * (edges[:-1] + edges[1:]), 0.5 * (edges[1:] - edges[:-1])
    t = np.empty((3, PANEL_NODES * P))
    t[0] = (mid[:, None] + half[:, None] * x[None, :]).ravel()
    t[1] = np.log((half[:, None] * w[None, :]).ravel())
    with np.errstate(divide="ignore"):
        t[2] = np.log((half[:, None] * g[None, :]).ravel())
    return t


def workspace_bytes(num_problems, chains, panels=DEFAULT_PANELS):
    """device bytes SavageDickey holds: the accumulators and the node table (the entries are the sampler's own)"""
    return 8 * (num_problems * chains * ACC_DOUBLES + 3 * PANEL_NODES * int(panels))


class SavageDickey(accumulator.RowAccumulator):
    """Streaming sums of r for num_problems model-2 problems over `chains` chains: accumulate() takes the post-burn-in rows in order,
    a segment at a time, as views of the sampler's row buffer [rows][Q][4][chains] (asynchronous, on the current stream); exactly
    the global rows r with r mod every == 0 are used, however the calls cut them.  points: the sampler's DevicePoints (or a
    PackedPoints), pair q <-> problem q.  result() downloads the sums and finalizes."""

    tensors = ("acc", "table")

    def __init__(self, points, num_problems, chains, panels=DEFAULT_PANELS, every=DEFAULT_EVERY, device="cuda"):
        check_priors()
        accumulator.RowAccumulator.__init__(self, device)
        self.panels, self.every = check_panels(panels), int(every)
        if self.every < 1:
            raise ValueError("every must be >= 1, got %r" % (every,))
        self.points = points if isinstance(points, DevicePoints) else DevicePoints(points, self.device)
        self.Q, self.C = int(num_problems), int(chains)
        if self.points.packed.num_pairs != self.Q:
            raise ValueError("the points must have one pair per problem (%d pairs, %d problems)" % (self.points.packed.num_pairs, self.Q))
        if self.points.packed.stride > MAX_ENTRIES:
            raise ValueError("the Savage-Dickey kernel takes at most %d entries per pair, got %d" % (MAX_ENTRIES, self.points.packed.stride))
        self.table = torch.from_numpy(node_table(self.panels)).to(self.device)
        self.acc = torch.zeros((self.Q, self.C, ACC_DOUBLES), dtype=torch.float64, device=self.device)

    def _check_rows(self, rows):
        if rows.dim() != 4 or rows.shape[1] != self.Q or rows.shape[3] != self.C or rows.shape[2] != 4:
            raise ValueError("rows must be model-2 rows [n][%d][4][%d], got %s" % (self.Q, self.C, tuple(rows.shape)))
        accumulator.check_tensor(rows, self.device)

    def _accumulate(self, rows, n):
        _lib.check(self.lib.phf_savage_dickey_accumulate(C.byref(self.points.struct), self.panels, _ptr(self.table), _ptr(rows), n, self.Q,
                                                         rows.shape[2], self.C, self.rows_seen, self.every, _ptr(self.acc),
                                                         self.acc.numel() * 8, _stream_ptr(self.device)), "phf_savage_dickey_accumulate")

    def accumulators(self):
        """numpy [Q][C][8]"""
        return self.acc.cpu().numpy()

    def result(self):
        """one dict per problem"""
        acc = self.accumulators()
        return [finalize(acc[q], self.panels, self.every) for q in range(self.Q)]


def _log(v):
    return math.log(v) if v > 0.0 and math.isfinite(v) else float("nan")


def _mean_of_means(acc, column):
    """(mean over the chains with a used draw of their means, those means)"""
    n = acc[:, USED]
    have = n > 0
    means = acc[have, column] / n[have]
    return (float(np.mean(means)) if means.size else float("nan")), means


def finalize(acc, panels, every):
    """one problem: acc [C][8] -> the Bayes factor, its Monte Carlo error and its health"""
    acc = np.asarray(acc, dtype=np.float64)
    chains = acc.shape[0]
    b, means = _mean_of_means(acc, SUM_R)
    bc, _ = _mean_of_means(acc, SUM_RC)
    m = means.size
    se = float(np.std(means, ddof=1) / math.sqrt(m)) if m >= 2 else float("nan")
    log_b, log_bc = _log(b), _log(bc)
    n = float(acc[:, USED].sum())
    s1, s2 = float(acc[:, SUM_R].sum()), float(acc[:, SUM_R2].sum())
    frac = s1 * s1 / (n * s2) if n > 0 and s2 > 0.0 and math.isfinite(s2) else float("nan")
    parity = [_log(_mean_of_means(acc[h::2], SUM_R)[0]) if acc[h::2].shape[0] else float("nan") for h in (0, 1)]
    res = {"panels": int(panels), "every": int(every), "chains": int(chains), "b12": b, "log_b12": log_b, "se": se,
           "log_b12_se": se / b if b > 0.0 else float("nan"), "log_b12_coarse": log_bc,
           "gap": abs(log_b - log_bc) if log_b != log_bc else 0.0, "quadrature_gap_max": float(acc[:, MAX_GAP].max()) if n > 0 else float("nan"),
           "ess_fraction": frac, "ess": frac * n, "max_share": float(acc[:, MAX_R].max()) / s1 if s1 > 0.0 else float("nan"),
           "log_b12_parity": parity, "draws_used": int(n), "draws_skipped": int(acc[:, SKIPPED].sum())}
    res["reliable"], res["reason"] = verdict(res)
    return res


def verdict(res):
    """(reliable, reason): the two conventions MIN_ESS and GAP_FRACTION, and a number that exists at all"""
    if not math.isfinite(res["log_b12"]):
        return False, "no usable draw" if res["draws_used"] == 0 else "log B12 is not finite"
    if not res["ess"] >= MIN_ESS:
        return False, "ess {:.3g} is below {:g}: few draws carry the sum (Hill = 1 in the tail of the posterior); a bound, not an estimate".format(
            res["ess"], MIN_ESS)
    scale = max(abs(res["log_b12"]), res["log_b12_se"] if math.isfinite(res["log_b12_se"]) else 0.0)
    if res["gap"] > GAP_FRACTION * scale:
        return False, "the fine-coarse quadrature gap {:.3g} exceeds {:g} % of max(|log B12|, se) = {:.3g}: use more panels".format(
            res["gap"], 100 * GAP_FRACTION, scale)
    return True, None


def json_record(res):
    """the summary's "bayes_factor" object of one problem (NaN -> null)"""
    num = _lib._num
    rec = {"method": METHOD, "panels": res["panels"], "every": res["every"], "b12": num(res["b12"]), "log_b12": num(res["log_b12"]),
           "log_b12_se": num(res["log_b12_se"]),
           "hill_one_posterior_density": num(res["b12"] / (HILL_UPPER - HILL_LOWER)), "log_b12_coarse": num(res["log_b12_coarse"]),
           "gap": num(res["gap"]), "quadrature_gap_max": num(res["quadrature_gap_max"]), "ess_fraction": num(res["ess_fraction"]),
           "ess": num(res["ess"]), "max_share": num(res["max_share"]),
           "log_b12_by_chain_parity": [num(v) for v in res["log_b12_parity"]] if res["chains"] > 1 else None,
           "draws_used": res["draws_used"], "draws_skipped": res["draws_skipped"],
           "favours": None if not math.isfinite(res["log_b12"]) else ("model 1" if res["log_b12"] > 0.0 else "model 2"),
           "reliable": bool(res["reliable"]), "note": NOTE}
    if not res["reliable"]:
        rec["reason"] = res["reason"]
    return rec


def report_line(rank, names, results):
    """one line per rank: how many pairs favour each model, how many are not reliable, and the pair with the largest |log B12|"""
    if len(names) == 0:
        return "bayes-factor [rank %d]: no problems" % rank
    finite = [(abs(r["log_b12"]), q) for q, r in enumerate(results) if math.isfinite(r["log_b12"])]
    if not finite:
        return "bayes-factor [rank {}]: {} problems, none with a usable draw".format(rank, len(names))
    one = sum(1 for r in results if math.isfinite(r["log_b12"]) and r["log_b12"] > 0.0)
    _, q = max(finite)
    r = results[q]
    return ("bayes-factor [rank {}]: {} problems, P = {} panels, {} draws each; {} favour model 1 (Hill = 1), {} favour model 2 (Hill free), "
            "{} not reliable; largest |log B12|: {} with {:.4g} +- {:.2g} (ess {:.3g}); {} draws skipped"
            .format(rank, len(names), r["panels"], r["draws_used"], one, len(finite) - one, sum(1 for x in results if not x["reliable"]),
                    names[q], r["log_b12"], r["log_b12_se"], r["ess"], sum(x["draws_skipped"] for x in results)))


def bayes_factor_of_draws(concs, responses, draws, panels=DEFAULT_PANELS, every=1, device="cuda:0"):
    """draws [rows][4][chains] of one model-2 problem (chain files) with the data concs, responses -> its finalized result, through
    the same kernel"""
    x = np.ascontiguousarray(np.asarray(draws, dtype=np.float64)[:, None, :, :])
    sd = SavageDickey(dr.PackedPoints([(concs, responses)]), 1, x.shape[3], panels, every, device)
    sd.accumulate(torch.from_numpy(x).to(sd.device))
    res = sd.result()[0]
    sd.free()
    return res
