"""Expected information gain (EIG) of one further measurement at a candidate dose: at which concentration should the next
measurement be taken?  (Lindley 1956; Chaloner & Verdinelli 1995.)

    EIG(d) = H[ pbar(y | d) ] - E_theta H[ p(y | theta, d) ],      pbar(y | d) = E_theta p(y | theta, d)

is the mutual information between the new response y at dose d and the parameters under the current posterior.  The single-level
models only: a draw is (pIC50, sigma) with Hill = 1 or (pIC50, Hill, sigma), the new response the likelihood's censored normal.  The
estimator is the gain of a measurement RECORDED TO A RESOLUTION of 100/K % block: the response falls into one of K + 2 categories
(the point masses at 0 and at 100, K equal bins of (0, 100)) whose masses are exact differences of Phi, well defined for every sigma
(pyhillfit_amd/csrc/phf_design.h).  It is a lower bound of the continuous mutual information (data-processing inequality) and rises
monotonically when K doubles (the partitions are nested); `eig_coarse`, the K/2 value, comes out of the same pass and `gap` =
eig - eig_coarse says how much the last doubling still added.

The GPU keeps, per (problem, dose, slot of chains), the sums over the draws of the K + 2 masses and of the two per-draw entropies
while the rows stream past (phf_design_accumulate); the final H[pbar] - mean h is taken here, in fp64, from the downloaded sums."""
import ctypes as C

import numpy as np
import torch

from . import _lib, accumulator
from .sampler import _ptr, _stream_ptr

BIN_CHOICES = (128, 256, 512, 1024)
DEFAULT_BINS = 256
DEFAULT_DOSES = 16                      # chain_design's grid
DEFAULT_EVERY = 17                      # --next-dose-every: measured, the densest thinning whose cost stays within the sampling time
                                        # of a default `-m 2 -a` Crumb run at G = 16, K = 256 ("Next dose")
LANES = 64                              # phf_design.h
MAX_SLOTS = 64
TARGET_WAVEFRONTS = 4096                # (problem, dose, slot) wavefronts that fill the chip: 256 CUs x 4 SIMDs x 4
CRITERION = ("expected information gain (mutual information between the new response and the parameters; Lindley 1956, Chaloner & "
             "Verdinelli 1995), in nats, of ONE further measurement at the dose recorded to a resolution of 100/K % block: K + 2 "
             "categories (point masses at 0 and 100 of the censored normal, K equal bins between) with exact masses from differences "
             "of Phi; a lower bound of the continuous value that rises with K; eig_coarse is the K/2 value, gap = eig - eig_coarse; "
             "over every T-th post-burn-in row of all chains; eig_by_chain_parity: the even and the odd chains' own values")


def check_bins(bins):
    if int(bins) not in BIN_CHOICES:
        raise ValueError("--next-dose-bins must be one of %s, got %r" % (", ".join(map(str, BIN_CHOICES)), bins))
    return int(bins)


def acc_doubles(bins):
    """doubles of one (problem, dose, slot) accumulator: PHF_DS_ACC_DOUBLES of phf_design.h"""
    return int(bins) + 2 + 2 * LANES + 2


def rows_used(first_row, num_rows, every):
    """the number of global rows r in [first_row, first_row + num_rows) with r mod every == 0"""
    if first_row < 0 or num_rows < 0 or every < 1:
        raise ValueError("first_row and num_rows must be >= 0 and every >= 1")
    end = first_row + num_rows
    return (end + every - 1) // every - (first_row + every - 1) // every


def default_slots(num_problems, num_doses, chains):
    """the accumulator slots the chains are dealt to: a power of two, at least 2 (the parities), doubled while the
    (problem, dose, slot) wavefronts do not fill the chip and every slot still has a chain.  A function of the run's shape alone."""
    ns = 2
    while ns < MAX_SLOTS and num_problems * num_doses * ns < TARGET_WAVEFRONTS and 2 * ns <= chains:
        ns *= 2
    return ns


def candidate_doses(concs, points, named=()):
    """the candidates of a pair (uM): `points` doses log-spaced from its smallest dose / 10 to its largest x 10, then the named ones"""
    from .quantiles import curve_doses
    return np.concatenate([curve_doses(concs, points), np.asarray(named or (), dtype=np.float64)])


def parse_concs(text):
    """'0.1,10' -> tuple of concentrations in uM, all > 0 and finite (raises ValueError)"""
    concs = tuple(float(v) for v in str(text).split(",") if v.strip())
    if not concs or not all(np.isfinite(c) and c > 0.0 for c in concs):
        raise ValueError("--next-dose-concs must be concentrations in uM, all > 0, got %r" % (text,))
    return concs


def workspace_bytes(num_problems, num_doses, bins, chains, slots=None):
    """device bytes NextDose holds: the accumulators and the doses"""
    ns = default_slots(num_problems, num_doses, chains) if slots is None else int(slots)
    return 8 * num_problems * num_doses * (ns * acc_doubles(bins) + 1)


class NextDose(accumulator.RowAccumulator):
    """Streaming EIG sums of num_problems single-level problems (model 1 | 2) over `chains` chains at the candidate doses `doses`
    ([num_problems][G], uM): accumulate() takes the post-burn-in rows in order, a segment at a time, as views of the sampler's row
    buffer [rows][Q][stride][chains] (asynchronous, on the current stream); exactly the global rows r with r mod every == 0 are
    used, however the calls cut them.  result() downloads the sums and finalizes; tested: per problem, the concentrations it has
    data at (for `already_tested`)."""

    tensors = ("acc", "ln_doses")

    def __init__(self, model, num_problems, chains, doses, tested=None, bins=DEFAULT_BINS, every=DEFAULT_EVERY, device="cuda", slots=None):
        if model not in (1, 2):
            raise ValueError("the next-dose analysis is single-level only (model 1 or 2), got %r" % (model,))
        accumulator.RowAccumulator.__init__(self, device)
        self.model, self.bins, self.every = int(model), check_bins(bins), int(every)
        self.min_cols = self.model + 1
        if self.every < 1:
            raise ValueError("every must be >= 1, got %r" % (every,))
        self.Q, self.C = int(num_problems), int(chains)
        d = np.ascontiguousarray(np.asarray(doses, dtype=np.float64))
        if d.ndim != 2 or d.shape[0] != self.Q or d.shape[1] < 1 or not np.all(np.isfinite(d) & (d > 0.0)):
            raise ValueError("doses must be [%d][G >= 1] positive finite concentrations" % self.Q)
        self.doses, self.G = d, d.shape[1]
        self.tested = [np.asarray(t, dtype=np.float64) for t in tested] if tested is not None else [np.zeros(0)] * self.Q
        self.slots = default_slots(self.Q, self.G, self.C) if slots is None else int(slots)
        self.ln_doses = torch.from_numpy(np.log(d)).to(self.device)
        self.acc = torch.zeros((self.Q, self.G, self.slots, acc_doubles(self.bins)), dtype=torch.float64, device=self.device)

    def _accumulate(self, rows, n):
        _lib.check(self.lib.phf_design_accumulate(self.model, self.bins, _ptr(rows), n, self.Q, rows.shape[2], self.C, self.rows_seen,
                                                  self.every, _ptr(self.ln_doses), self.G, self.slots, _ptr(self.acc),
                                                  self.acc.numel() * 8, _stream_ptr(self.device)), "phf_design_accumulate")

    def accumulators(self):
        """numpy [Q][G][slots][acc_doubles(bins)]"""
        return self.acc.cpu().numpy()

    def result(self):
        """one dict per problem"""
        acc = self.accumulators()
        return [finalize(acc[q], self.doses[q], self.tested[q], self.bins, self.every, self.C) for q in range(self.Q)]


def _entropy(p):
    """-sum p ln p, 0 ln 0 = 0"""
    p = np.asarray(p, dtype=np.float64)
    pos = p > 0.0
    return float(-np.sum(p[pos] * np.log(p[pos])))


def gain(masses, h_fine, h_coarse, n, bins):
    """(eig, eig_coarse, pbar at 0, pbar at 100) from SUM masses [K + 2], SUM h_fine, SUM h_coarse over n draws; NaN without draws"""
    if n <= 0:
        return (float("nan"),) * 4
    p = np.asarray(masses, dtype=np.float64) / n
    pc = np.concatenate([p[:1], p[1:bins + 1].reshape(-1, 2).sum(axis=1), p[bins + 1:]])
    return _entropy(p) - h_fine / n, _entropy(pc) - h_coarse / n, float(p[0]), float(p[bins + 1])


def fold(acc, bins):
    """acc [slots][acc_doubles] of one (problem, dose) -> per parity (even slots, odd slots) the SUM masses [2][K + 2], SUM h_fine
    [2], SUM h_coarse [2], draws used [2], draws skipped [2].  One fixed order: a slot's 64 lane sums first, then the slots of a
    parity in ascending order."""
    K = int(bins)
    hf = acc[:, K + 2:K + 2 + LANES].sum(axis=1)
    hc = acc[:, K + 2 + LANES:K + 2 + 2 * LANES].sum(axis=1)
    out = [np.zeros((2, K + 2)), np.zeros(2), np.zeros(2), np.zeros(2), np.zeros(2)]
    for s in range(acc.shape[0]):
        out[0][s & 1] += acc[s, :K + 2]
        out[1][s & 1] += hf[s]
        out[2][s & 1] += hc[s]
        out[3][s & 1] += acc[s, K + 2 + 2 * LANES]
        out[4][s & 1] += acc[s, K + 3 + 2 * LANES]
    return out


def finalize(acc, doses, tested, bins, every, chains):
    """one problem: acc [G][slots][acc_doubles] -> the per-candidate arrays and the best candidate"""
    G = acc.shape[0]
    res = {k: np.full(G, np.nan) for k in ("eig", "eig_coarse", "mass_at_0", "mass_at_100")}
    res["eig_parity"] = np.full((G, 2), np.nan)
    used = skipped = 0
    for g in range(G):
        m, hf, hc, n, sk = fold(acc[g], bins)
        res["eig"][g], res["eig_coarse"][g], res["mass_at_0"][g], res["mass_at_100"][g] = gain(m[0] + m[1], hf[0] + hf[1], hc[0] + hc[1],
                                                                                              n[0] + n[1], bins)
        for h in (0, 1):
            res["eig_parity"][g, h] = gain(m[h], hf[h], hc[h], n[h], bins)[0]
        if g == 0:
            used, skipped = int(n[0] + n[1]), int(sk[0] + sk[1])
    tested = np.asarray(tested, dtype=np.float64)
    res["doses"] = np.asarray(doses, dtype=np.float64)
    res["already_tested"] = [bool(np.any(np.isclose(d, tested, rtol=1e-9, atol=0.0))) for d in res["doses"]]
    res["gap"] = res["eig"] - res["eig_coarse"]
    res["best"] = int(np.nanargmax(res["eig"])) if np.any(np.isfinite(res["eig"])) else None
    res.update(bins=int(bins), every=int(every), chains=int(chains), draws_used=used, draws_skipped=skipped)
    return res


def _candidate(res, g):
    num = _lib._num
    return {"dose": float(res["doses"][g]), "eig": num(res["eig"][g]), "eig_coarse": num(res["eig_coarse"][g]), "gap": num(res["gap"][g]),
            "eig_by_chain_parity": [num(v) for v in res["eig_parity"][g]] if res["chains"] > 1 else None,
            "predictive_mass_at_0": num(res["mass_at_0"][g]), "predictive_mass_at_100": num(res["mass_at_100"][g]),
            "already_tested": bool(res["already_tested"][g])}


def json_record(res):
    """the summary's "next_dose" object of one problem (NaN -> null)"""
    cands = [_candidate(res, g) for g in range(len(res["doses"]))]
    return {"bins": res["bins"], "every": res["every"], "draws_used": res["draws_used"], "draws_skipped": res["draws_skipped"],
            "candidates": cands, "best": dict(cands[res["best"]]) if res["best"] is not None else None, "criterion": CRITERION}


def report_line(rank, names, results, grid=None):
    """one line per rank: the pair with the largest best-dose EIG, and how many pairs have their best dose at an end of the grid
    (grid: the number of log-spaced candidates in front of the named ones; all of them if not given)"""
    if len(names) == 0:
        return "next-dose [rank %d]: no problems" % rank
    best = [(r["eig"][r["best"]], q) for q, r in enumerate(results) if r["best"] is not None]
    if not best:
        return "next-dose [rank {}]: {} problems, none with a usable draw".format(rank, len(names))
    top, q = max(best)
    r = results[q]
    ends = 0
    for res in results:
        G = len(res["doses"]) if grid is None else int(grid)
        ends += int(res["best"] is not None and G > 1 and res["best"] in (0, G - 1))
    return ("next-dose [rank {}]: {} problems, K = {} bins, {} draws each; largest best-dose EIG {:.4f} nats: {} at {:.4g} uM; {} problems "
            "have their best dose at an end of the grid (widen the range); {} draws skipped"
            .format(rank, len(names), r["bins"], r["draws_used"], top, names[q], r["doses"][r["best"]], ends,
                    sum(res["draws_skipped"] for res in results)))


def design_of_draws(model, draws, doses, tested=None, bins=DEFAULT_BINS, every=1, device="cuda:0", slots=None):
    """draws [rows][columns][chains] of one problem (chain files) -> its finalized result, through the same kernel"""
    x = np.ascontiguousarray(np.asarray(draws, dtype=np.float64)[:, None, :, :])
    nd = NextDose(model, 1, x.shape[3], np.asarray(doses, dtype=np.float64)[None, :], [tested] if tested is not None else None, bins,
                  every, device, slots)
    nd.accumulate(torch.from_numpy(x).to(nd.device))
    res = nd.result()[0]
    nd.free()
    return res
