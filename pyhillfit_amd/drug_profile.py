"""The per-drug multi-channel block profile: what all the channels of one drug say together at a concentration.

    python -m pyhillfit_amd.drug_profile (--concs c1,c2,... | --cmax-nM X [--multiples 1,3,10]) --channel NAME=FILE[,FILE...]
           [--channel ...] [--weights name=w,...] [--quantile-probs ...] [--bins 4096] [--hierarchical] [--drug NAME] [--device cuda:0]

The posteriors of a drug's channels are independent (each pair is fitted on its own data), so post-burn-in row r, chain c of one
channel beside row r, chain c of the others is one draw of the drug's joint posterior — the pairing of the reference's
chaste/TestCrumbPredictions.hpp:184-216, sample s of each channel with sample s of the others.  Per draw and concentration c (uM):

    block_k  = 100 (1 - 1/(1 + (c / IC50_k)^Hill_k))     percent block of channel k; ApPredict's conductance scaling is 1 - block/100
    net      = SUM_k w_k block_k                         in channel order
    dominant = argmax_k block_k                          ties to the first channel

The device (csrc/phf_drug_profile.hip) keeps exact-count histograms of every block_k and of net on the grid of the quantiles
(quantiles.py: every quantile comes with the bracket that holds the exact sample quantile) and integer tallies of net > 0 and of the
dominant channel, over all draws and by chain parity.  A draw in which a loaded channel has a non-finite pIC50 or Hill is counted
apart.  The default weights are a CONVENTION, not a measurement: +1 for the repolarising currents (hERG, KvLQT1_mink, Kv4.3, Kir2.1),
-1 for the depolarising ones (Nav1.5-peak, Nav1.5-late, Cav1.2), 0 for any other name — repolarising minus depolarising block, after
the "Bnet" of Mistry (2018).  The profile is the input of a cell model with its uncertainty; it is not an action-potential
prediction and not a risk category.

The tool reads, per channel, this package's or the reference's single-level chain files, `_all_chains.npy` files, hierarchical chain
files (chain_correlations.load_rows; the underlying effect, Hill = alpha and pIC50 = mu) and the two-column `*_hill_pic50_samples.txt`
files (a `#` header, then Hill, pIC50: the reference's chaste/samples and this package's alpha_mu_samples/), read as model 2.  Several
files of one channel are several chains; rows and chains beyond the shortest channel's are not used."""
import argparse
import ctypes as C
import json
import os

import numpy as np

from . import _lib, accumulator

DEFAULT_BINS = 4096
DEFAULT_MULTIPLES = (1.0, 3.0, 10.0)
MAX_DOSES, MAX_CHANNELS = 16, 16           # csrc/phf_drug_profile.h
WEIGHTS_NOTE = ("a convention, not a measurement: +1 repolarising currents (hERG, KvLQT1_mink, Kv4.3, Kir2.1), -1 depolarising currents "
                "(Nav1.5-peak, Nav1.5-late, Cav1.2), 0 any other name: repolarising minus depolarising block, after the Bnet of Mistry (2018)")
MULTIPLES_NOTE = "multiples of the clinical concentration Cmax; the default 1, 3, 10 is a convention"
METHOD = ("per post-burn-in draw (row r, chain c of every loaded channel side by side: the channels' posteriors are independent) and dose: "
          "percent block 100 (1 - 1/(1 + exp(Hill (ln c - ln IC50)))) of every channel (conductance scaling = 1 - block/100), net = "
          "SUM_k weight_k block_k in channel order, dominant = the first channel with the largest block; quantiles by the inverse "
          "empirical CDF from exact-count histograms ([lo, hi] holds the exact sample quantile), p_net_positive and "
          "dominant_probability from integer counts over the draws used; a draw with a non-finite pIC50 or Hill in a loaded channel "
          "is skipped; not an action-potential prediction, not a risk category")


# ---- the flags' values (no GPU, no library) --------------------------------------------------------------------------------------
def _positive_list(text, flag, most):
    try:
        vals = tuple(float(v) for v in str(text).split(",") if v.strip())
    except ValueError:
        raise ValueError("%s must be comma-separated numbers, got %r" % (flag, text))
    if not vals or len(vals) > most or not all(np.isfinite(v) and v > 0.0 for v in vals):
        raise ValueError("%s must be 1 to %d numbers, all > 0, got %r" % (flag, most, text))
    return vals


def parse_concs(text, flag="--drug-profile-concs"):
    """'0.045,0.45' -> concentrations in uM, at most 16"""
    return _positive_list(text, flag, MAX_DOSES)


def parse_multiples(text, flag="--drug-profile-multiples"):
    return _positive_list(text, flag, MAX_DOSES)


def parse_weights(text):
    """'hERG=1,Cav1.2=-0.5' -> {name: weight} (raises ValueError)"""
    out = {}
    for part in str(text).split(","):
        if not part.strip():
            continue
        name, eq, w = part.rpartition("=")
        try:
            val = float(w)
        except ValueError:
            val = float("nan")
        if not eq or not name.strip() or not np.isfinite(val):
            raise ValueError("--drug-profile-weights takes name=w,...: %r" % part)
        out[name.strip()] = val
    if not out:
        raise ValueError("--drug-profile-weights names no channel")
    return out


def check_bins(bins):
    b = int(bins)
    if b < 64 or b > 32768 or b & (b - 1):
        raise ValueError("--drug-profile-bins must be a power of two in [64, 32768], got %d" % b)
    return b


def read_cmax(path):
    """a file like the reference's chaste/drug_list.txt — a header line, then `Drug EFTPCmax(nM) [anything]` — -> {drug: Cmax in uM}"""
    out = {}
    with open(path) as f:
        lines = f.read().splitlines()
    for n, line in enumerate(lines[1:], 2):
        parts = line.split()
        if not parts:
            continue
        try:
            nm = float(parts[1])
        except (IndexError, ValueError):
            raise ValueError("%s line %d: expected `Drug EFTPCmax(nM) ...`, got %r" % (path, n, line))
        if not (np.isfinite(nm) and nm > 0.0):
            raise ValueError("%s line %d: Cmax must be > 0 nM, got %r" % (path, n, parts[1]))
        out[parts[0]] = nm / 1000.0
    return out


def doses_of(drug, concs, cmax, multiples):
    """the doses (uM) of a drug: the multiples of its Cmax, then the named concentrations; None when it has neither"""
    doses = []
    if cmax is not None and drug in cmax:
        doses += [m * cmax[drug] for m in multiples]
    doses += list(concs or ())
    if len(doses) > MAX_DOSES:
        raise ValueError("at most %d doses per drug (multiples of Cmax and named concentrations together), got %d" % (MAX_DOSES, len(doses)))
    return doses or None


def default_weights(channels, overrides=None):
    """the weight of every channel: the override by name, else the default by name (csrc/phf_drug_profile.h)"""
    lib = _lib.load()
    overrides = overrides or {}
    unknown = sorted(set(overrides) - set(channels))
    if unknown:
        raise ValueError("--drug-profile-weights names channels that are not there: %s" % ", ".join(unknown))
    return np.array([overrides.get(ch, lib.phf_drug_profile_default_weight(ch.encode())) for ch in channels], dtype=np.float64)


class Plan(object):
    """what a run profiles: from the (drug, channel) of each problem, the drugs with doses (in first-appearance order), those skipped
    for want of a Cmax, the channel places (the data file's channel order, restricted to the channels some problem has), the
    drug x channel -> problem map (-1: not loaded), the doses [drugs][D] and the weights [K]"""

    def __init__(self, pairs, channel_order, concs=None, cmax=None, multiples=DEFAULT_MULTIPLES, weights=None):
        have = {ch for _, ch in pairs}
        self.channels = [ch for ch in channel_order if ch in have] + sorted(have - set(channel_order))
        if len(self.channels) > MAX_CHANNELS:
            raise ValueError("the drug profile holds at most %d channels, the run has %d" % (MAX_CHANNELS, len(self.channels)))
        self.drugs, self.skipped, self.doses = [], [], []
        for drug, _ in pairs:
            if drug in self.drugs or drug in self.skipped:
                continue
            d = doses_of(drug, concs, cmax, multiples)
            if d is None:
                self.skipped.append(drug)
            else:
                self.drugs.append(drug); self.doses.append(d)
        D = max([len(d) for d in self.doses] or [0])                      # a drug named in no Cmax file has the named doses only
        self.doses = [d + [np.nan] * (D - len(d)) for d in self.doses]
        self.cmax = [None if cmax is None else cmax.get(d) for d in self.drugs]
        self.multiples = list(multiples) if cmax is not None else []
        self.map = np.full((len(self.drugs), len(self.channels)), -1, dtype=np.int32)
        for p, (drug, ch) in enumerate(pairs):
            if drug in self.drugs:
                self.map[self.drugs.index(drug), self.channels.index(ch)] = p
        self.weights = default_weights(self.channels, weights) if self.drugs else np.zeros(len(self.channels))
        self.doses = np.array(self.doses, dtype=np.float64).reshape(len(self.drugs), -1)

    def first_problem(self, d):
        return int(min(p for p in self.map[d] if p >= 0))


def workspace_bytes(num_drugs, num_channels, num_doses, bins=DEFAULT_BINS):
    """device bytes DrugProfile holds (raises on an invalid shape)"""
    return accumulator.workspace_bytes("phf_drug_profile_workspace_bytes", num_drugs, num_channels, num_doses, bins)


class DrugProfile(accumulator.RowAccumulator):
    """Streaming profile of `drugs` drugs over the single-level rows [n][num_problems][stride][chains] of model 1 | 2.
    channel_problem [drugs][K] (int, -1: not loaded), weights [K], doses [drugs][D] in uM."""

    tensors = ("ws", "map", "weights", "ln_doses")

    def __init__(self, model, num_problems, chains, channel_problem, weights, doses, total_rows, probs, bins=DEFAULT_BINS, device="cuda"):
        import torch
        from .quantiles import parse_probs
        accumulator.RowAccumulator.__init__(self, device)
        if model not in (1, 2):
            raise ValueError("the drug profile needs the single-level model 1 or 2")
        cp = np.ascontiguousarray(channel_problem, dtype=np.int32)
        ds = np.ascontiguousarray(doses, dtype=np.float64)
        w = np.ascontiguousarray(weights, dtype=np.float64)
        if cp.ndim != 2 or ds.ndim != 2 or ds.shape[0] != cp.shape[0] or w.shape != (cp.shape[1],):
            raise ValueError("channel_problem must be [drugs][K], doses [drugs][D] and weights [K]")
        if not (np.all((ds > 0.0) & ~np.isinf(ds) | np.isnan(ds)) and np.all(np.isfinite(ds[:, 0])) and np.all(np.isfinite(w))):
            raise ValueError("doses must be > 0 and finite (NaN: a place the drug does not use, never the first), weights finite")
        if np.any(cp >= int(num_problems)):
            raise ValueError("channel_problem names a problem beyond num_problems = %d" % num_problems)
        self.model, self.Q, self.C, self.N, self.B = int(model), int(num_problems), int(chains), int(total_rows), check_bins(bins)
        self.drugs, self.K = cp.shape
        self.D = ds.shape[1]
        self.min_cols = self.model
        self.probs = parse_probs(",".join(repr(float(p)) for p in probs))
        self.loaded = cp >= 0
        self.map = torch.from_numpy(np.where(cp >= 0, cp, -1).astype(np.int32)).to(self.device)
        self.weights = torch.from_numpy(w).to(self.device)
        self.ln_doses = torch.from_numpy(np.log(ds)).to(self.device)
        self.doses, self.w = ds, w
        shape = (self.drugs, self.K, self.D, self.B)
        self.tally_offset = int(self.lib.phf_drug_profile_tally_offset(*shape))
        self._init_workspace(workspace_bytes(*shape), "phf_drug_profile_init", *shape)

    def _accumulate(self, rows, n):
        from .sampler import _ptr, _stream_ptr
        step = max(1, (2 ** 31 - 1) // self.C)                 # rows x chains < 2^31 per call
        for r0 in range(0, n, step):
            part = rows[r0:r0 + step]
            _lib.check(self.lib.phf_drug_profile_accumulate(_ptr(part), part.shape[0], self.Q, rows.shape[2], self.C, self.model,
                                                            self.drugs, self.K, self.D, _ptr(self.map), _ptr(self.weights),
                                                            _ptr(self.ln_doses), self.B, self.rows_seen + r0, self.N, _ptr(self.ws),
                                                            C.c_size_t(self.nbytes), _stream_ptr(self.device)),
                       "phf_drug_profile_accumulate")

    def counts(self):
        """(histograms uint64 [drugs][D][K + 1][B], non-finite counts [drugs][D][K + 1], tallies [drugs][D][2][K + 3])"""
        import torch
        S = self.drugs * self.D * (self.K + 1)
        raw = self.ws.view(torch.int64).cpu().numpy().view(np.uint64)
        hist = raw[:S * self.B].reshape(self.drugs, self.D, self.K + 1, self.B)
        nf = raw[S * self.B + S * 8:S * self.B + S * 9].reshape(self.drugs, self.D, self.K + 1)
        t0 = self.tally_offset // 8
        tally = raw[t0:t0 + self.drugs * self.D * 2 * (self.K + 3)].reshape(self.drugs, self.D, 2, self.K + 3)
        return hist, nf, tally

    def result(self):
        """the reduce of every slot in the form quantiles.column_record reads — arrays [drugs][D (K + 1)] and [..][P] — plus
        "tally" [drugs][D][2][K + 3] (int64) and the profile's own facts"""
        import torch
        from .quantiles import HEAD, PER_PROB
        from .sampler import _ptr, _stream_ptr
        S, P = self.drugs * self.D * (self.K + 1), len(self.probs)
        out = torch.empty((S, HEAD + PER_PROB * P), dtype=torch.float64, device=self.device)
        probs = (C.c_double * P)(*self.probs)
        _lib.check(self.lib.phf_drug_profile_reduce(self.drugs, self.K, self.D, self.B, probs, P, _ptr(self.ws), C.c_size_t(self.nbytes),
                                                    _ptr(out), _stream_ptr(self.device)), "phf_drug_profile_reduce")
        red = out.cpu().numpy().reshape(self.drugs, self.D * (self.K + 1), HEAD + PER_PROB * P)
        per = red[..., HEAD:].reshape(self.drugs, self.D * (self.K + 1), P, PER_PROB)
        return {"min": red[..., 0], "max": red[..., 1], "draws": red[..., 2], "non_finite": red[..., 3], "bin_width": red[..., 4],
                "level": red[..., 5], "value": per[..., 0], "lo": per[..., 1], "hi": per[..., 2], "bin": per[..., 3],
                "probs": np.array(self.probs), "tally": self.counts()[2].astype(np.int64), "K": self.K, "D": self.D, "bins": self.B,
                "model": self.model, "chains": self.C, "rows": self.rows_seen, "loaded": self.loaded, "doses": self.doses,
                "weights": self.w}


# ---- records ---------------------------------------------------------------------------------------------------------------------
def _tally_record(t, channels, loaded):
    """t [K + 3] integer tallies -> counts and probabilities over the draws used"""
    K = len(channels)
    used = int(t[K + 1])
    frac = (lambda n: int(n) / used) if used else (lambda n: None)
    return {"draws_used": used, "draws_skipped": int(t[K + 2]), "net_positive_draws": int(t[K]), "p_net_positive": frac(t[K]),
            "dominant_draws": {ch: int(t[k]) for k, ch in enumerate(channels) if loaded[k]},
            "dominant_probability": {ch: frac(t[k]) for k, ch in enumerate(channels) if loaded[k]}}


def json_record(res, d, drug, channels, cmax=None, multiples=()):
    """the profile of drug d of a result(): one object per dose with the quantiles of every loaded channel's block and of the net
    block, the tallies over all draws and by chain parity"""
    from .quantiles import column_record
    K, D = int(res["K"]), int(res["D"])
    loaded = [bool(v) for v in res["loaded"][d]]
    doses = []
    for j in range(D):
        if not np.isfinite(res["doses"][d, j]):
            continue
        t = res["tally"][d, j]
        rec = {"dose_uM": float(res["doses"][d, j]),
               "block": {ch: column_record(res, d, j * (K + 1) + k) for k, ch in enumerate(channels) if loaded[k]},
               "net": column_record(res, d, j * (K + 1) + K)}
        rec.update(_tally_record(t[0] + t[1], channels, loaded))
        rec["by_chain_parity"] = {"even": _tally_record(t[0], channels, loaded), "odd": _tally_record(t[1], channels, loaded)}
        doses.append(rec)
    return {"drug": drug, "model": int(res["model"]), "chains": int(res["chains"]), "rows": int(res["rows"]),
            "channels": list(channels), "channels_loaded": [ch for k, ch in enumerate(channels) if loaded[k]],
            "weights": {ch: float(res["weights"][k]) for k, ch in enumerate(channels)}, "weights_note": WEIGHTS_NOTE,
            "cmax_uM": cmax, "cmax_multiples": list(multiples) if cmax is not None else [], "multiples_note": MULTIPLES_NOTE,
            "probs": [float(p) for p in res["probs"]], "bins": int(res["bins"]), "doses": doses, "method": METHOD}


def net_width95(rec):
    """the width of the 95 % interval of the net block at the record's first dose, or None without one"""
    ci = rec["doses"][0]["net"].get("ci95")
    return None if ci is None or ci[0] is None or ci[1] is None else ci[1] - ci[0]


def report_line(rank, records, skipped=()):
    """one line per rank: the drugs profiled, the one with the widest 95 % interval of the net block at its first dose, the drugs
    skipped for want of a Cmax"""
    line = "drug-profile [rank {}]: {} drugs".format(rank, len(records))
    wide = [(w, r["drug"]) for r in records for w in [net_width95(r)] if w is not None]
    if wide:
        w, drug = max(wide)
        first = next(r for r in records if r["drug"] == drug)["doses"][0]
        line += "; widest 95 % interval of the net block at the first dose: {} at {:.4g} uM, [{:.2f}, {:.2f}] percentage points".format(
            drug, first["dose_uM"], *first["net"]["ci95"])
    elif records:
        line += "; no 95 % interval (0.025 and 0.975 are not among the probabilities)"
    line += "; {} draws skipped".format(sum(r["doses"][0]["draws_skipped"] for r in records))
    if skipped:
        line += "; skipped, no Cmax: " + ", ".join(skipped)
    return line


# ---- chain files on disk ---------------------------------------------------------------------------------------------------------
def load_channel_file(path, hierarchical=False):
    """(pIC50 [rows][chains], Hill [rows][chains] or None for a model-1 file, kind)"""
    from . import chain_correlations as cc
    if not path.endswith(".npy"):
        table = np.loadtxt(path, ndmin=2)
        if table.shape[1] == 2:                                  # `# N (alpha,mu) samples ...`, then Hill, pIC50
            return table[:, 1:2], table[:, 0:1], "hill pic50 samples"
    rows, kind = cc.load_rows(path, hierarchical)
    if hierarchical or kind == "hierarchical text":
        if rows.shape[1] < 4:
            raise SystemExit("%s: a hierarchical chain has at least the columns alpha, beta, mu, s" % path)
        return rows[:, 2, :], rows[:, 0, :], "hierarchical (Hill = alpha, pIC50 = mu)"
    if rows.shape[1] == 3:
        return rows[:, 0, :], None, kind + ", model 1"
    if rows.shape[1] == 4:
        return rows[:, 0, :], rows[:, 1, :], kind + ", model 2"
    raise SystemExit("%s: %d columns are no single-level chain (3 or 4) and no Hill, pIC50 sample file (2)" % (path, rows.shape[1]))


def load_channels(named_files, hierarchical=False):
    """named_files: [(channel, [files])] -> (model, pIC50 [rows][K][chains], Hill likewise, facts of what was read and dropped)"""
    per, facts = [], {}
    for name, files in named_files:
        parts = [load_channel_file(f, hierarchical) for f in files]
        n = min(p[0].shape[0] for p in parts)
        pic50 = np.concatenate([p[0][:n] for p in parts], axis=1)
        hill = np.concatenate([np.ones_like(p[0][:n]) if p[1] is None else p[1][:n] for p in parts], axis=1)
        per.append((pic50, hill, all(p[1] is None for p in parts)))
        facts[name] = {"files": list(files), "kinds": [p[2] for p in parts], "rows": int(n), "chains": int(pic50.shape[1])}
    n, c = min(p[0].shape[0] for p in per), min(p[0].shape[1] for p in per)
    for name, _ in named_files:
        facts[name].update(rows_dropped=facts[name]["rows"] - n, chains_dropped=facts[name]["chains"] - c)
    model = 1 if all(p[2] for p in per) else 2
    return (model, np.stack([p[0][:n, :c] for p in per], axis=1), np.stack([p[1][:n, :c] for p in per], axis=1),
            {"rows_used": int(n), "chains_used": int(c), "files_by_channel": facts})


def profile_of_draws(model, pic50, hill, channels, doses, weights=None, probs=None, bins=DEFAULT_BINS, device="cuda:0", drug="drug",
                     cmax=None, multiples=()):
    """pic50, hill [rows][K][chains] of ONE drug's K channels (hill None: model 1) -> its json_record, through the same entry points"""
    import torch
    from .quantiles import DEFAULT_PROBS
    pic50 = np.asarray(pic50, dtype=np.float64)
    n, K, c = pic50.shape
    rows = np.zeros((n, K, 2, c))
    rows[:, :, 0] = pic50
    rows[:, :, 1] = 1.0 if hill is None else np.asarray(hill, dtype=np.float64)
    w = default_weights(channels, weights)
    acc = DrugProfile(model, K, c, np.arange(K)[None, :], w, np.asarray(doses, dtype=np.float64)[None, :], n,
                      DEFAULT_PROBS if probs is None else probs, bins, device)
    acc.accumulate(torch.from_numpy(rows).to(acc.device))
    res = acc.result()
    acc.free()
    return json_record(res, 0, drug, channels, cmax, multiples)


def build_parser():
    ap = argparse.ArgumentParser(prog="drug_profile")
    ap.add_argument("--channel", action="append", required=True, metavar="NAME=FILE[,FILE...]", help="the chain files of one channel; "
                    "several files are several chains; repeat the flag per channel, in the order the net block is summed in")
    ap.add_argument("--concs", type=str, default=None, metavar="c1,c2,...", help="concentrations in uM")
    ap.add_argument("--cmax-nM", type=float, default=None, metavar="X", help="the clinical concentration in nM; the doses are its --multiples")
    ap.add_argument("--multiples", type=str, default=None, metavar="m1,...", help="multiples of --cmax-nM (default 1,3,10, a convention)")
    ap.add_argument("--weights", type=str, default=None, metavar="name=w,...", help="weights of the net block instead of the defaults by name")
    ap.add_argument("--quantile-probs", type=str, default=None)
    ap.add_argument("--bins", type=int, default=DEFAULT_BINS)
    ap.add_argument("--hierarchical", action="store_true", default=False, help="the chain files are hierarchical chain files")
    ap.add_argument("--drug", type=str, default="drug", help="the name the record carries")
    ap.add_argument("--device", default="cuda:0")
    return ap


def parse_tool_args(ap, argv=None):
    """-> (args, [(channel, files)], doses in uM, cmax in uM or None, multiples, weights or None, probs or None); refusals need no GPU"""
    from .quantiles import parse_probs
    a = ap.parse_args(argv)
    named = []
    for text in a.channel:
        name, eq, files = text.partition("=")
        if not eq or not name or not files:
            ap.error("--channel takes NAME=FILE[,FILE...], got %r" % text)
        if name in [n for n, _ in named]:
            ap.error("--channel names %s twice (several files of one channel: NAME=FILE,FILE)" % name)
        named.append((name, [f for f in files.split(",") if f]))
    if a.concs is None and a.cmax_nM is None:
        ap.error("one of --concs and --cmax-nM is needed")
    if a.multiples is not None and a.cmax_nM is None:
        ap.error("--multiples needs --cmax-nM")
    try:
        if a.cmax_nM is not None and not (np.isfinite(a.cmax_nM) and a.cmax_nM > 0):
            raise ValueError("--cmax-nM must be > 0")
        multiples = DEFAULT_MULTIPLES if a.multiples is None else parse_multiples(a.multiples, "--multiples")
        cmax = None if a.cmax_nM is None else {a.drug: a.cmax_nM / 1000.0}
        doses = doses_of(a.drug, parse_concs(a.concs, "--concs") if a.concs is not None else None, cmax, multiples)
        weights = None if a.weights is None else parse_weights(a.weights)
        probs = None if a.quantile_probs is None else parse_probs(a.quantile_probs)
        a.bins = check_bins(a.bins)
        if len(named) > MAX_CHANNELS:
            raise ValueError("at most %d channels" % MAX_CHANNELS)
        if weights is not None and set(weights) - {n for n, _ in named}:
            raise ValueError("--weights names channels that are not there: %s" % ", ".join(sorted(set(weights) - {n for n, _ in named})))
    except ValueError as e:
        ap.error(str(e))
    return a, named, doses, (None if cmax is None else cmax[a.drug]), multiples, weights, probs


def main(argv=None):
    a, named, doses, cmax, multiples, weights, probs = parse_tool_args(build_parser(), argv)
    for _, files in named:
        for f in files:
            if not os.path.exists(f):
                raise SystemExit("no such file: %s" % f)
    model, pic50, hill, facts = load_channels(named, a.hierarchical)
    rec = profile_of_draws(model, pic50, hill, [n for n, _ in named], doses, weights, probs, a.bins, a.device, a.drug, cmax, multiples)
    print(json.dumps(dict(rec, **facts)))


if __name__ == "__main__":
    main()
