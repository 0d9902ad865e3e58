"""Posterior quantiles of chains already on disk (pyhillfit_amd/quantiles.py).

    python -m pyhillfit_amd.chain_quantiles FILE... [--probs 0.025,...,0.975] [--bins 16384] [--exact] [--device cuda:0]

FILE is read as by chain_diagnostics: a `<chain file>_all_chains.npy` of --save-all-chains ([rows][columns][chains], burn-in
removed) or a reference-format chain text file (a hierarchical one, recognised by its header, loses its first quarter here).
Without --exact the histograms are accumulated on the GPU (phf_quantiles_accumulate), like the command lines' --quantiles; with
--exact every column is sorted on the host, np.quantile(method="inverted_cdf"): the ground truth the device brackets hold.
One JSON object per file on stdout.

    python -m pyhillfit_amd.chain_quantiles FILE... --hier-bands G --data-file F [--band-concs c1,c2,...] [--seed 25] [--problem-id N]
                                            [--drug D --channel C]

FILE is a hierarchical chain text file (this package's or the reference's): the dose-response bands of the hierarchical model
(quantiles.py, "Hierarchical bands") at G grid doses and the named concentrations, as the command line's --predictive-bands.  The
pair is found from the file name (`<data>_<drug>_<channel>_hierarchical_chain.txt`) unless named; the stream uses chain id 0, rows
indexed from the first post-burn-in row, --seed and the pair's problem id (by default its index in the data file's drug x channel
product, as the command lines number it): given a one-chain run's --seed, this reproduces its "hierarchical_bands" object exactly."""
import argparse
import itertools as it
import json
import os
import sys

import numpy as np

from . import quantiles as qn
from .chain_diagnostics import load_rows


def quantiles_file(path, probs=qn.DEFAULT_PROBS, bins=qn.DEFAULT_BINS, exact=False, device="cuda:0"):
    rows, kind = load_rows(path)
    probs = tuple(probs)
    rec = {"file": path, "kind": kind, "rows": int(rows.shape[0]), "chains": int(rows.shape[2]), "probs": list(probs)}
    if exact:
        rec["method"] = "exact: np.quantile(method='inverted_cdf') of every column's finite draws"
        q = qn.exact_quantiles(rows, probs)
        rec["columns"] = [{"value": [qn._num(v) for v in q[c]]} for c in range(q.shape[0])]
        for c, col in enumerate(rec["columns"]):
            col.update(qn._intervals(list(probs), q[c], q[c], q[c]))
        return rec
    res = qn.quantiles_of_draws(rows, probs, bins, device)
    res = {k: (v[None] if isinstance(v, np.ndarray) and k not in ("probs",) else v) for k, v in res.items()}
    rec["method"] = qn.METHOD
    rec["bins"] = int(bins)
    rec["columns"] = [qn.column_record(res, 0, c) for c in range(rows.shape[1])]
    return rec


def pair_of_file_name(path, drugs, channels):
    """the (drug, channel) of the data file whose cleaned names end a hierarchical chain file's name"""
    from . import doseresponse as dr
    base = os.path.basename(path)
    hits = [(d, c) for d, c in it.product(drugs, channels)
            if base.endswith("_{}_{}_hierarchical_chain.txt".format(dr._clean(d), dr._clean(c)))]
    if not hits:
        raise SystemExit("{}: no drug + channel of the data file in the file name; name the pair with --drug and --channel".format(path))
    return max(hits, key=lambda h: len(h[0]) + len(h[1]))           # the longest match: a name may end with another


def hier_bands_file(path, grid, named=(), probs=qn.DEFAULT_PROBS, bins=qn.DEFAULT_BINS, seed=25, problem_id=None, drug=None,
                    channel=None, device="cuda:0"):
    """dr.setup(data file) first.  The record of one hierarchical chain text file, "hierarchical_bands" as the command line writes it"""
    import torch
    from . import doseresponse as dr
    from .PyHillFit import experiments_and_labels
    rows, kind = load_rows(path)
    if kind != "hierarchical text":
        raise SystemExit("{}: --hier-bands reads hierarchical chain text files".format(path))
    if not drug or not channel:
        drug, channel = pair_of_file_name(path, dr.drugs, dr.channels)
    ne = (rows.shape[1] - 6) // 2
    expts = experiments_and_labels(drug, channel, ne)[0]
    doses = qn.band_doses(np.concatenate([np.asarray(e)[:, 0] for e in expts]), grid, named)
    if problem_id is None:
        problem_id = list(it.product(dr.drugs, dr.channels)).index((drug, channel))
    q = qn.PosteriorQuantiles(1, 1, 4, rows.shape[0], probs, bins, device, band_ln_doses=np.log(doses)[None], seed=seed,
                              problem_ids=[problem_id], chain_id_base=0)
    q.accumulate(torch.from_numpy(np.ascontiguousarray(rows[:, None, :4, :])).to(q.device))
    res = q.result()
    q.free()
    return {"file": path, "kind": kind, "drug": drug, "channel": channel, "num_expts": ne, "rows": int(rows.shape[0]), "chains": 1,
            "problem_id": int(problem_id), "chain_id_base": 0, "bins": int(bins),
            "hierarchical_bands": qn.hier_band_record(res, 0, doses, grid)}


def main(argv=None):
    ap = argparse.ArgumentParser(prog="chain_quantiles")
    ap.add_argument("files", nargs="+")
    ap.add_argument("--probs", default=",".join(str(p) for p in qn.DEFAULT_PROBS), help="probabilities, comma-separated")
    ap.add_argument("--bins", type=int, default=qn.DEFAULT_BINS, help="histogram bins per column, a power of two")
    ap.add_argument("--exact", action="store_true", help="sort on the host instead (np.quantile, method='inverted_cdf')")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--hier-bands", type=int, default=0, metavar="G", help="hierarchical chain text files: the bands of the underlying "
                    "effect and of a predicted future experiment at G grid doses instead of the columns' quantiles (needs --data-file)")
    ap.add_argument("--band-concs", default=None, metavar="c1,c2,...", help="--hier-bands: named concentrations (uM) after the grid")
    ap.add_argument("--data-file", default=None, help="--hier-bands: csv or json data file the chains were fitted to")
    ap.add_argument("--seed", type=int, default=25, help="--hier-bands: key of the future experiment's random stream (a run's --seed)")
    ap.add_argument("--problem-id", type=int, default=None, help="--hier-bands: the pair's problem id in the stream (default: its index "
                    "in the data file's drug x channel product)")
    ap.add_argument("--drug", default=None)
    ap.add_argument("--channel", default=None)
    a = ap.parse_args(argv)
    probs = qn.parse_probs(a.probs)
    if a.hier_bands < 0:
        ap.error("--hier-bands must be >= 1")
    named = ()
    if a.band_concs is not None:
        if not a.hier_bands:
            ap.error("--band-concs needs --hier-bands")
        try:
            named = qn.parse_band_concs(a.band_concs)
        except ValueError as e:
            ap.error(str(e))
    if a.hier_bands:
        if a.exact:
            ap.error("--exact does not go with --hier-bands (the bands are accumulated on the GPU)")
        if not a.data_file:
            ap.error("--hier-bands needs --data-file")
        from . import doseresponse as dr
        dr.setup(a.data_file)
    out = []
    for p in a.files:
        if a.hier_bands:
            rec = hier_bands_file(p, a.hier_bands, named, probs, qn.check_bins(a.bins), a.seed, a.problem_id, a.drug, a.channel, a.device)
        else:
            rec = quantiles_file(p, probs, qn.check_bins(a.bins), a.exact, a.device)
        out.append(rec)
        print(json.dumps(rec))
        sys.stdout.flush()
    return out


if __name__ == "__main__":
    main()
