"""Posterior quantiles of chains already on disk (pyhillfit_amd/quantiles.py).

    python -m pyhillfit_amd.chain_quantiles FILE... [--probs 0.025,...,0.975] [--bins 16384] [--exact] [--device cuda:0]

FILE is read as by chain_diagnostics: a `<chain file>_all_chains.npy` of --save-all-chains ([rows][columns][chains], burn-in
removed) or a reference-format chain text file (a hierarchical one, recognised by its header, loses its first quarter here).
Without --exact the histograms are accumulated on the GPU (phf_quantiles_accumulate), like the command lines' --quantiles; with
--exact every column is sorted on the host, np.quantile(method="inverted_cdf"): the ground truth the device brackets hold.
One JSON object per file on stdout."""
import argparse
import json
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


def main(argv=None):
    ap = argparse.ArgumentParser(prog="chain_quantiles")
    ap.add_argument("files", nargs="+")
    ap.add_argument("--probs", default=",".join(str(p) for p in qn.DEFAULT_PROBS), help="probabilities, comma-separated")
    ap.add_argument("--bins", type=int, default=qn.DEFAULT_BINS, help="histogram bins per column, a power of two")
    ap.add_argument("--exact", action="store_true", help="sort on the host instead (np.quantile, method='inverted_cdf')")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    probs = qn.parse_probs(a.probs)
    out = []
    for p in a.files:
        rec = quantiles_file(p, probs, qn.check_bins(a.bins), a.exact, a.device)
        out.append(rec)
        print(json.dumps(rec))
        sys.stdout.flush()
    return out


if __name__ == "__main__":
    main()
