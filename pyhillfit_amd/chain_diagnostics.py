"""Convergence diagnostics of chains already on disk (split-R-hat, multi-chain ESS, MCSE: pyhillfit_amd/diagnostics.py).

    python -m pyhillfit_amd.chain_diagnostics FILE... [--lags 256] [--batch-means] [--device cuda:0]

FILE is a `<chain file>_all_chains.npy` of --save-all-chains ([rows][columns][chains], burn-in removed) or a reference-format
chain text file holding one chain: single-level and tempered files have their burn-in removed already; a hierarchical file
(recognised by its header) holds the whole chain, and its first quarter is dropped here as construct_hierarchical_cdfs.py does.
A single chain still gives two half-chains, so split-R-hat is defined for the reference's own chain files.  One JSON object per
file on stdout.  The accumulation runs on the GPU (phf_diagnostics_accumulate), like the command lines' --diagnostics.
--batch-means adds the object "batch_means" (ESS and MCSE beyond the lag limit: pyhillfit_amd/batch_means.py), like the command lines'
--diagnostic-batch-means."""
import argparse
import json
import sys

import numpy as np

from . import chainio
from . import diagnostics as dg


def load_rows(path):
    """(rows [rows][columns][chains] with the burn-in removed, kind)"""
    if path.endswith(".npy"):
        return np.asarray(np.load(path), dtype=np.float64), "all chains"
    with open(path) as f:
        first = f.readline()
    rows = chainio.load_chain(path)
    if first == chainio.HIERARCHICAL_HEADER[0]:
        return rows[len(rows) // 4:, :, None], "hierarchical text"                # construct_hierarchical_cdfs.py: burn = len // 4
    return rows[:, :, None], "text"


def diagnose_file(path, lags=dg.DEFAULT_LAGS, device="cuda:0", batch_means=False):
    rows, kind = load_rows(path)
    res = dg.diagnose(rows, lags, device)
    rec = dg.json_record({k: v[None] for k, v in res.items()}, 0, lags, rows.shape[0], rows.shape[2])
    if batch_means:
        from . import batch_means as bm
        rec["batch_means"] = bm.json_record({k: v[None] for k, v in bm.diagnose(rows, device).items()}, 0)
    return dict({"file": path, "kind": kind, "rows": int(rows.shape[0]), "chains": int(rows.shape[2])}, **rec)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="chain_diagnostics")
    ap.add_argument("files", nargs="+")
    ap.add_argument("--lags", type=int, default=dg.DEFAULT_LAGS, help="lag limit K of the autocorrelation sums")
    ap.add_argument("--batch-means", action="store_true", default=False, help="also ESS and MCSE by batch means on a dyadic ladder")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    for p in a.files:
        print(json.dumps(diagnose_file(p, a.lags, a.device, a.batch_means)))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
