"""Posterior correlations and the multivariate R-hat of chains already on disk (pyhillfit_amd/correlations.py).

    python -m pyhillfit_amd.chain_correlations FILE... [--hierarchical] [--device cuda:0]

FILE is read as by chain_diagnostics: a `<chain file>_all_chains.npy` of --save-all-chains ([rows][columns][chains], burn-in removed)
or a reference-format chain text file holding one chain, this package's or the reference's own: single-level and tempered files have
their burn-in removed already; a hierarchical file (recognised by its header, or named so with --hierarchical) holds the whole chain,
and its first quarter is dropped here as construct_hierarchical_cdfs.py does.  Several files are several chains of ONE posterior: they
must have the same columns, and rows beyond the shortest file's are not used.  The last column, the log-target, is left out.  A
single chain still gives two half-chains, so the multivariate R-hat is defined for the reference's own chain files.  One JSON object
on stdout.  The accumulation runs on the GPU (phf_comoments_accumulate), like the command lines' --correlations."""
import argparse
import json

import numpy as np

from . import chainio
from . import correlations as cr


def load_rows(path, hierarchical=False):
    """(rows [rows][columns][chains] with the burn-in removed, kind)"""
    if path.endswith(".npy"):
        return np.asarray(np.load(path), dtype=np.float64), "all chains"
    with open(path) as f:
        first = f.readline()
    rows = chainio.load_chain(path)
    if hierarchical or first == chainio.HIERARCHICAL_HEADER[0]:
        return rows[len(rows) // 4:, :, None], "hierarchical text"                # construct_hierarchical_cdfs.py: burn = len // 4
    return rows[:, :, None], "text"


def column_names(d, hierarchical):
    """the names of the d parameter columns of a chain file"""
    if hierarchical and d >= 7 and (d - 5) % 2 == 0:
        from .hierarchical import hierarchical_columns
        return hierarchical_columns((d - 5) // 2)[:d]
    if not hierarchical and d in (2, 3):
        return ["pIC50", "sigma"] if d == 2 else ["pIC50", "Hill", "sigma"]
    return ["column_%d" % i for i in range(d)]


def load_draws(paths, hierarchical=False):
    """(draws [rows][d][chains] of all files side by side, their column names, the files' kinds)"""
    loaded = [load_rows(p, hierarchical) for p in paths]
    cols = {r.shape[1] for r, _ in loaded}
    if len(cols) != 1:
        raise SystemExit("the files have different numbers of columns: %s" % sorted(cols))
    n = min(r.shape[0] for r, _ in loaded)
    draws = np.concatenate([r[:n, :-1] for r, _ in loaded], axis=2)
    kinds = [k for _, k in loaded]
    return draws, column_names(draws.shape[1], hierarchical or "hierarchical text" in kinds), kinds


def correlations_of_files(paths, hierarchical=False, device="cuda:0"):
    draws, names, kinds = load_draws(paths, hierarchical)
    rec = cr.json_record(cr.correlations_of_draws(draws, names, device))
    return dict({"files": list(paths), "kinds": kinds, "rows": int(draws.shape[0]), "chains": int(draws.shape[2])}, **rec)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="chain_correlations")
    ap.add_argument("files", nargs="+")
    ap.add_argument("--hierarchical", action="store_true", default=False, help="the files are hierarchical chain files")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    print(json.dumps(correlations_of_files(a.files, a.hierarchical, a.device)))


if __name__ == "__main__":
    main()
