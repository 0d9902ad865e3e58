"""WAIC of chains already on disk (pyhillfit_amd/waic.py), as chain_diagnostics does for the diagnostics.

    python -m pyhillfit_amd.chain_waic --data-file F FILE... [--drug D --channel C] [--model 1|2] [--device cuda:0]

FILE is a `<chain file>_all_chains.npy` of --save-all-chains ([rows][columns][chains], burn-in removed; single-level) or a
reference-format chain text file: single-level (burn-in removed already; the pair and the model are read from its header) or
hierarchical (recognised by its header; the whole chain, whose first quarter is dropped as construct_hierarchical_cdfs.py does;
Ne from the columns).  The pair of a .npy comes from the header of its chain text file beside it, the model from its columns;
--drug/--channel/--model override.  The data points come from --data-file.  One JSON object per file on stdout; the accumulation
runs on the GPU (phf_waic_accumulate), like the command lines' --waic."""
import argparse
import json
import os
import re
import sys

import numpy as np

from . import chainio
from . import doseresponse as dr
from . import waic as wc
from .PyHillFit import experiments_and_labels

_SL_HEADER = re.compile(r"# Nonhierarchical MCMC output for (.+) \+ (.+): \((.*)\)")


def _pair_of_header(line):
    m = _SL_HEADER.match(line.strip())
    return (m.group(1), m.group(2), 2 if "Hill" in m.group(3) else 1) if m else None


def _raw_name(clean, names):
    """data-file name of a (cleaned: '/' -> '_') name in a file header"""
    for n in names:
        if n == clean or dr._clean(n) == clean:
            return n
    raise SystemExit("{} is not in the data file".format(clean))


def load(path, drug=None, channel=None, model=None):
    """(draws [rows][columns][chains], kind, drug, channel, model or None)"""
    header = None
    if path.endswith(".npy"):
        rows = np.asarray(np.load(path), dtype=np.float64)
        txt = path[:-len("_all_chains.npy")] + ".txt" if path.endswith("_all_chains.npy") else None
        if txt and os.path.exists(txt):
            with open(txt) as f:
                header = _pair_of_header(f.readline())
        kind = "all chains"
        model = model or (rows.shape[1] - 2)                            # columns: theta, then the log-target
    else:
        with open(path) as f:
            first = f.readline()
        rows = chainio.load_chain(path)
        if first == chainio.HIERARCHICAL_HEADER[0]:
            rows, kind, model = rows[len(rows) // 4:, :, None], "hierarchical text", None
        else:
            header = _pair_of_header(first)
            rows, kind = rows[:, :, None], "text"
            model = model or (header[2] if header else rows.shape[1] - 2)
    if header:
        drug, channel = drug or header[0], channel or header[1]
    if not drug or not channel:
        raise SystemExit("{}: name the pair with --drug and --channel".format(path))
    return rows, kind, _raw_name(drug, dr.drugs), _raw_name(channel, dr.channels), model


def waic_file(path, drug=None, channel=None, model=None, device="cuda:0"):
    rows, kind, drug, channel, model = load(path, drug, channel, model)
    if kind == "hierarchical text":
        ne = (rows.shape[1] - 6) // 2
        expts, labels = experiments_and_labels(drug, channel, ne)
        pts, lik = wc.Points.hierarchical([expts], [labels]), "hierarchical"
    else:
        if model not in (1, 2):
            raise SystemExit("{}: model must be 1 or 2".format(path))
        expts, labels = experiments_and_labels(drug, channel)
        pts, lik = wc.Points.single_level([expts], [labels]), model
    res = wc.waic_of_draws(pts, lik, rows[:, :wc.columns_read(lik, pts)], device)
    rec = wc.json_record(res, pts, 0)
    return dict({"file": path, "kind": kind, "drug": drug, "channel": channel, "model": "hierarchical" if lik == "hierarchical" else lik,
                 "rows": int(rows.shape[0]), "chains": int(rows.shape[2])}, **rec)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="chain_waic")
    ap.add_argument("files", nargs="+")
    ap.add_argument("--data-file", required=True, help="csv or json data file the chains were fitted to")
    ap.add_argument("--drug", default=None)
    ap.add_argument("--channel", default=None)
    ap.add_argument("--model", type=int, default=None, help="single-level model (1 | 2) if the file does not say")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    dr.setup(a.data_file)
    for p in a.files:
        print(json.dumps(waic_file(p, a.drug, a.channel, a.model, a.device)))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
