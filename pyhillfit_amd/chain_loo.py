"""PSIS-LOO of chains already on disk (pyhillfit_amd/loo.py), as chain_waic does for WAIC.

    python -m pyhillfit_amd.chain_loo --data-file F FILE... [--drug D --channel C] [--model 1|2] [--tail-per-chain K] [--device cuda:0]

FILE is a `<chain file>_all_chains.npy` of --save-all-chains ([rows][columns][chains], burn-in removed; single-level) or a
reference-format chain text file: single-level (burn-in removed already; the pair and the model are read from its header) or
hierarchical (recognised by its header; the whole chain, whose first quarter is dropped as construct_hierarchical_cdfs.py does;
Ne from the columns).  Files are read exactly as chain_waic reads them.  The data points come from --data-file.  One JSON object per
file on stdout; the accumulation and the Pareto smoothing run on the GPU (phf_psis_accumulate / phf_psis_reduce), like --loo."""
import argparse
import json
import sys

from . import doseresponse as dr
from . import loo as lo
from . import waic as wc
from .chain_waic import load
from .PyHillFit import experiments_and_labels


def loo_file(path, drug=None, channel=None, model=None, tail_per_chain=0, device="cuda:0"):
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
    res = lo.loo_of_draws(pts, lik, rows[:, :wc.columns_read(lik, pts)], device, tail_per_chain)
    rec = lo.json_record(res, pts, 0, res["tail_length"], res["tail_per_chain"])
    return dict({"file": path, "kind": kind, "drug": drug, "channel": channel, "model": "hierarchical" if lik == "hierarchical" else lik,
                 "rows": int(rows.shape[0]), "chains": int(rows.shape[2])}, **rec)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="chain_loo")
    ap.add_argument("files", nargs="+")
    ap.add_argument("--data-file", required=True, help="csv or json data file the chains were fitted to")
    ap.add_argument("--drug", default=None)
    ap.add_argument("--channel", default=None)
    ap.add_argument("--model", type=int, default=None, help="single-level model (1 | 2) if the file does not say")
    ap.add_argument("--tail-per-chain", type=int, default=0, help="smallest log-likelihoods kept per (point, chain); 0: the default rule")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    dr.setup(a.data_file)
    for p in a.files:
        print(json.dumps(loo_file(p, a.drug, a.channel, a.model, a.tail_per_chain, a.device)))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
