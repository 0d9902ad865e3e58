"""Posterior predictive checks of chains already on disk (pyhillfit_amd/ppc.py), as chain_waic does for WAIC.

    python -m pyhillfit_amd.chain_ppc --data-file F FILE... [--drug D --channel C] [--model 1|2] [--seed 25] [--problem-id Q]
                                      [--chain-id-base 0] [--device cuda:0]

FILE is what chain_waic reads: a `<chain file>_all_chains.npy` of --save-all-chains or a reference-format chain text file
(single-level or hierarchical).  The replicates depend on the seed, the problem id and the chains' ids: given a command-line run's
--seed, the pair's problem id (by default its index in the data file's drug x channel product, which is what the command lines use)
and chain id base 0, the check of that run's .npy reproduces its "ppc" record exactly.  One JSON object per file on stdout; the
accumulation runs on the GPU (phf_ppc_accumulate), like the command lines' --ppc."""
import argparse
import itertools as it
import json
import sys

from . import chain_waic as cw
from . import doseresponse as dr
from . import ppc as pp
from . import waic as wc
from .PyHillFit import experiments_and_labels


def ppc_file(path, drug=None, channel=None, model=None, seed=25, problem_id=None, chain_id_base=0, device="cuda:0"):
    rows, kind, drug, channel, model = cw.load(path, drug, channel, model)
    if kind == "hierarchical text":
        ne = (rows.shape[1] - 6) // 2
        expts, labels = experiments_and_labels(drug, channel, ne)
        pts, lik = wc.Points.hierarchical([expts], [labels]), "hierarchical"
    else:
        if model not in (1, 2):
            raise SystemExit("{}: model must be 1 or 2".format(path))
        expts, labels = experiments_and_labels(drug, channel)
        pts, lik = wc.Points.single_level([expts], [labels]), model
    if problem_id is None:
        problem_id = list(it.product(dr.drugs, dr.channels)).index((drug, channel))
    res = pp.ppc_of_draws(pts, lik, rows[:, :wc.columns_read(lik, pts)], seed, problem_id, chain_id_base, device)
    rec = pp.json_record(res, pts, 0)
    return dict({"file": path, "kind": kind, "drug": drug, "channel": channel, "model": "hierarchical" if lik == "hierarchical" else lik,
                 "rows": int(rows.shape[0]), "chains": int(rows.shape[2]), "seed": seed, "problem_id": problem_id,
                 "chain_id_base": chain_id_base}, **rec)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="chain_ppc")
    ap.add_argument("files", nargs="+")
    ap.add_argument("--data-file", required=True, help="csv or json data file the chains were fitted to")
    ap.add_argument("--drug", default=None)
    ap.add_argument("--channel", default=None)
    ap.add_argument("--model", type=int, default=None, help="single-level model (1 | 2) if the file does not say")
    ap.add_argument("--seed", type=int, default=25, help="key of the replicates' random stream (a command-line run's --seed)")
    ap.add_argument("--problem-id", type=int, default=None, help="the pair's problem id in the stream (default: its index in the data "
                    "file's drug x channel product, as the command lines number it)")
    ap.add_argument("--chain-id-base", type=int, default=0, help="id of the file's chain 0 in the stream")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    dr.setup(a.data_file)
    for p in a.files:
        print(json.dumps(ppc_file(p, a.drug, a.channel, a.model, a.seed, a.problem_id, a.chain_id_base, a.device)))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
