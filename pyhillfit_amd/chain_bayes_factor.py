"""Savage-Dickey Bayes factor B12 (Hill = 1 against Hill free) of model-2 chains already on disk (pyhillfit_amd/savage_dickey.py), as
chain_design and chain_sensitivity do for their analyses.

    python -m pyhillfit_amd.chain_bayes_factor --data-file F FILE... [--drug D --channel C] [--panels 32] [--every 1] [--device cuda:0]

FILE is read as by chain_waic: a `<chain file>_all_chains.npy` of PyHillFit -m 2 --save-all-chains ([rows][columns][chains], burn-in
removed) or a single-level model-2 chain text file in the reference's format, this package's or the reference's own (the pair from its
header).  SEVERAL files are several chains of ONE pair: their chains are put side by side (the rows cut to the shortest file), so
that independent runs of the reference give a between-chain standard error.  The sums are accumulated on the GPU by the kernel the
command line's --savage-dickey uses.  One JSON object on stdout."""
import argparse
import json
import sys

import numpy as np

from . import doseresponse as dr
from . import savage_dickey as sd


def build_parser():
    ap = argparse.ArgumentParser(prog="chain_bayes_factor")
    ap.add_argument("files", nargs="+")
    ap.add_argument("--data-file", required=True, help="csv or json data file the chains were fitted to")
    ap.add_argument("--drug", default=None)
    ap.add_argument("--channel", default=None)
    ap.add_argument("--panels", type=int, default=sd.DEFAULT_PANELS, metavar="P")
    ap.add_argument("--every", type=int, default=1, metavar="T")
    ap.add_argument("--device", default="cuda:0")
    return ap


def check_args(ap, a):
    try:
        a.panels = sd.check_panels(a.panels)
    except ValueError as e:
        ap.error(str(e).replace("--savage-dickey-", "--"))
    if a.every < 1:
        ap.error("--every must be >= 1")


def bayes_factor_files(paths, drug=None, channel=None, panels=sd.DEFAULT_PANELS, every=1, device="cuda:0"):
    from . import chain_waic as cw
    parts, kinds, pair = [], [], None
    for path in paths:
        rows, kind, d, c, model = cw.load(path, drug, channel, None)
        if kind == "hierarchical text":
            raise SystemExit("{}: a hierarchical chain file; the Savage-Dickey Bayes factor is single-level only".format(path))
        if model != 2 or rows.shape[1] != 4:
            raise SystemExit("{}: not a model-2 chain (pIC50, Hill, sigma, log-target): B12 is read off the Hill-free fit".format(path))
        if pair is not None and (d, c) != pair:
            raise SystemExit("{}: chains of {} + {}, the files before were of {} + {}".format(path, d, c, *pair))
        pair = (d, c)
        parts.append(rows)
        kinds.append(kind)
    n = min(p.shape[0] for p in parts)
    draws = np.concatenate([p[:n] for p in parts], axis=2)
    num_expts, _, experiments = dr.load_crumb_data(*pair)
    concs, responses = dr.concatenate_experiments(num_expts, experiments)
    res = sd.bayes_factor_of_draws(concs, responses, draws, panels, every, device)
    return dict({"files": list(paths), "kinds": kinds, "drug": pair[0], "channel": pair[1], "model": 2, "rows": int(n),
                 "chains": int(draws.shape[2])}, **sd.json_record(res))


def main(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    check_args(ap, a)
    dr.setup(a.data_file)
    rec = bayes_factor_files(a.files, a.drug, a.channel, a.panels, a.every, a.device)
    print(json.dumps(rec))
    sys.stdout.flush()
    return rec


if __name__ == "__main__":
    main()
