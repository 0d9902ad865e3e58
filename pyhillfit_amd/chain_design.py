"""Expected information gain of a next dose from chains already on disk (pyhillfit_amd/design.py), as chain_quantiles and
chain_sensitivity do for their analyses.

    python -m pyhillfit_amd.chain_design --data-file F -m M FILE... [--drug D --channel C] [--doses 16] [--concs c1,c2,...]
           [--bins 256] [--every 1] [--device cuda:0]

FILE is read as by chain_waic: a `<chain file>_all_chains.npy` of --save-all-chains ([rows][columns][chains], burn-in removed) or a
single-level chain text file in the reference's format, this package's or the reference's own (the pair and the model from its
header; -m says the model if the file does not).  The candidates are --doses doses log-spaced from the pair's smallest dose / 10 to
its largest x 10 in the data of --data-file, then the named --concs (uM).  The sums are accumulated on the GPU by the kernel the
command line's --next-dose uses.  One JSON object per file on stdout."""
import argparse
import json
import sys

from . import design as ds
from . import doseresponse as dr


def build_parser():
    ap = argparse.ArgumentParser(prog="chain_design")
    ap.add_argument("files", nargs="+")
    ap.add_argument("--data-file", required=True, help="csv or json data file the chains were fitted to")
    ap.add_argument("-m", "--model", type=int, default=None, help="single-level model (1 | 2) if the file does not say")
    ap.add_argument("--drug", default=None)
    ap.add_argument("--channel", default=None)
    ap.add_argument("--doses", type=int, default=ds.DEFAULT_DOSES, metavar="G")
    ap.add_argument("--concs", type=str, default=None, metavar="C1,C2,...")
    ap.add_argument("--bins", type=int, default=ds.DEFAULT_BINS, metavar="K")
    ap.add_argument("--every", type=int, default=1, metavar="T")
    ap.add_argument("--device", default="cuda:0")
    return ap


def check_args(ap, a):
    try:
        a.bins = ds.check_bins(a.bins)
        a.concs = ds.parse_concs(a.concs) if isinstance(a.concs, str) else (a.concs or ())
    except ValueError as e:
        ap.error(str(e).replace("--next-dose-", "--"))
    if a.doses < 1:
        ap.error("--doses must be >= 1")
    if a.every < 1:
        ap.error("--every must be >= 1")
    if a.model not in (None, 1, 2):
        ap.error("-m must be 1 or 2 (single-level)")


def design_file(path, drug=None, channel=None, model=None, doses=ds.DEFAULT_DOSES, concs=(), bins=ds.DEFAULT_BINS, every=1,
                device="cuda:0"):
    from . import chain_waic as cw
    rows, kind, drug, channel, model = cw.load(path, drug, channel, model)
    if kind == "hierarchical text":
        raise SystemExit("{}: a hierarchical chain file; the next-dose analysis is single-level only".format(path))
    if model not in (1, 2):
        raise SystemExit("{}: model must be 1 or 2".format(path))
    num_expts, _, experiments = dr.load_crumb_data(drug, channel)
    tested, _ = dr.concatenate_experiments(num_expts, experiments)
    res = ds.design_of_draws(model, rows, ds.candidate_doses(tested, doses, concs), tested, bins, every, device)
    return dict({"file": path, "kind": kind, "drug": drug, "channel": channel, "model": model, "rows": int(rows.shape[0]),
                 "chains": int(rows.shape[2])}, **ds.json_record(res))


def main(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    check_args(ap, a)
    dr.setup(a.data_file)
    out = []
    for p in a.files:
        rec = design_file(p, a.drug, a.channel, a.model, a.doses, a.concs, a.bins, a.every, a.device)
        print(json.dumps(rec))
        sys.stdout.flush()
        out.append(rec)
    return out


if __name__ == "__main__":
    main()
