"""Power-scaling sensitivity of chains already on disk (pyhillfit_amd/sensitivity.py), as chain_waic does for WAIC.

    python -m pyhillfit_amd.chain_sensitivity --data-file F [--hierarchical] FILE... [--drug D --channel C] [--model 1|2]
           [--delta 0.01] [--bins 4096] [--threshold 0.05] [--given PRIOR_COL,LIK_COL] [--device cuda:0]

FILE is read as by chain_waic: a `<chain file>_all_chains.npy` of --save-all-chains ([rows][columns][chains], burn-in removed;
single-level) or a reference-format chain text file, this package's or the reference's own: single-level (the pair and the model
from its header) or hierarchical (recognised by its header, or named so with --hierarchical; its first quarter is dropped as
construct_hierarchical_cdfs.py does; Ne from the columns; the pair from the file name unless named).  The components are evaluated
from the data of --data-file, on the GPU, like the command lines' --sensitivity.  With --given PRIOR_COL,LIK_COL the two named
columns of the file are the components instead (chain files of other models) and every other column is a parameter; --data-file is
then not read.  One JSON object per file on stdout."""
import argparse
import json
import sys

import numpy as np

from . import doseresponse as dr
from . import sensitivity as sn


def _given(text):
    try:
        p, l = (int(v) for v in str(text).split(","))
    except ValueError:
        raise argparse.ArgumentTypeError("--given takes PRIOR_COL,LIK_COL, got %r" % (text,))
    if p < 0 or l < 0 or p == l:
        raise argparse.ArgumentTypeError("--given: two different non-negative column indices, got %r" % (text,))
    return p, l


def build_parser():
    ap = argparse.ArgumentParser(prog="chain_sensitivity")
    ap.add_argument("files", nargs="+")
    ap.add_argument("--data-file", default=None, help="csv or json data file the chains were fitted to (not needed with --given)")
    ap.add_argument("--hierarchical", action="store_true", default=False, help="the files are hierarchical chain files")
    ap.add_argument("--drug", default=None)
    ap.add_argument("--channel", default=None)
    ap.add_argument("--model", type=int, default=None, help="single-level model (1 | 2) if the file does not say")
    ap.add_argument("--delta", type=float, default=sn.DEFAULT_DELTA)
    ap.add_argument("--bins", type=int, default=sn.DEFAULT_BINS)
    ap.add_argument("--threshold", type=float, default=sn.DEFAULT_THRESHOLD)
    ap.add_argument("--given", type=_given, default=None, metavar="PRIOR_COL,LIK_COL")
    ap.add_argument("--device", default="cuda:0")
    return ap


def check_args(ap, a):
    try:
        a.delta, a.bins, a.threshold = sn.check_delta(a.delta), sn.check_bins(a.bins), sn.check_threshold(a.threshold)
    except ValueError as e:
        ap.error(str(e).replace("--sensitivity-", "--"))
    if a.given is None and not a.data_file:
        ap.error("--data-file is required (unless --given names the component columns)")


def given_file(path, given, delta, bins, threshold, device):
    from .chain_diagnostics import load_rows
    rows, kind = load_rows(path)
    ncol = rows.shape[1]
    if max(given) >= ncol:
        raise SystemExit("{}: --given names column {}, the file has {}".format(path, max(given), ncol))
    params = [c for c in range(ncol) if c not in given]
    # the parameters first, then the two components: the leading columns are the slots
    x = np.concatenate([rows[:, params], rows[:, list(given)]], axis=1)
    res = sn.sensitivity_of_draws(None, "given", x, delta, bins, threshold, device, given=(len(params), len(params) + 1), columns=len(params))
    rec = sn.json_record(res, 0, ["column_%d" % c for c in params])
    return dict({"file": path, "kind": kind, "model": "given", "given": list(given), "rows": int(rows.shape[0]), "chains": int(rows.shape[2])}, **rec)


def sensitivity_file(path, drug=None, channel=None, model=None, hierarchical=False, delta=sn.DEFAULT_DELTA, bins=sn.DEFAULT_BINS,
                     threshold=sn.DEFAULT_THRESHOLD, device="cuda:0"):
    from . import chain_waic as cw
    from .PyHillFit import experiments_and_labels
    if (hierarchical or not path.endswith(".npy")) and not (drug and channel):
        with open(path) as f:
            first = f.readline()
        from . import chainio
        if hierarchical or first == chainio.HIERARCHICAL_HEADER[0]:
            from .chain_quantiles import pair_of_file_name
            drug, channel = pair_of_file_name(path, dr.drugs, dr.channels)
    rows, kind, drug, channel, model = cw.load(path, drug, channel, model)
    if hierarchical and kind != "hierarchical text":
        raise SystemExit("{}: not a hierarchical chain file".format(path))
    if kind == "hierarchical text":
        from .hierarchical import DeviceHierPoints, PackedHierPoints, hierarchical_columns, make_prior, prior_params
        ne = (rows.shape[1] - 6) // 2
        expts, _ = experiments_and_labels(drug, channel, ne)
        pts = DeviceHierPoints(PackedHierPoints([expts]), device)
        res = sn.sensitivity_of_draws(pts, "hierarchical", rows, delta, bins, threshold, device, prior=make_prior(*prior_params()),
                                      columns=5 + 2 * ne)
        names, label = hierarchical_columns(ne)[:5 + 2 * ne], "hierarchical"
    else:
        if model not in (1, 2):
            raise SystemExit("{}: model must be 1 or 2".format(path))
        from .sampler import DevicePoints
        num_expts, _, experiments = dr.load_crumb_data(drug, channel)
        concs, responses = dr.concatenate_experiments(num_expts, experiments)
        pts = DevicePoints(dr.PackedPoints([(concs, responses)]), device)
        res = sn.sensitivity_of_draws(pts, model, rows, delta, bins, threshold, device, columns=model + 1)
        names, label = (["pIC50", "sigma"] if model == 1 else ["pIC50", "Hill", "sigma"]), model
    rec = sn.json_record(res, 0, names)
    return dict({"file": path, "kind": kind, "drug": drug, "channel": channel, "model": label, "rows": int(rows.shape[0]),
                 "chains": int(rows.shape[2])}, **rec)


def main(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    check_args(ap, a)
    if a.given is None:
        dr.setup(a.data_file)
    for p in a.files:
        if a.given is not None:
            rec = given_file(p, a.given, a.delta, a.bins, a.threshold, a.device)
        else:
            rec = sensitivity_file(p, a.drug, a.channel, a.model, a.hierarchical, a.delta, a.bins, a.threshold, a.device)
        print(json.dumps(rec))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
