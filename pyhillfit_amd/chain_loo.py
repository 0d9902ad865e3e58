"""PSIS-LOO of chains already on disk (pyhillfit_amd/loo.py), as chain_waic does for WAIC.

    python -m pyhillfit_amd.chain_loo --data-file F FILE... [--drug D --channel C] [--model 1|2] [--tail-per-chain K] [--device cuda:0]

FILE is a `<chain file>_all_chains.npy` of --save-all-chains ([rows][columns][chains], burn-in removed; single-level) or a
reference-format chain text file: single-level (burn-in removed already; the pair and the model are read from its header) or
hierarchical (recognised by its header; the whole chain, whose first quarter is dropped as construct_hierarchical_cdfs.py does;
Ne from the columns).  Files are read exactly as chain_waic reads them.  The data points come from --data-file.  One JSON object per
file on stdout; the accumulation and the Pareto smoothing run on the GPU (phf_psis_accumulate / phf_psis_reduce), like --loo.

    python -m pyhillfit_amd.chain_loo --experiments --data-file F FILE... [--marginal-nodes 128] [--marginal-every 1]

scores a HIERARCHICAL chain file (the reference's own included) by the integrated leave-one-experiment-out instead
(pyhillfit_amd/marginal.py): the marginal log-likelihood of every experiment at every --marginal-every-th row after the burn-in through
the batch evaluator (phf_hier_marginal_loglik), then WAIC and PSIS over the experiments: the "loo_experiment" record of
PyHillFit --hierarchical --leave-experiment-out for the file's one chain."""
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


def logo_file(path, drug=None, channel=None, nodes=None, every=1, device="cuda:0"):
    """the "loo_experiment" record of a hierarchical chain file"""
    import numpy as np
    import torch
    from . import marginal as mg
    rows, kind, drug, channel, _ = load(path, drug, channel, None)
    if kind != "hierarchical text":
        raise SystemExit("{}: --experiments scores hierarchical chain files (this is a {} file): a single-level fit has no "
                         "experiment-level parameters to integrate out".format(path, kind))
    nodes = mg.DEFAULT_NODES if nodes is None else mg.check_nodes(nodes)
    ne = (rows.shape[1] - 6) // 2
    expts, labels = experiments_and_labels(drug, channel, ne)
    pts = wc.Points.hierarchical([expts], [labels])
    x = np.asarray(rows, dtype=np.float64)                                  # [rows][columns][chains]
    used = x[::every]
    n, _, c = used.shape
    theta = used[:, :5 + 2 * ne].transpose(0, 2, 1).reshape(n * c, 5 + 2 * ne)
    m, g = mg.MarginalLogLik(pts, nodes, device)(np.zeros(n * c, dtype=np.int32), theta)
    ll = np.ascontiguousarray(m.reshape(n, c, ne).transpose(0, 2, 1)[:, None])   # [used][1][Ne][chains]
    ep = mg.experiment_points(pts)
    w, p = wc.PointwiseWAIC(ep, "given", 1, c, n, device), lo.PointwiseLOO(ep, "given", 1, c, n, device)
    t = torch.from_numpy(ll).to(w.device)
    w.accumulate(t)
    p.accumulate(t)
    lse, var = w.reduced()
    r = p.reduced()
    with np.errstate(invalid="ignore"):
        gap = np.fmax.reduce(np.vstack([np.zeros((1, ne)), g]), axis=0)     # NaN gaps are passed over, as the streaming maximum does
    res = mg.finalize(r["elpd_loo"][0], r["lppd"][0], r["khat"][0], r["determined"][0], lse[0], var[0], gap,
                      [len(e) for e in expts], n * c)
    rec = mg.json_record(res, labels, nodes, every)
    return dict({"file": path, "kind": kind, "drug": drug, "channel": channel, "model": "hierarchical", "rows": int(x.shape[0]),
                 "chains": int(c)}, loo_experiment=rec)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="chain_loo")
    ap.add_argument("files", nargs="+")
    ap.add_argument("--data-file", required=True, help="csv or json data file the chains were fitted to")
    ap.add_argument("--drug", default=None)
    ap.add_argument("--channel", default=None)
    ap.add_argument("--model", type=int, default=None, help="single-level model (1 | 2) if the file does not say")
    ap.add_argument("--tail-per-chain", type=int, default=0, help="smallest log-likelihoods kept per (point, chain); 0: the default rule")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--experiments", action="store_true", help="hierarchical chain files: the integrated leave-one-experiment-out "
                    "(the \"loo_experiment\" record) instead of the pointwise PSIS-LOO")
    ap.add_argument("--marginal-nodes", type=int, default=None, help="--experiments: nodes a side of the rule, 32, 64, 128 (default) or 256")
    ap.add_argument("--marginal-every", type=int, default=None, help="--experiments: every T-th row after the burn-in (default 1: a chain file "
                    "holds one chain, where PyHillFit's default thins the rows of all its chains)")
    a = ap.parse_args(argv)
    if not a.experiments and (a.marginal_nodes is not None or a.marginal_every is not None):
        ap.error("--marginal-nodes and --marginal-every need --experiments")
    if a.experiments:
        from .marginal import NODE_CHOICES
        if a.marginal_nodes is not None and a.marginal_nodes not in NODE_CHOICES:
            ap.error("--marginal-nodes must be one of %s" % ", ".join(str(q) for q in NODE_CHOICES))
        if a.marginal_every is not None and a.marginal_every < 1:
            ap.error("--marginal-every must be >= 1")
    dr.setup(a.data_file)
    for p in a.files:
        if a.experiments:
            print(json.dumps(logo_file(p, a.drug, a.channel, a.marginal_nodes, a.marginal_every or 1, a.device)))
        else:
            print(json.dumps(loo_file(p, a.drug, a.channel, a.model, a.tail_per_chain, a.device)))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
