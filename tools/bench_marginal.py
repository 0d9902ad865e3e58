"""Measurements of the integrated leave-one-experiment-out (pyhillfit_amd/marginal.py; results under profiles/marginal/).

    python tools/bench_marginal.py kernel [--nodes 64,128,256] [--rows 2]
    python tools/bench_marginal.py run --output-root DIR [--every T] [--nodes 128] [--flag | --loo-too] [-- extra PyHillFit flags]
    python tools/bench_marginal.py table SUMMARY_DIR

  kernel  ms per (draw, experiment) of phf_hier_marginal_rows at each node count on two shapes:
            c4   BASELINE C4: 210 hierarchical problems of Ne = 3 experiments x 4 points x 1 024 chains
            cli  the hierarchical command line's defaults: every Crumb pair, grouped by its number of experiments, x 128 chains
          on synthetic draws near the posterior (alpha ~ 1, beta ~ 5, mu ~ 5.5, s ~ 0.2, sigma ~ 8), `--rows` used rows a launch.
          Also the largest --marginal-every count of draws whose cost stays below a given sampling time (--sampling-seconds).
  run     one `PyHillFit --hierarchical -a` of the Crumb set in a child process, with --leave-experiment-out (--flag), with it and
          --loo (--loo-too) or without: the wall time and the run's own "timing" line.  One JSON line.
  table   from the summaries of a --loo --leave-experiment-out run: per pair, the points with a conditional pointwise k-hat above the
          threshold against the experiments with an integrated k-hat above it, and the experiments whose quadrature gap exceeds 0.01."""
import argparse
import glob
import json
import os
import re
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def crumb_groups():
    """{Ne: Points} of every Crumb pair with data"""
    from pyhillfit_amd import doseresponse as dr
    from pyhillfit_amd import waic as wc
    from pyhillfit_amd.PyHillFit import experiments_and_labels
    dr.setup(os.path.join(REPO, "data", "crumb_dataset.json"))
    groups = {}
    for d in dr.drugs:
        for c in dr.channels:
            try:
                ex, lab = experiments_and_labels(d, c)
            except ValueError:
                continue
            groups.setdefault(len(ex), []).append((ex, lab))
    return {ne: wc.Points.hierarchical(*zip(*g)) for ne, g in sorted(groups.items())}


def c4_points():
    import numpy as np
    from pyhillfit_amd import waic as wc
    rng = np.random.default_rng(0)
    return {3: wc.Points.hierarchical([[np.column_stack([10.0 ** np.arange(-1, 3), rng.uniform(0, 100, 4)]) for _ in range(3)]
                                       for _ in range(210)])}


def draws(n, Q, ne, C, dev):
    import torch
    x = torch.full((n, Q, 5 + 2 * ne + 1, C), float("nan"), dtype=torch.float64, device=dev)
    shape = (n, Q, C)
    x[:, :, 0] = 1.0 + 0.1 * torch.randn(shape, dtype=torch.float64, device=dev)
    x[:, :, 1] = 5.0 + 0.5 * torch.randn(shape, dtype=torch.float64, device=dev)
    x[:, :, 2] = 5.5 + 0.3 * torch.randn(shape, dtype=torch.float64, device=dev)
    x[:, :, 3] = 0.2 + 0.05 * torch.rand(shape, dtype=torch.float64, device=dev)
    x[:, :, 4 + 2 * ne] = 8.0 + torch.rand(shape, dtype=torch.float64, device=dev)
    return x


def kernel(a):
    import numpy as np
    import torch
    from pyhillfit_amd import marginal as mg
    dev = "cuda:0"
    res = []
    for shape, groups, C in (("c4", c4_points(), 1024), ("cli", crumb_groups(), 128)):
        for nodes in [int(v) for v in a.nodes.split(",")]:
            units, ms = 0, 0.0
            for ne, pts in groups.items():
                w = mg.MarginalRows(pts, pts.num_problems, C, nodes, 1, dev)
                x = draws(a.rows, pts.num_problems, ne, C, dev)
                w(x[:1])                                               # warm-up: tables, code object
                torch.cuda.synchronize(dev)
                t = []
                for _ in range(3):
                    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    ev0.record()
                    w(x)
                    ev1.record()
                    torch.cuda.synchronize(dev)
                    t.append(ev0.elapsed_time(ev1))
                ms += float(np.median(t))
                units += a.rows * pts.num_problems * ne * C
                del w, x
            per_row_ms = ms / a.rows                                   # one used row of every chain of every problem
            rec = {"shape": shape, "nodes": nodes, "chains": C, "experiments": units // (a.rows * C), "rows_timed": a.rows,
                   "ms_per_used_row": round(per_row_ms, 3), "us_per_draw_experiment": round(1e3 * ms / units, 4)}
            if shape == "cli" and a.sampling_seconds:
                rows_affordable = int(a.sampling_seconds * 1e3 / per_row_ms)
                rec["used_rows_within_sampling_time"] = rows_affordable
                rec["every_for_75001_rows"] = -(-75001 // max(1, rows_affordable))
            res.append(rec)
    print(json.dumps({"tool": "bench_marginal", "mode": "kernel", "sampling_seconds": a.sampling_seconds, "results": res}))


def run(a, extra):
    cmd = [sys.executable, "-m", "pyhillfit_amd.PyHillFit", "--data-file", os.path.join(REPO, "data", "crumb_dataset.json"), "-m", "2",
           "--hierarchical", "-a", "--output-root", a.output_root] + extra
    if a.flag or a.loo_too:
        cmd += ["--leave-experiment-out", "--marginal-nodes", str(a.run_nodes)] + (["--marginal-every", str(a.every)] if a.every else [])
    if a.loo_too:
        cmd += ["--loo"]
    t0 = time.time()
    # a whole Crumb run takes about a minute; the limit ends a child that hangs (subprocess.run kills it and raises)
    p = subprocess.run(cmd, cwd=a.tree or REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=a.limit)
    wall = time.time() - t0
    lines = p.stdout.splitlines()
    timing = [l for l in lines if l.startswith("timing [rank")]
    m = re.search(r"sampling ([0-9.]+) s", timing[-1]) if timing else None
    print(json.dumps({"tool": "bench_marginal", "mode": "run", "tree": a.tree or REPO, "flags": cmd[cmd.index("-a") + 1:], "returncode": p.returncode,
                      "wall_seconds": round(wall, 1), "sampling_seconds": float(m.group(1)) if m else None, "timing": timing[-1] if timing else None,
                      "report": [l for l in lines if l.startswith(("loo-experiment [rank", "loo [rank"))],
                      "tail": lines[-5:] if p.returncode else []}))
    return p.returncode


def table(a):
    rows = []
    for f in sorted(glob.glob(os.path.join(a.summaries, "**", "*_summary.json"), recursive=True)):
        with open(f) as fh:
            s = json.load(fh)
        if "loo_experiment" not in s:
            continue
        e = s["loo_experiment"]
        c = s.get("loo")
        rows.append((s["drug"], s["channel"], s["num_expts"], c["n_points"] if c else None, c["n_khat_above_threshold"] if c else None,
                     e["n_khat_above_threshold"], e["n_gap_above_0.01"], e["max_khat"], e["elpd_logo"], e["draws"], e["nodes"], e["every"]))
    out = ["# flagged Pareto k-hat per pair: conditional pointwise PSIS-LOO (--loo) against integrated leave-one-experiment-out",
           "# (--leave-experiment-out, %s nodes, every %s-th row: %s draws per experiment)" % ((rows[0][10], rows[0][11], rows[0][9]) if rows else ("?",) * 3),
           "{:<16} {:<12} {:>3} {:>7} {:>13} {:>13} {:>9} {:>9} {:>10}".format("drug", "channel", "Ne", "points", "cond. k>thr", "integ. k>thr",
                                                                          "gap>0.01", "max k", "elpd_logo")]
    for r in rows:
        out.append("{:<16} {:<12} {:>3} {:>7} {:>13} {:>13} {:>9} {:>9} {:>10}".format(
            r[0], r[1], r[2], "-" if r[3] is None else r[3], "-" if r[4] is None else r[4], r[5], r[6],
            "-" if r[7] is None else "%.3f" % r[7], "-" if r[8] is None else "%.2f" % r[8]))
    cond = [r for r in rows if r[4] is not None]
    out.append("# pairs: {}; conditional: {} flagged points of {} in {} pairs; integrated: {} flagged experiments of {} in {} pairs; "
               "experiments with a quadrature gap above 0.01: {} in {} pairs".format(
                   len(rows), sum(r[4] for r in cond), sum(r[3] for r in cond), sum(1 for r in cond if r[4]), sum(r[5] for r in rows),
                   sum(r[2] for r in rows), sum(1 for r in rows if r[5]), sum(r[6] for r in rows), sum(1 for r in rows if r[6])))
    print("\n".join(out))


def main():
    argv = sys.argv[1:]
    extra = []
    if "--" in argv:
        extra = argv[argv.index("--") + 1:]
        argv = argv[:argv.index("--")]
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernel", "run", "table"])
    ap.add_argument("summaries", nargs="?", default=None)
    ap.add_argument("--nodes", default="64,128,256")
    ap.add_argument("--rows", type=int, default=2)
    ap.add_argument("--sampling-seconds", type=float, default=0.0)
    ap.add_argument("--output-root", default="output")
    ap.add_argument("--tree", default=None, help="run: the checkout whose PyHillFit runs (default: this one)")
    ap.add_argument("--every", type=int, default=0)
    ap.add_argument("--run-nodes", type=int, default=128)
    ap.add_argument("--limit", type=float, default=600.0, help="run: seconds after which the child run is ended")
    ap.add_argument("--flag", action="store_true")
    ap.add_argument("--loo-too", action="store_true")
    a = ap.parse_args(argv)
    if a.mode == "kernel":
        kernel(a)
    elif a.mode == "run":
        sys.exit(run(a, extra))
    else:
        if not a.summaries:
            ap.error("table needs the output directory of a --loo --leave-experiment-out run")
        table(a)


if __name__ == "__main__":
    main()
