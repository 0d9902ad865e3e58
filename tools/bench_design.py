"""Measurements of the next-dose analysis (pyhillfit_amd/design.py; results under profiles/next_dose/).

    python tools/bench_design.py kernel [--bins 256,1024] [--doses 16] [--rows 2] [--sampling-seconds S]
    python tools/bench_design.py run --output-root DIR [--tree CHECKOUT] [--flag [--every T] [--doses 16] [--bins 256]] [-- extra PyHillFit flags]
    python tools/bench_design.py table SUMMARY_DIR

  kernel  ms per used row of phf_design_accumulate (HIP events, the median of three launches after a warm-up) at each bin count on
            cli  the single-level command line's defaults: every Crumb pair with data x 64 chains
            c3   BASELINE C3: 210 problems x 4 096 chains
          on synthetic draws near a posterior (pIC50 ~ 5.5, Hill ~ 1, sigma ~ 6), `--rows` used rows a launch.  With
          --sampling-seconds also the smallest --next-dose-every whose cost over 75 001 post-burn-in rows stays below that time.
  run     one `PyHillFit -m 2 -a` of the Crumb set in a child process, with --next-dose (--flag) or without, from this checkout or
          from --tree: the wall time and the run's own "timing" line.  One JSON line.
  table   from the summaries of a --next-dose run: per pair the best dose and its EIG, and how many pairs have a gap above 1 % of
          the EIG at their best dose."""
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
POST_BURN_IN_ROWS = 75001               # the default run: 500 000 iterations, thinning 5, a quarter burnt in


def crumb_concs():
    """per Crumb pair with data, its concentrations"""
    from pyhillfit_amd import doseresponse as dr
    from pyhillfit_amd.PyHillFit import load_single_level_pairs
    dr.setup(os.path.join(REPO, "data", "crumb_dataset.json"))
    return [c for _, _, c, _ in load_single_level_pairs([(d, c) for d in dr.drugs for c in dr.channels])]


def draws(n, Q, C, dev):
    import torch
    x = torch.zeros((n, Q, 4, C), dtype=torch.float64, device=dev)
    shape = (n, Q, C)
    x[:, :, 0] = 5.5 + 0.3 * torch.randn(shape, dtype=torch.float64, device=dev)
    x[:, :, 1] = 1.0 + 0.2 * torch.rand(shape, dtype=torch.float64, device=dev)
    x[:, :, 2] = 6.0 + 2.0 * torch.rand(shape, dtype=torch.float64, device=dev)
    return x


def kernel(a):
    import numpy as np
    import torch
    from pyhillfit_amd import design as ds
    dev = "cuda:0"
    cli = crumb_concs()
    res = []
    for shape, concs, C in (("cli", cli, 64), ("c3", [[0.1, 1.0, 10.0, 100.0]] * 210, 4096)):
        doses = [ds.candidate_doses(c, a.doses) for c in concs]
        Q = len(concs)
        x = draws(a.rows, Q, C, dev)
        for bins in [int(v) for v in a.bins.split(",")]:
            w = ds.NextDose(2, Q, C, doses, None, bins, 1, dev)
            w.accumulate(x[:1])                                        # warm-up: tables, code object
            torch.cuda.synchronize(dev)
            t = []
            for _ in range(3):
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record()
                w.accumulate(x)
                ev1.record()
                torch.cuda.synchronize(dev)
                t.append(ev0.elapsed_time(ev1))
            per_row_ms = float(np.median(t)) / a.rows                  # one used row of every chain of every problem
            rec = {"shape": shape, "problems": Q, "chains": C, "doses": a.doses, "bins": bins, "slots": w.slots, "rows_timed": a.rows,
                   "ms_per_used_row": round(per_row_ms, 4), "ns_per_draw_dose": round(1e6 * per_row_ms / (Q * C * a.doses), 3)}
            if shape == "cli" and a.sampling_seconds:
                affordable = int(a.sampling_seconds * 1e3 / per_row_ms)
                rec["used_rows_within_sampling_time"] = affordable
                rec["every_for_%d_rows" % POST_BURN_IN_ROWS] = -(-POST_BURN_IN_ROWS // max(1, affordable))
            res.append(rec)
            w.free()
        del x
    print(json.dumps({"tool": "bench_design", "mode": "kernel", "sampling_seconds": a.sampling_seconds, "results": res}))


def run(a, extra):
    cmd = [sys.executable, "-m", "pyhillfit_amd.PyHillFit", "--data-file", os.path.join(REPO, "data", "crumb_dataset.json"), "-m", "2",
           "-a", "--output-root", a.output_root] + extra
    if a.flag:
        cmd += ["--next-dose", str(a.doses), "--next-dose-bins", str(a.run_bins)] + (["--next-dose-every", str(a.every)] if a.every else [])
    t0 = time.time()
    # a whole Crumb run takes a minute or two; the limit ends a child that hangs (subprocess.run kills it and raises)
    p = subprocess.run(cmd, cwd=a.tree or REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=a.limit)
    wall = time.time() - t0
    lines = p.stdout.splitlines()
    timing = [l for l in lines if l.startswith("timing [rank")]
    m = re.search(r"sampling ([0-9.]+) s", timing[-1]) if timing else None
    print(json.dumps({"tool": "bench_design", "mode": "run", "tree": a.tree or REPO, "flags": cmd[cmd.index("-a") + 1:], "returncode": p.returncode,
                      "wall_seconds": round(wall, 1), "sampling_seconds": float(m.group(1)) if m else None, "timing": timing[-1] if timing else None,
                      "report": [l for l in lines if l.startswith("next-dose [rank")], "tail": lines[-5:] if p.returncode else []}))
    return p.returncode


def table(a):
    rows = []
    for f in sorted(glob.glob(os.path.join(a.summaries, "**", "*_summary.json"), recursive=True)):
        with open(f) as fh:
            s = json.load(fh)
        if "next_dose" in s:
            rows.append((s["drug"], s["channel"], s["next_dose"]))
    head = rows[0][2] if rows else {"bins": "?", "every": "?", "draws_used": "?"}
    out = ["# best next dose per pair: expected information gain (nats) of one further measurement recorded to 100/K % block",
           "# (--next-dose, K = %s bins, every %s-th row: %s draws per pair)" % (head["bins"], head["every"], head["draws_used"]),
           "{:<16} {:<12} {:>12} {:>9} {:>10} {:>9} {:>8} {:>7}".format("drug", "channel", "best uM", "eig", "eig K/2", "gap/eig", "at end", "tested")]
    wide = ends = 0
    for drug, channel, r in rows:
        b, c = r["best"], r["candidates"]
        i = c.index(b)
        rel = b["gap"] / b["eig"] if b["eig"] else float("nan")
        at_end = i in (0, (a.grid or len(c)) - 1)
        wide += int(rel > 0.01)
        ends += int(at_end)
        out.append("{:<16} {:<12} {:>12.4g} {:>9.5f} {:>10.5f} {:>9.2e} {:>8} {:>7}".format(drug, channel, b["dose"], b["eig"], b["eig_coarse"], rel,
                                                                                      "yes" if at_end else "-", "yes" if b["already_tested"] else "-"))
    out.append("# pairs: {}; gap above 1 % of eig at the best dose: {}; best dose at an end of the grid: {}".format(len(rows), wide, ends))
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
    ap.add_argument("--bins", default="256,1024")
    ap.add_argument("--doses", type=int, default=16)
    ap.add_argument("--rows", type=int, default=2)
    ap.add_argument("--sampling-seconds", type=float, default=0.0)
    ap.add_argument("--output-root", default="output")
    ap.add_argument("--tree", default=None, help="run: the checkout whose PyHillFit runs (default: this one)")
    ap.add_argument("--every", type=int, default=0)
    ap.add_argument("--run-bins", type=int, default=256)
    ap.add_argument("--grid", type=int, default=0, help="table: the number of log-spaced candidates (default: all candidates)")
    ap.add_argument("--limit", type=float, default=600.0, help="run: seconds after which the child run is ended")
    ap.add_argument("--flag", action="store_true")
    a = ap.parse_args(argv)
    if a.mode == "kernel":
        kernel(a)
    elif a.mode == "run":
        sys.exit(run(a, extra))
    else:
        if not a.summaries:
            ap.error("table needs the output directory of a --next-dose run")
        table(a)


if __name__ == "__main__":
    main()
