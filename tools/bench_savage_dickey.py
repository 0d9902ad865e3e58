"""Measurements of the Savage-Dickey Bayes factor (pyhillfit_amd/savage_dickey.py; results under profiles/savage_dickey/).

    python tools/bench_savage_dickey.py kernel [--panels 16,32,64] [--rows 2] [--sampling-seconds S]
    python tools/bench_savage_dickey.py run --output-root DIR [--tree CHECKOUT] [--flag [--every T] [--run-panels 32]] [-- extra PyHillFit flags]
    python tools/bench_savage_dickey.py table SUMMARY_DIR

  kernel  ms per used row of phf_savage_dickey_accumulate (HIP events, the median of three launches after a warm-up) at each panel
          count on
            cli  the single-level command line's defaults: every Crumb pair with data x 64 chains
            c3   BASELINE C3: 210 problems x 4 096 chains (the Crumb pairs' entries, repeated to 210)
          on synthetic draws near a posterior (pIC50 ~ 5.5, sigma ~ 6), `--rows` used rows a launch.  With --sampling-seconds also
          the smallest --savage-dickey-every whose cost over 75 001 post-burn-in rows stays below that time.
  run     one `PyHillFit -m 2 -a` of the Crumb set in a child process, with --savage-dickey (--flag) or without, from this checkout
          or from --tree: the wall time and the run's own "timing" line.  One JSON line.
  table   from the summaries of a --savage-dickey run: per pair log B12 +- se, ess and gap; the counts favouring each model and the
          count not reliable."""
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


def crumb_packed(repeat_to=None):
    """PackedPoints of every Crumb pair with data (repeated cyclically to `repeat_to` pairs if given)"""
    from pyhillfit_amd import doseresponse as dr
    from pyhillfit_amd.PyHillFit import load_single_level_pairs
    dr.setup(os.path.join(REPO, "data", "crumb_dataset.json"))
    pairs = [(c, y) for _, _, c, y in load_single_level_pairs([(d, c) for d in dr.drugs for c in dr.channels])]
    if repeat_to:
        pairs = [pairs[i % len(pairs)] for i in range(repeat_to)]
    return dr.PackedPoints(pairs)


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
    from pyhillfit_amd import savage_dickey as sd
    dev = "cuda:0"
    res = []
    for shape, packed, C in (("cli", crumb_packed(), 64), ("c3", crumb_packed(210), 4096)):
        Q = packed.num_pairs
        x = draws(a.rows, Q, C, dev)
        for panels in [int(v) for v in a.panels.split(",")]:
            w = sd.SavageDickey(packed, Q, C, panels, 1, dev)
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
            entries = float(packed.counts[:, :3].sum(axis=1).mean())
            rec = {"shape": shape, "problems": Q, "chains": C, "panels": panels, "nodes": 15 * panels, "mean_entries_per_pair": round(entries, 2),
                   "rows_timed": a.rows, "ms_per_used_row": round(per_row_ms, 4), "ns_per_draw": round(1e6 * per_row_ms / (Q * C), 2)}
            if shape == "cli" and a.sampling_seconds:
                affordable = int(a.sampling_seconds * 1e3 / per_row_ms)
                rec["used_rows_within_sampling_time"] = affordable
                rec["every_for_%d_rows" % POST_BURN_IN_ROWS] = -(-POST_BURN_IN_ROWS // max(1, affordable))
            res.append(rec)
            w.free()
        del x
    print(json.dumps({"tool": "bench_savage_dickey", "mode": "kernel", "sampling_seconds": a.sampling_seconds, "results": res}))


def run(a, extra):
    cmd = [sys.executable, "-m", "pyhillfit_amd.PyHillFit", "--data-file", os.path.join(REPO, "data", "crumb_dataset.json"), "-m", "2",
           "-a", "--output-root", a.output_root] + extra
    if a.flag:
        cmd += ["--savage-dickey", "--savage-dickey-panels", str(a.run_panels)] + (["--savage-dickey-every", str(a.every)] if a.every else [])
    t0 = time.time()
    # a whole Crumb run takes a minute or two; the limit ends a child that hangs (subprocess.run kills it and raises)
    p = subprocess.run(cmd, cwd=a.tree or REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=a.limit)
    wall = time.time() - t0
    lines = p.stdout.splitlines()
    timing = [l for l in lines if l.startswith("timing [rank")]
    m = re.search(r"sampling ([0-9.]+) s", timing[-1]) if timing else None
    print(json.dumps({"tool": "bench_savage_dickey", "mode": "run", "tree": a.tree or REPO, "flags": cmd[cmd.index("-a") + 1:],
                      "returncode": p.returncode, "wall_seconds": round(wall, 1), "sampling_seconds": float(m.group(1)) if m else None,
                      "timing": timing[-1] if timing else None, "report": [l for l in lines if l.startswith("bayes-factor [rank")],
                      "tail": lines[-5:] if p.returncode else []}))
    return p.returncode


def table(a):
    rows = []
    for f in sorted(glob.glob(os.path.join(a.summaries, "**", "*_summary.json"), recursive=True)):
        with open(f) as fh:
            s = json.load(fh)
        if "bayes_factor" in s:
            rows.append((s["drug"], s["channel"], s["bayes_factor"]))
    head = rows[0][2] if rows else {"panels": "?", "every": "?", "draws_used": "?"}
    out = ["# Savage-Dickey log B12 (Hill = 1 against Hill free; > 0 favours Hill = 1) per pair, from the model-2 draws alone",
           "# (--savage-dickey, P = %s panels, every %s-th row: %s draws per pair); se: between-chain Monte Carlo error only"
           % (head["panels"], head["every"], head["draws_used"]),
           "{:<16} {:<12} {:>10} {:>9} {:>10} {:>9} {:>9} {:>10} {:>9}".format("drug", "channel", "log B12", "se", "ess", "gap", "gap max", "max share",
                                                                               "reliable")]

    def fmt(v, spec):
        return format(v, spec) if v is not None else "n/a"
    one = two = bad = 0
    for drug, channel, r in rows:
        one += int(r["favours"] == "model 1")
        two += int(r["favours"] == "model 2")
        bad += int(not r["reliable"])
        out.append("{:<16} {:<12} {:>10} {:>9} {:>10} {:>9} {:>9} {:>10} {:>9}".format(
            drug, channel, fmt(r["log_b12"], ".4f"), fmt(r["log_b12_se"], ".2g"), fmt(r["ess"], ".0f"), fmt(r["gap"], ".1e"),
            fmt(r["quadrature_gap_max"], ".1e"), fmt(r["max_share"], ".2g"), "yes" if r["reliable"] else "NO"))
    out.append("# pairs: {}; favour model 1 (Hill = 1): {}; favour model 2 (Hill free): {}; not reliable: {}".format(len(rows), one, two, bad))
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
    ap.add_argument("--panels", default="16,32,64")
    ap.add_argument("--rows", type=int, default=2)
    ap.add_argument("--sampling-seconds", type=float, default=0.0)
    ap.add_argument("--output-root", default="output")
    ap.add_argument("--tree", default=None, help="run: the checkout whose PyHillFit runs (default: this one)")
    ap.add_argument("--every", type=int, default=0)
    ap.add_argument("--run-panels", type=int, default=32)
    ap.add_argument("--limit", type=float, default=600.0, help="run: seconds after which the child run is ended")
    ap.add_argument("--flag", action="store_true")
    a = ap.parse_args(argv)
    if a.mode == "kernel":
        kernel(a)
    elif a.mode == "run":
        sys.exit(run(a, extra))
    else:
        if not a.summaries:
            ap.error("table needs the output directory of a --savage-dickey run")
        table(a)


if __name__ == "__main__":
    main()
