"""Measurement of the streaming posterior predictive check (phf_ppc_accumulate) against WAIC's accumulation at the same shapes, in the
same process, and of the command line's main() with and without --ppc; also writes the Crumb set's checks.

    python tools/bench_ppc.py [--shapes cli,c3,c4] [--segments 3] [--cli] [--out profiles/ppc]

Shapes (tools/bench_waic.py): cli = 210 Crumb pairs x 64 chains, model 2, segments of 4 000 rows; c3 = the same x 4 096 chains,
segments of 4 800; c4 = 210 hierarchical problems of Ne = 3 x 4 points x 1 024 chains, segments of 4 000.  With --cli: main() of
`-a -m 2` and `--hierarchical -a` at the defaults, each without and with --ppc, and `-a -m 1 --ppc`; the three --ppc runs' summaries
become <out>/crumb_ppc.txt.  One JSON line on stdout, also written to <out>/bench_ppc.json."""
import argparse
import glob
import io
import json
import os
import sys
import tempfile
import time
from contextlib import redirect_stdout

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import bench_waic as bw  # noqa: E402


def _time_segments(acc, rows, segments, dev):
    import torch
    acc.accumulate(rows)                                   # warm-up segment
    torch.cuda.synchronize(dev)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(segments):
        acc.accumulate(rows)
    ev1.record()
    torch.cuda.synchronize(dev)
    return ev0.elapsed_time(ev1) / segments


def measure(name, segments, dev, points):
    import torch
    from pyhillfit_amd.ppc import PosteriorPredictiveCheck, workspace_bytes
    from pyhillfit_amd.waic import PointwiseWAIC
    sh = bw.SHAPES[name]
    pts = points[1] if sh["kind"] == "hierarchical" else points[0]
    Q, C, seg = pts.num_problems, sh["chains"], sh["seg"]
    cols = 5 + 2 * pts.num_expts + 1 if sh["kind"] == "hierarchical" else 4
    total = seg * (segments + 1)
    rows = bw.synthetic_rows(Q, cols, C, seg, sh["kind"], dev)
    p = PosteriorPredictiveCheck(pts, sh["kind"], Q, C, total, 25, None, 0, dev)
    ppc_ms = _time_segments(p, rows, segments, dev)
    del p
    w = PointwiseWAIC(pts, sh["kind"], Q, C, total, dev)
    waic_ms = _time_segments(w, rows, segments, dev)
    del w, rows
    torch.cuda.empty_cache()
    n_points = int(pts.count.sum())
    return {"shape": name, "problems": Q, "points": n_points, "chains": C, "rows_per_segment": seg,
            "ppc_ms_per_segment": round(ppc_ms, 3), "waic_ms_per_segment": round(waic_ms, 3), "ppc_over_waic": round(ppc_ms / waic_ms, 2),
            "ppc_ns_per_point_draw": round(ppc_ms * 1e6 / (seg * C * n_points), 4),
            "ppc_ms_per_run_estimate": round(ppc_ms / seg * sh["run_rows"], 1),
            "workspace_gb": round(workspace_bytes(Q, pts.stride, C, sh["run_rows"]) / 1e9, 3)}


def _main_run(argv):
    from pyhillfit_amd import PyHillFit
    buf = io.StringIO()
    t0 = time.time()
    with redirect_stdout(buf):
        PyHillFit.main(argv)
    wall = time.time() - t0
    lines = [l for l in buf.getvalue().splitlines() if l.startswith(("ppc [", "timing ["))]
    return wall, lines


def _crumb_table(roots):
    """one line per pair and model: p of every statistic, points flagged (with their PIT)"""
    from pyhillfit_amd.ppc import STATS
    out = ["# posterior predictive checks of the Crumb set at the command line's defaults (seed 25); p = mid-p of T(y_rep) against T(y);",
           "# '*' marks p outside [0.01, 0.99]; flagged = points whose posterior-predictive PIT is outside [0.005, 0.995]",
           "{:<34} {:<6} {:>5} ".format("pair", "model", "n") + " ".join("{:>9}".format(s) for s in STATS) + "  flagged points"]
    totals = {}
    for label, root in roots:
        pairs = flagged = extreme = zeros_bad = with_zero = 0
        for path in sorted(glob.glob(os.path.join(root, "**", "*_summary.json"), recursive=True)):
            s = json.load(open(path))
            r = s["ppc"]
            ps = [r["statistics"][k]["p"] for k in STATS]
            cells = " ".join("{:>8.4f}{}".format(p, "*" if p is not None and not 0.01 <= p <= 0.99 else " ") if p is not None else "{:>9}".format("-")
                             for p in ps)
            pts = r["points"]
            fl = ["{}@{:g}:{:g}(u={:.4f})".format(e, d, y, u) for e, d, y, u, f in
                  zip(pts["experiment"], pts["dose"], pts["response"], pts["pit"], pts["flagged"]) if f]
            out.append("{:<34} {:<6} {:>5} {} {}".format(s["drug"] + " + " + s["channel"], label, r["n_points"], cells, " ".join(fl)))
            pairs += 1
            flagged += r["n_flagged"]
            extreme += 1 if r["extreme_statistics"] else 0
            if 0.0 in pts["response"]:
                with_zero += 1
                zeros_bad += 1 if r["statistics"]["zeros"]["p"] < 0.01 else 0
        totals[label] = {"pairs": pairs, "pairs_with_some_extreme_p": extreme, "points_flagged": flagged,
                         "pairs_with_a_zero_response": with_zero, "of_them_zeros_p_below_0.01": zeros_bad}
    out.append("# totals: " + json.dumps(totals))
    return "\n".join(out) + "\n", totals


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="cli,c3,c4")
    ap.add_argument("--segments", type=int, default=3)
    ap.add_argument("--cli", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ppc"))
    a = ap.parse_args()
    dev = "cuda:0"
    points = bw.crumb_points()
    res = {"tool": "bench_ppc", "shapes": [measure(n, a.segments, dev, points) for n in a.shapes.split(",") if n]}
    if a.cli:
        data = os.path.join(REPO, "data", "crumb_dataset.json")
        runs, roots = [], []
        with tempfile.TemporaryDirectory() as tmp:
            for label, extra in (("m2", ["-a", "-m", "2"]), ("hier", ["--hierarchical", "-a", "-m", "2"]), ("m1", ["-a", "-m", "1"])):
                for ppc in ((False, True) if label != "m1" else (True,)):
                    root = os.path.join(tmp, label + ("_ppc" if ppc else ""))
                    wall, lines = _main_run(["--data-file", data, "--output-root", root] + extra + (["--ppc"] if ppc else []))
                    runs.append({"run": " ".join(extra + (["--ppc"] if ppc else [])), "main_s": round(wall, 2), "report": lines})
                    if ppc:
                        roots.append((label if label != "hier" else "hier", root))
            table, totals = _crumb_table(roots)
        res["main"] = runs
        res["crumb"] = totals
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "crumb_ppc.txt"), "w") as f:
            f.write(table)
    line = json.dumps(res)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "bench_ppc.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
