"""Measurement of the streaming PSIS-LOO accumulation and reduce (phf_psis_accumulate / phf_psis_reduce) over whole runs at three
shapes.  One JSON line.

    python tools/bench_psis.py [--shapes cli,c3,c4] [--rows N]

  cli  the single-level command line's defaults: the 210 Crumb pairs (2 584 points) x 64 chains, model 2, 75 001 post-burn-in rows,
       segments of 4 000
  c3   BASELINE C3: the same pairs x 4 096 chains, segments of 4 800 rows
  c4   BASELINE C4: 210 hierarchical problems of Ne = 3 experiments x 4 points (12 columns) x 1 024 chains, segments of 4 000 rows
Every segment is fresh synthetic draws near the posterior (tools/bench_waic.py's), generated outside the timed region; the draws are
independent, so the heap insertions per draw are those of an ideally mixed chain (MCMC streams repeat values and drift: the command
lines' summaries report their own rate).  --rows shortens the run (the tail length, the heap capacity and the reduce follow it)."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from bench_waic import SHAPES, crumb_points, synthetic_rows  # noqa: E402


def measure(name, dev, points, run_rows=None):
    import numpy as np
    import torch
    from pyhillfit_amd.loo import PointwiseLOO, workspace_bytes
    sh = SHAPES[name]
    pts = points[1] if sh["kind"] == "hierarchical" else points[0]
    Q, C, seg = pts.num_problems, sh["chains"], sh["seg"]
    total = run_rows or sh["run_rows"]
    cols = 5 + 2 * pts.num_expts + 1 if sh["kind"] == "hierarchical" else 4
    w = PointwiseLOO(pts, sh["kind"], Q, C, total, dev)
    times, done = [], 0
    while done < total:
        n = min(seg, total - done)
        rows = synthetic_rows(Q, cols, C, n, sh["kind"], dev)
        torch.cuda.synchronize(dev)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        w.accumulate(rows)
        ev1.record()
        torch.cuda.synchronize(dev)
        times.append((n, ev0.elapsed_time(ev1)))
        done += n
        del rows
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    r = w.reduced()
    ev1.record()
    torch.cuda.synchronize(dev)
    reduce_ms = ev0.elapsed_time(ev1)
    ins = w.insertions()
    valid = np.arange(pts.stride)[None, :] < pts.count[:, None]
    n_points = int(pts.count.sum())
    full = [t for n, t in times[1:] if n == seg]                  # steady state: the first segment fills the heaps
    out = {"shape": name, "problems": Q, "points": n_points, "chains": C, "columns": cols, "rows_per_segment": seg, "run_rows": total,
           "tail_length": w.M, "tail_per_chain": w.k, "reduce_path": "hbm" if w.M + 1 > 8192 else "lds",
           "first_segment_ms": round(times[0][1], 3), "ms_per_segment": round(float(np.median(full)), 3) if full else None,
           "accumulate_ms_total": round(sum(t for _, t in times), 1), "reduce_ms": round(reduce_ms, 1),
           "insertions_per_draw": float(ins[valid].sum() / (n_points * C * total)),
           "undetermined_points": int(np.sum(r["determined"][valid] == 0.0)),
           "workspace_gb": round(workspace_bytes(Q, pts.stride, C, total) / 1e9, 3)}
    w.free()
    del w
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="cli,c3,c4")
    ap.add_argument("--rows", type=int, default=None, help="post-burn-in rows of the run (default: each shape's 75 001)")
    a = ap.parse_args()
    dev = "cuda:0"
    points = crumb_points()
    res = [measure(n, dev, points, a.rows) for n in a.shapes.split(",")]
    print(json.dumps({"tool": "bench_psis", "results": res}))


if __name__ == "__main__":
    main()
