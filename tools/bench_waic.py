"""Measurement of the streaming WAIC accumulation (phf_waic_accumulate): the time of accumulate() per segment at three shapes,
scaled to a whole run.  One JSON line.

    python tools/bench_waic.py [--shapes cli,c3,c4] [--segments 3]

  cli  the single-level command line's defaults: the 210 Crumb pairs (2 584 points) x 64 chains, model 2, 75 001 post-burn-in rows,
       segments of 4 000
  c3   BASELINE C3: the same pairs x 4 096 chains, segments of 4 800 rows
  c4   BASELINE C4: 210 hierarchical problems of Ne = 3 experiments x 4 points (12 columns) x 1 024 chains, segments of 4 000 rows
The rows are synthetic draws near the posterior (the cost does not depend on their values beyond the points' kinds)."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = {"cli": dict(chains=64, seg=4000, run_rows=75001, kind=2),
          "c3": dict(chains=4096, seg=4800, run_rows=75001, kind=2),
          "c4": dict(chains=1024, seg=4000, run_rows=75001, kind="hierarchical")}


def crumb_points():
    import numpy as np
    from pyhillfit_amd import doseresponse as dr
    from pyhillfit_amd import waic as wc
    from pyhillfit_amd.PyHillFit import experiments_and_labels
    dr.setup(os.path.join(REPO, "data", "crumb_dataset.json"))
    el = []
    for d in dr.drugs:
        for c in dr.channels:
            try:
                el.append(experiments_and_labels(d, c))
            except ValueError:
                pass
    sl = wc.Points.single_level(*zip(*el))
    rng = np.random.default_rng(0)
    hier = wc.Points.hierarchical([[np.column_stack([10.0 ** np.arange(-1, 3), rng.uniform(0, 100, 4)]) for _ in range(3)]
                                   for _ in range(210)])
    return sl, hier


def synthetic_rows(Q, cols, C, n, kind, dev):
    import torch
    x = torch.empty((n, Q, cols, C), dtype=torch.float64, device=dev)
    if kind == "hierarchical":
        x[:, :, :4] = 1.0
        x[:, :, 4:cols - 2:2] = 5.5 + 0.3 * torch.randn((n, Q, (cols - 6) // 2, C), dtype=torch.float64, device=dev)
        x[:, :, 5:cols - 2:2] = 1.0 + 0.1 * torch.randn((n, Q, (cols - 6) // 2, C), dtype=torch.float64, device=dev)
    else:
        x[:, :, 0] = 5.5 + 0.3 * torch.randn((n, Q, C), dtype=torch.float64, device=dev)
        x[:, :, 1] = 1.0 + 0.1 * torch.randn((n, Q, C), dtype=torch.float64, device=dev)
    x[:, :, cols - 2] = 8.0 + torch.rand((n, Q, C), dtype=torch.float64, device=dev)
    x[:, :, cols - 1] = -40.0
    return x


def measure(name, segments, dev, points):
    import torch
    from pyhillfit_amd.waic import PointwiseWAIC, workspace_bytes
    sh = SHAPES[name]
    pts = points[1] if sh["kind"] == "hierarchical" else points[0]
    Q, C, seg = pts.num_problems, sh["chains"], sh["seg"]
    cols = 5 + 2 * pts.num_expts + 1 if sh["kind"] == "hierarchical" else 4
    total = seg * (segments + 2)
    rows = synthetic_rows(Q, cols, C, seg, sh["kind"], dev)
    w = PointwiseWAIC(pts, sh["kind"], Q, C, total, dev)
    w.accumulate(rows)                                     # warm-up segment
    torch.cuda.synchronize(dev)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(segments):
        w.accumulate(rows)
    ev1.record()
    torch.cuda.synchronize(dev)
    ms = ev0.elapsed_time(ev1) / segments
    t0 = time.time()
    w.accumulate(rows)
    w.result()
    final_ms = (time.time() - t0) * 1e3
    n_points = int(pts.count.sum())
    out = {"shape": name, "problems": Q, "points": n_points, "chains": C, "columns": cols, "rows_per_segment": seg,
           "ms_per_segment": round(ms, 3), "ns_per_point_draw": round(ms * 1e6 / (seg * C * n_points), 4),
           "ms_per_run_estimate": round(ms / seg * sh["run_rows"], 1),
           "workspace_gb": round(workspace_bytes(Q, pts.stride, C, sh["run_rows"]) / 1e9, 3),
           "last_segment_plus_result_ms": round(final_ms, 1)}
    del w, rows
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="cli,c3,c4")
    ap.add_argument("--segments", type=int, default=3)
    a = ap.parse_args()
    dev = "cuda:0"
    points = crumb_points()
    res = [measure(n, a.segments, dev, points) for n in a.shapes.split(",")]
    print(json.dumps({"tool": "bench_waic", "results": res}))


if __name__ == "__main__":
    main()
