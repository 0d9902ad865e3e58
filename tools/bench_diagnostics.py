"""Measurement of the streaming convergence diagnostics (phf_diagnostics_accumulate): the time of accumulate() per segment at
three shapes, scaled to a whole run.  One JSON line.

    python tools/bench_diagnostics.py [--lags 256] [--shapes cli,c3,c4] [--segments 3]

  cli  the single-level command line's defaults: 210 pairs x 64 chains x 4 columns, 75 001 post-burn-in rows, segments of 4 000
  c3   BASELINE C3: 210 pairs x 4 096 chains x 4 columns, segments of 4 800 rows
  c4   BASELINE C4: 210 hierarchical pairs (Ne = 3 shape: 12 columns) x 1 024 chains, segments of 4 000 rows
The rows are synthetic (the cost does not depend on their values); flop = 2 per (row, lag, column, chain)."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = {"cli": dict(pairs=210, chains=64, cols=4, seg=4000, run_rows=75001),
          "c3": dict(pairs=210, chains=4096, cols=4, seg=4800, run_rows=75001),
          "c4": dict(pairs=210, chains=1024, cols=12, seg=4000, run_rows=75001)}


def measure(name, lags, segments, dev):
    import torch
    from pyhillfit_amd.diagnostics import ChainDiagnostics, workspace_bytes
    sh = SHAPES[name]
    Q, C, cols, seg = sh["pairs"], sh["chains"], sh["cols"], sh["seg"]
    total = seg * (segments + 2)
    rows = torch.randn((seg, Q, cols, C), dtype=torch.float64, device=dev)
    d = ChainDiagnostics(Q, C, cols, total, lags, dev)
    d.accumulate(rows)                                     # warm-up segment (the first rows of half 0)
    torch.cuda.synchronize(dev)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(segments):
        d.accumulate(rows)
    ev1.record()
    torch.cuda.synchronize(dev)
    ms = ev0.elapsed_time(ev1) / segments
    t0 = time.time()
    d.accumulate(rows)
    d.result()
    final_ms = (time.time() - t0) * 1e3
    per_row_ms = ms / seg
    flop = 2.0 * seg * d.L * cols * C * Q
    out = {"shape": name, "pairs": Q, "chains": C, "columns": cols, "rows_per_segment": seg, "lags": d.L,
           "ms_per_segment": round(ms, 3), "tflops": round(flop / ms / 1e9, 2),
           "ms_per_run_estimate": round(per_row_ms * sh["run_rows"], 1),
           "workspace_gb_at_run_rows": round(workspace_bytes(Q, cols, C, sh["run_rows"], lags) / 1e9, 2),
           "last_segment_plus_result_ms": round(final_ms, 1)}
    del d, rows
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lags", type=int, default=256)
    ap.add_argument("--shapes", default="cli,c3,c4")
    ap.add_argument("--segments", type=int, default=3)
    a = ap.parse_args()
    dev = "cuda:0"
    res = [measure(n, a.lags, a.segments, dev) for n in a.shapes.split(",")]
    print(json.dumps({"tool": "bench_diagnostics", "results": res}))


if __name__ == "__main__":
    main()
