"""Measurement of the streaming power-scaling sensitivity (phf_sensitivity_accumulate): the time of accumulate() per segment at three
shapes, beside the sampler's time for a segment of the same rows, measured in the same run.  One JSON line.

    python tools/bench_sensitivity.py [--shapes cli,c3,hier_cli] [--segments 2] [--bins 4096] [--delta 0.01] [--out FILE]

  cli       the single-level command line's defaults: the 210 Crumb pairs x 64 chains, model 2 (3 parameter columns of 4), segments of
            4 000 rows (20 000 iterations at thinning 5)
  c3        BASELINE C3: the same pairs x 4 096 chains, segments of 4 800 rows
  hier_cli  the hierarchical command line's defaults: 210 problems of Ne = 3 (11 parameter columns of 12) x 128 chains, segments of
            4 000 rows
The rows are the sampler's own: a warm-up segment, then one timed segment whose rows feed the accumulator (the components are
evaluated on real draws of the pairs' posteriors).  No target is set: the figures are written down as they come."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_quantiles import THINNING, crumb, timed  # noqa: E402

SHAPES = {"cli": dict(chains=64, seg=4000, kind="single"),
          "c3": dict(chains=4096, seg=4800, kind="single"),
          "hier_cli": dict(chains=128, seg=4000, kind="hierarchical")}


def sampler_for(name, data, dev):
    import numpy as np
    sh = SHAPES[name]
    dr, single, ne3 = data
    C = sh["chains"]
    if sh["kind"] == "single":
        from pyhillfit_amd import bestfit
        from pyhillfit_amd.sampler import SingleLevelSampler
        th0 = [bestfit.chain_start(t, 2) for t in bestfit.best_fit_batch(single, 2)[0]]
        s = SingleLevelSampler(dr.PackedPoints(single), 2, list(range(len(single))), [1.0] * len(single), C, thinning=THINNING,
                               seed=25, adapt_start=3000, device=dev)
        s.init(np.array(th0), cov_identity=False, cov_scale=0.05)
        return s, 2, None
    from pyhillfit_amd import hierarchical as H
    exs = [ne3[i % len(ne3)] for i in range(210)]
    s = H.HierarchicalSampler(H.PackedHierPoints(exs), list(range(210)), C, thinning=THINNING, seed=25,
                              problem_ids=list(range(210)), device=dev)
    th0 = np.array([1., 5., 6., .3, 6., .8, 6.1, .7, 6.0, .9, 0.5])
    s.init(np.tile(th0, (210, 1)), cov_scale=0.01)
    return s, "hierarchical", s.prior


def measure(name, segments, bins, delta, dev, data):
    import torch
    from pyhillfit_amd import sensitivity as sn
    sh = SHAPES[name]
    C, seg = sh["chains"], sh["seg"]
    iters = seg * THINNING
    s, kind, prior = sampler_for(name, data, dev)
    s.reserve(3 * iters)
    buf = torch.empty((seg, s.Q, s.d + 1, C), dtype=torch.float64, device=dev)
    s.advance(iters, out=buf)                                  # warm-up: past the start of the adaptation
    out = {"shape": name, "pairs": s.Q, "chains": C, "columns": s.d, "rows_per_segment": seg, "bins": bins, "delta": delta}
    out["sampling_ms_per_segment"] = round(timed(lambda: s.advance(iters, out=buf), 1, dev), 2)
    ps = sn.PowerScaling(s.points, kind, s.Q, C, s.d, seg * (segments + 1), delta, bins, dev, prior=prior)
    ps.accumulate(buf)                                         # the first segment: anchors, reference components, levels
    out["ms_per_segment"] = round(timed(lambda: ps.accumulate(buf), segments, dev), 3)
    out["workspace_gb"] = round(ps.nbytes / 1e9, 3)
    out["reduce_ms"] = round(timed(ps.reduced, 1, dev), 2)
    res = ps.result()
    out["sensitivity_over_sampling"] = round(out["ms_per_segment"] / out["sampling_ms_per_segment"], 4)
    out["lowest_ess_fraction"] = float(res["ess_fraction"].min())
    out["clamped"] = int(res["clamped"].sum())
    out["flagged_columns"] = int((res["diagnosis"] != sn.DIAGNOSES[3]).sum())
    ps.free()
    del ps, s, buf
    torch.cuda.empty_cache()
    return out


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="cli,c3,hier_cli")
    ap.add_argument("--segments", type=int, default=2)
    ap.add_argument("--bins", type=int, default=4096)
    ap.add_argument("--delta", type=float, default=0.01)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    dev = torch.device(a.device)
    data = crumb()
    res = [measure(n, a.segments, a.bins, a.delta, dev, data) for n in a.shapes.split(",")]
    line = json.dumps({"bench": "sensitivity", "device": torch.cuda.get_device_name(dev), "results": res})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
