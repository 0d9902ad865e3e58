"""Measurement of the streaming posterior quantiles (phf_quantiles_accumulate, phf_quantiles_accumulate_curves): the time of
accumulate() per segment at three shapes, against the sampling time of the same segment.  One JSON line.

    python tools/bench_quantiles.py [--shapes cli,c3,c4] [--segments 3] [--bins 16384] [--curve-bands 64]
    python tools/bench_quantiles.py --hier-bands [--shapes hier_cli,c4] [--band-points 40,64] [--out FILE]

  cli  the single-level command line's defaults: the 210 Crumb pairs x 64 chains x 4 columns, model 2, segments of 4 000 rows
       (20 000 iterations at thinning 5)
  c3   BASELINE C3: the same pairs x 4 096 chains, segments of 4 800 rows
  c4   BASELINE C4: 210 hierarchical problems of Ne = 3 (12 columns) x 1 024 chains, segments of 4 000 rows
  hier_cli  the hierarchical command line's defaults: the same 210 problems x 128 chains, segments of 4 000 rows
Rows are synthetic draws near a posterior (the histograms' cost depends on the values only through how they crowd into bins).
Curve bands (single-level shapes) are timed at G doses per pair on their own.  Sampling: the samplers on the Crumb pairs (C4: the
Ne = 3 pairs repeated to 210 problems), one segment of the same rows after one warm-up segment.
--hier-bands: the hierarchical bands (phf_quantiles_accumulate_hier_curves: the underlying effect and a future experiment at G doses
per problem, 2 G slots) on their own at the hierarchical shapes, beside the hierarchical sampler's segment time of the same run."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = {"cli": dict(chains=64, cols=4, seg=4000, kind="single"),
          "c3": dict(chains=4096, cols=4, seg=4800, kind="single"),
          "c4": dict(chains=1024, cols=12, seg=4000, kind="hierarchical"),
          "hier_cli": dict(chains=128, cols=12, seg=4000, kind="hierarchical")}
THINNING = 5


def crumb():
    from pyhillfit_amd import doseresponse as dr
    dr.setup(os.path.join(REPO, "data", "crumb_dataset.json"))
    dr.define_model(2)
    single, ne3 = [], []
    for d in dr.drugs:
        for c in dr.channels:
            try:
                ne, _, ex = dr.load_crumb_data(d, c)
                concs, y = dr.concatenate_experiments(ne, ex)
            except Exception:
                continue
            single.append((concs, y))
            if ne == 3:
                ne3.append(ex)
    return dr, single, ne3


def synthetic_rows(Q, cols, C, n, dev):
    import torch
    x = 5.5 + 0.3 * torch.randn((n, Q, cols, C), dtype=torch.float64, device=dev)
    x[:, :, 1] = 1.0 + 0.1 * torch.randn((n, Q, C), dtype=torch.float64, device=dev)
    x[:, :, cols - 1] = -40.0 + torch.randn((n, Q, C), dtype=torch.float64, device=dev)
    return x


def hierarchical_rows(Q, cols, C, n, dev):
    """synthetic_rows with (alpha, beta, mu, s) near a hierarchical posterior in columns 0..3"""
    import torch
    x = synthetic_rows(Q, cols, C, n, dev)
    for col, (m, sd) in enumerate(((1.0, 0.1), (5.0, 0.5), (5.5, 0.3), (0.3, 0.03))):
        x[:, :, col] = m + sd * torch.randn((n, Q, C), dtype=torch.float64, device=dev)
    return x


def timed(fn, reps, dev):
    import torch
    torch.cuda.synchronize(dev)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(reps):
        fn()
    ev1.record()
    torch.cuda.synchronize(dev)
    return ev0.elapsed_time(ev1) / reps


def sampling_ms(name, data, dev):
    """one segment of the sampler at the shape, after a warm-up segment"""
    import numpy as np
    import torch
    sh = SHAPES[name]
    dr, single, ne3 = data
    C, iters = sh["chains"], sh["seg"] * THINNING
    if sh["kind"] == "single":
        from pyhillfit_amd import bestfit
        from pyhillfit_amd.sampler import SingleLevelSampler
        th0 = [bestfit.chain_start(t, 2) for t in bestfit.best_fit_batch(single, 2)[0]]
        s = SingleLevelSampler(dr.PackedPoints(single), 2, list(range(len(single))), [1.0] * len(single), C, thinning=THINNING,
                               seed=25, adapt_start=3000, device=dev)
        s.init(np.array(th0), cov_identity=False, cov_scale=0.05)
    else:
        from pyhillfit_amd import hierarchical as H
        exs = [ne3[i % len(ne3)] for i in range(210)]
        s = H.HierarchicalSampler(H.PackedHierPoints(exs), list(range(210)), C, thinning=THINNING, seed=25,
                                  problem_ids=list(range(210)), device=dev)
        th0 = np.array([1., 5., 6., .3, 6., .8, 6.1, .7, 6.0, .9, 0.5])
        s.init(np.tile(th0, (210, 1)), cov_scale=0.01)
    s.reserve(3 * iters)
    buf = torch.empty((sh["seg"], s.Q, s.d + 1, C), dtype=torch.float64, device=dev)
    s.advance(iters, out=buf)
    ms = timed(lambda: s.advance(iters, out=buf), 1, dev)
    del s, buf
    return ms


def measure(name, segments, bins, G, dev, data):
    import numpy as np
    import torch
    from pyhillfit_amd import quantiles as qn
    sh = SHAPES[name]
    Q, C, cols, seg = 210, sh["chains"], sh["cols"], sh["seg"]
    total = seg * (segments + 2)
    rows = synthetic_rows(Q, cols, C, seg, dev)
    out = {"shape": name, "pairs": Q, "chains": C, "columns": cols, "rows_per_segment": seg, "bins": bins}
    q = qn.PosteriorQuantiles(Q, C, cols, total, qn.DEFAULT_PROBS, bins, dev)
    q.accumulate(rows)                                         # the first segment: anchors and levels
    out["ms_per_segment"] = round(timed(lambda: q.accumulate(rows), segments, dev), 3)
    out["workspace_gb"] = round(q.nbytes / 1e9, 3)
    q.accumulate(rows)
    out["reduce_ms"] = round(timed(q.reduced, 1, dev), 2)
    q.free()
    del q
    if sh["kind"] == "single" and G:
        _, single, _ = data
        lnd = np.log(np.array([qn.curve_doses(c, G) for c, _ in single][:Q]))
        b = qn.PosteriorQuantiles(Q, C, 0, total, qn.DEFAULT_PROBS, bins, dev, curve_ln_doses=lnd, model=2)
        b.accumulate(rows)
        out["curve_points"] = G
        out["curve_ms_per_segment"] = round(timed(lambda: b.accumulate(rows), segments, dev), 3)
        out["curve_workspace_gb"] = round(b.nbytes / 1e9, 3)
        b.free()
        del b
    del rows
    torch.cuda.empty_cache()
    try:
        out["sampling_ms_per_segment"] = round(sampling_ms(name, data, dev), 2)
        out["quantiles_over_sampling"] = round(out["ms_per_segment"] / out["sampling_ms_per_segment"], 4)
        if "curve_ms_per_segment" in out:
            out["curves_over_sampling"] = round(out["curve_ms_per_segment"] / out["sampling_ms_per_segment"], 4)
    except Exception as e:                                     # the figure of the accumulator stands without it
        out["sampling_error"] = repr(e)[:200]
    torch.cuda.empty_cache()
    return out


def measure_hier_bands(name, segments, bins, points, dev, data):
    import numpy as np
    import torch
    from pyhillfit_amd import quantiles as qn
    sh = SHAPES[name]
    if sh["kind"] != "hierarchical":
        raise SystemExit("--hier-bands times the hierarchical shapes (hier_cli, c4), not %s" % name)
    Q, C, cols, seg = 210, sh["chains"], sh["cols"], sh["seg"]
    total = seg * (segments + 1)
    _, _, ne3 = data
    concs = [np.concatenate([np.asarray(e)[:, 0] for e in ne3[i % len(ne3)]]) for i in range(Q)]
    rows = hierarchical_rows(Q, cols, C, seg, dev)
    out = {"shape": name, "pairs": Q, "chains": C, "columns": cols, "rows_per_segment": seg, "bins": bins, "bands": []}
    for G in points:
        lnd = np.log(np.array([qn.curve_doses(c, G) for c in concs]))
        b = qn.PosteriorQuantiles(Q, C, 0, total, qn.DEFAULT_PROBS, bins, dev, band_ln_doses=lnd, seed=25, problem_ids=list(range(Q)))
        b.accumulate(rows)                                     # the first segment: anchors and levels
        rec = {"doses": G, "slots_per_problem": 2 * G, "band_ms_per_segment": round(timed(lambda: b.accumulate(rows), segments, dev), 3),
               "band_workspace_gb": round(b.nbytes / 1e9, 3)}
        red = b.reduced()
        rec["non_finite"] = int(red[..., 3].sum())
        out["bands"].append(rec)
        b.free()
        del b
    del rows
    torch.cuda.empty_cache()
    out["sampling_ms_per_segment"] = round(sampling_ms(name, data, dev), 2)
    for rec in out["bands"]:
        rec["bands_over_sampling"] = round(rec["band_ms_per_segment"] / out["sampling_ms_per_segment"], 4)
    torch.cuda.empty_cache()
    return out


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=None, help="default cli,c3,c4; with --hier-bands hier_cli,c4")
    ap.add_argument("--segments", type=int, default=3)
    ap.add_argument("--bins", type=int, default=16384)
    ap.add_argument("--curve-bands", type=int, default=64)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--hier-bands", action="store_true", help="time the hierarchical bands instead, at the hierarchical shapes")
    ap.add_argument("--band-points", default="40,64", help="--hier-bands: doses per problem, comma-separated")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    dev = torch.device(a.device)
    data = crumb()
    if a.hier_bands:
        points = [int(g) for g in a.band_points.split(",")]
        res = [measure_hier_bands(n, a.segments, a.bins, points, dev, data) for n in (a.shapes or "hier_cli,c4").split(",")]
        line = json.dumps({"bench": "hier_bands", "device": torch.cuda.get_device_name(dev), "results": res})
    else:
        res = [measure(n, a.segments, a.bins, a.curve_bands, dev, data) for n in (a.shapes or "cli,c3,c4").split(",")]
        line = json.dumps({"bench": "quantiles", "device": torch.cuda.get_device_name(dev), "results": res})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
