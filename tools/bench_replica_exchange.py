"""Cost of replica exchange (PyHillTemp --swap-every K, pyhillfit_amd/replica_exchange.py).  One JSON line.

    python tools/bench_replica_exchange.py [--parts cli,c5,round] [--every 0,5,20,100]

  cli    wall time of `PyHillTemp -d 0 -c 0 -m 2` (500 000 iterations, 41 rungs x 64 chains) in a child process per K (0 = no swaps)
  c5     BASELINE C5's tempered batch (210 pairs x 32 rungs x 1 024 chains, model 2, moments on): device time of 20 000 iterations per
         K, after 4 000 iterations of warm-up (the cost of a swap is mostly the extra launches: the state goes through HBM and the
         LDS tables reload at every sub-advance)
  round  device time of one swap round alone at both shapes (20 rounds, both parities)
For the swap kernel's share under the profiler run `rocprofv3 --kernel-trace --stats -- python tools/bench_replica_exchange.py
--parts round` in a run of its own."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def cli(every_list, iterations):
    from pyhillfit_amd import doseresponse as dr
    dr.setup(os.path.join(REPO, "data", "crumb_dataset.json"))
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        csv = os.path.join(tmp, "crumb_data.csv")
        dr.table.to_csv(csv)
        for k in every_list:
            cmd = [sys.executable, "-m", "pyhillfit_amd.PyHillTemp", "--data-file", csv, "-m", "2", "-d", "0", "-c", "0",
                   "-i", str(iterations), "--output-root", os.path.join(tmp, "k%d" % k), "--swap-every", str(k)]
            t0 = time.time()
            p = subprocess.run(cmd, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            wall = time.time() - t0
            if p.returncode != 0:
                raise SystemExit(p.stdout[-3000:])
            line = [l for l in p.stdout.splitlines() if l.startswith("replica exchange")]
            out.append({"every": k, "iterations": iterations, "wall_s": round(wall, 2), "report": line[0] if line else None})
    return out


def batch(dev, pairs_all, rungs, chains, model=2):
    import numpy as np
    from pyhillfit_amd import doseresponse as dr
    from pyhillfit_amd.sampler import SingleLevelSampler
    dr.setup(os.path.join(REPO, "data", "crumb_dataset.json"))
    pairs = [(a, b) for a in dr.drugs for b in dr.channels] if pairs_all else [("Amiodarone", "hERG")]
    t = dr.temperature_ladder(rungs - 1)
    packed = dr.pack_single_level(pairs)
    pair_index = np.repeat(np.arange(len(pairs)), rungs)
    s = SingleLevelSampler(packed, model, pair_index, np.tile(t, len(pairs)), chains, thinning=5, seed=1, adapt_start=3000,
                           reset_mean_at_adapt_start=True, problem_ids=np.arange(len(pair_index)), device=dev)
    s.init(np.ones(model + 1), cov_identity=True, cov_scale=1.0)
    s.enable_moments(after_iteration=0)
    return s, rungs


def c5(every_list, dev, iterations=20000, warm=4000):
    import torch
    from pyhillfit_amd.replica_exchange import ReplicaExchange
    out = []
    for k in every_list:
        s, R = batch(dev, True, 32, 1024)
        s.reserve(warm + iterations)
        rx = ReplicaExchange(s, R) if k else None
        go = (lambda n: s.advance(n, save=False)) if rx is None else (lambda n: rx.advance(n, every=k, save=False))
        go(warm)
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.time()
        e0.record()
        go(iterations)
        e1.record()
        torch.cuda.synchronize(dev)
        res = {"every": k, "iterations": iterations, "device_s": round(e0.elapsed_time(e1) / 1000, 3), "wall_s": round(time.time() - t0, 3)}
        if rx is not None:
            st = rx.statistics()
            rate = st["accepts"].sum(axis=0) / st["attempts"].sum(axis=0)
            res.update({"mean_accept_rate": round(float(rate.mean()), 4), "lowest_accept_rate": round(float(rate.min()), 4)})
        out.append(res)
        del s, rx
        torch.cuda.empty_cache()
    return out


def rounds(dev, n=20):
    import torch
    from pyhillfit_amd.replica_exchange import ReplicaExchange
    out = []
    for name, (pairs_all, R, C) in (("cli", (False, 41, 64)), ("c5", (True, 32, 1024))):
        s, _ = batch(dev, pairs_all, R, C)
        s.reserve(200)
        s.advance(100, save=False)
        rx = ReplicaExchange(s, R)
        rx.swap_round(1)
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for r in range(2, 2 + n):
            rx.swap_round(r)
        e1.record()
        torch.cuda.synchronize(dev)
        out.append({"shape": name, "problems": s.Q, "chains": C, "us_per_round": round(1000 * e0.elapsed_time(e1) / n, 1)})
        del s, rx
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="cli,c5,round")
    ap.add_argument("--every", default="0,5,20,100")
    ap.add_argument("--iterations", type=int, default=500000, help="iterations of the cli part")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    ks = [int(x) for x in args.every.split(",")]
    parts = args.parts.split(",")
    res = {"bench": "replica_exchange"}
    if "round" in parts:
        res["round"] = rounds(args.device)
    if "c5" in parts:
        res["c5"] = c5(ks, args.device)
    if "cli" in parts:
        res["cli"] = cli(ks, args.iterations)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
