"""Measurements of the drug profile (pyhillfit_amd/drug_profile.py; results under profiles/drug_profile/).

    python tools/bench_drug_profile.py kernel [--rows 4000] [--doses 3] [--bins 4096]
    python tools/bench_drug_profile.py run --output-root DIR [--tree CHECKOUT] [--flag] [-- extra PyHillFit flags]
    python tools/bench_drug_profile.py records OUTPUT_DIR Verapamil Quinidine

  kernel   ms per segment of phf_drug_profile_accumulate (HIP events, the median of five launches after a warm-up) on the single-level
           command line's shape: the 30 Crumb drugs x 7 channels (210 problems) x 64 chains, `--rows` saved rows a segment (the default
           segment of 20 000 iterations at thinning 5), `--doses` doses a drug, on synthetic draws near a posterior.
  run      one `PyHillFit -m 2 -a` of the Crumb set in a child process, with `--drug-profile-cmax tests/golden/drug_profile/drug_list.txt`
           (--flag) or without, from this checkout or from --tree: the wall time and the run's own "timing" line.  One JSON line.
  records  from the drug files of such a run: per named drug and dose the medians and 95 % intervals of the net block and of every
           channel's block, p_net_positive and the dominant-channel probabilities."""
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
CMAX_FILE = os.path.join(REPO, "tests", "golden", "drug_profile", "drug_list.txt")


def kernel(a):
    import numpy as np
    import torch
    from pyhillfit_amd import doseresponse as dr
    from pyhillfit_amd import drug_profile as dp
    from pyhillfit_amd.quantiles import DEFAULT_PROBS
    dev = "cuda:0"
    dr.setup(os.path.join(REPO, "data", "crumb_dataset.json"))
    channels = [dr._clean(c) for c in dr.channels]
    pairs = [(d, c) for d in dr.drugs for c in channels]
    plan = dp.Plan(pairs, channels, None, dp.read_cmax(CMAX_FILE), tuple(float(3 ** i) for i in range(a.doses)))
    Q, C = len(pairs), 64
    x = torch.zeros((a.rows, Q, 4, C), dtype=torch.float64, device=dev)
    x[:, :, 0] = 5.0 + 0.5 * torch.randn((a.rows, Q, C), dtype=torch.float64, device=dev)
    x[:, :, 1] = 0.6 + 0.8 * torch.rand((a.rows, Q, C), dtype=torch.float64, device=dev)
    acc = dp.DrugProfile(2, Q, C, plan.map, plan.weights, plan.doses, 7 * a.rows, DEFAULT_PROBS, a.bins, dev)
    acc.accumulate(x)                                                  # warm-up: code object, the grids' first levels
    torch.cuda.synchronize(dev)
    t = []
    for _ in range(5):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        acc.accumulate(x)
        ev1.record()
        torch.cuda.synchronize(dev)
        t.append(ev0.elapsed_time(ev1))
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    acc.result()
    ev1.record()
    torch.cuda.synchronize(dev)
    ms = float(np.median(t))
    print(json.dumps({"tool": "bench_drug_profile", "mode": "kernel", "drugs": len(plan.drugs), "channels": len(channels), "doses": a.doses,
                      "problems": Q, "chains": C, "bins": a.bins, "rows_per_segment": a.rows, "workspace_MB": round(acc.nbytes / 1e6, 1),
                      "ms_per_segment": round(ms, 3), "ms_per_segment_all": [round(v, 3) for v in t],
                      "ns_per_draw_and_dose": round(1e6 * ms / (a.rows * C * len(plan.drugs) * a.doses), 3),
                      "result_ms": round(ev0.elapsed_time(ev1), 3)}))
    acc.free()


def run(a, extra):
    cmd = [sys.executable, "-m", "pyhillfit_amd.PyHillFit", "--data-file", os.path.join(REPO, "data", "crumb_dataset.json"), "-m", "2",
           "-a", "--output-root", a.output_root] + extra
    if a.flag:
        cmd += ["--drug-profile-cmax", CMAX_FILE]
    t0 = time.time()
    # a whole Crumb run takes a minute or two; the limit ends a child that hangs (subprocess.run kills it and raises)
    p = subprocess.run(cmd, cwd=a.tree or REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=a.limit)
    wall = time.time() - t0
    lines = p.stdout.splitlines()
    timing = [l for l in lines if l.startswith("timing [rank")]
    m = re.search(r"sampling ([0-9.]+) s", timing[-1]) if timing else None
    files = glob.glob(os.path.join(a.output_root, "**", "drug_profiles", "*_drug_profile.json"), recursive=True)
    print(json.dumps({"tool": "bench_drug_profile", "mode": "run", "tree": a.tree or REPO, "flags": cmd[cmd.index("-a") + 1:],
                      "returncode": p.returncode, "wall_seconds": round(wall, 1), "sampling_seconds": float(m.group(1)) if m else None,
                      "timing": timing[-1] if timing else None, "report": [l for l in lines if l.startswith("drug-profile [rank")],
                      "drug_files": len(files), "tail": lines[-5:] if p.returncode else []}))
    return p.returncode


def records(a):
    out = []
    for drug in a.names[1:]:
        found = glob.glob(os.path.join(a.names[0], "**", "drug_profiles", "%s_drug_profile.json" % drug), recursive=True)
        if not found:
            out.append("# %s: no drug file" % drug)
            continue
        with open(found[0]) as f:
            rec = json.load(f)
        i50, lo, hi = rec["probs"].index(0.5), rec["probs"].index(0.025), rec["probs"].index(0.975)
        out.append("# {}: model {}, {} chains x {} rows, Cmax {} uM, weights {}".format(drug, rec["model"], rec["chains"], rec["rows"],
                                                                                        rec["cmax_uM"], rec["weights"]))
        for d in rec["doses"]:
            out.append("  dose {:.4g} uM: net block median {:+.2f} [{:+.2f}, {:+.2f}] percentage points; p(net > 0) = {:.4f} (even chains {:.4f}, "
                       "odd {:.4f}); draws used {}, skipped {}".format(d["dose_uM"], d["net"]["value"][i50], d["net"]["value"][lo],
                                                                       d["net"]["value"][hi], d["p_net_positive"],
                                                                       d["by_chain_parity"]["even"]["p_net_positive"],
                                                                       d["by_chain_parity"]["odd"]["p_net_positive"], d["draws_used"],
                                                                       d["draws_skipped"]))
            for ch in rec["channels_loaded"]:
                b = d["block"][ch]
                out.append("    {:<12} block median {:6.2f} [{:6.2f}, {:6.2f}] %; most blocked in {:.4f} of the draws".format(
                    ch, b["value"][i50], b["value"][lo], b["value"][hi], d["dominant_probability"][ch]))
    print("\n".join(out))


def main():
    argv = sys.argv[1:]
    extra = []
    if "--" in argv:
        extra = argv[argv.index("--") + 1:]
        argv = argv[:argv.index("--")]
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernel", "run", "records"])
    ap.add_argument("names", nargs="*", help="records: the output directory of a run with the flag, then drug names")
    ap.add_argument("--rows", type=int, default=4000)
    ap.add_argument("--doses", type=int, default=3)
    ap.add_argument("--bins", type=int, default=4096)
    ap.add_argument("--output-root", default="output")
    ap.add_argument("--tree", default=None, help="run: the checkout whose PyHillFit runs (default: this one)")
    ap.add_argument("--limit", type=float, default=600.0, help="run: seconds after which the child run is ended")
    ap.add_argument("--flag", action="store_true")
    a = ap.parse_args(argv)
    if a.mode == "kernel":
        kernel(a)
    elif a.mode == "run":
        sys.exit(run(a, extra))
    else:
        if len(a.names) < 2:
            ap.error("records needs the output directory of a run with the flag and at least one drug name")
        records(a)


if __name__ == "__main__":
    main()
