"""Compare fits by WAIC or PSIS-LOO: the elpd difference of every two summaries and its pointwise standard error (Vehtari, Gelman &
Gabry 2017).

    python -m pyhillfit_amd.compare_models SUMMARY_A SUMMARY_B [...] [--intersection] [--criterion {waic,loo,logo}]

Each argument is a `<chain>_summary.json` written with --waic (--criterion waic, the default) or --loo (--criterion loo), or an
output directory searched for them.  The summaries of each
argument are keyed by (drug, channel); for every two arguments A, B (in the order given) and every pair both hold:

    elpd_diff = sum_i (elpd_A,i - elpd_B,i),  se_diff = sqrt(n var_i(elpd_A,i - elpd_B,i)),  preferred: A if elpd_diff > 2 se_diff,
    B if elpd_diff < -2 se_diff, else neither.

Points are aligned by (experiment, dose, response) (replicates in order of appearance).  Pairs whose point sets differ are refused
(an error entry) unless --intersection asks for the common points.  Points where one fit has a censored MASS (single-level,
y == 0 or 100) and the other a DENSITY (uncensored or the hierarchical truncated normal) are compared all the same but counted as
"mixed": their log-likelihoods are not on one scale.  Model 1 against model 2 has none; single-level against hierarchical has one per
censored point.  With --criterion loo the pointwise elpd_loo are compared; a pair where either fit has a common point with Pareto
k-hat above its threshold is marked ("khat_flagged": its difference rests on unreliable points), and a pair where either fit has a
point without an elpd_loo (not determined, or -inf) is refused.  With --criterion logo two HIERARCHICAL summaries written with
--leave-experiment-out are compared (for example -Ne subsets or different seeds): the integrated leave-one-experiment-out elpd_i of the
experiments both hold, aligned by the experiment's label; a single-level summary is refused (it has no experiment-level parameters to
integrate out, and a pooled fit scored on the same scale would still give censored points a mass, not a density).  One JSON object
on stdout, then a table on stderr."""
import argparse
import glob
import json
import os
import sys

import numpy as np

CENSORED = ("censored-0", "censored-100")
OBJECT = {"waic": "waic", "loo": "loo", "logo": "loo_experiment"}       # the summary's object of each criterion
FLAG = {"waic": "--waic", "loo": "--loo", "logo": "--hierarchical --leave-experiment-out"}


def load_sources(path, criterion="waic"):
    """{(drug, channel): summary} of a summary file or of every summary under a directory (those with a `criterion` object)"""
    files = [path] if os.path.isfile(path) else sorted(glob.glob(os.path.join(path, "**", "*_summary.json"), recursive=True))
    out = {}
    for f in files:
        with open(f) as fh:
            s = json.load(fh)
        if criterion == "logo" and "model" in s and "num_expts" not in s:
            raise SystemExit("%s is a single-level summary (model %s): --criterion logo compares hierarchical fits only — the integrated "
                             "leave-one-experiment-out integrates experiment-level parameters a single-level fit does not have" % (f, s["model"]))
        if OBJECT[criterion] not in s:
            continue
        out[(s["drug"], s["channel"])] = dict(s, _file=f)
    if not out:
        raise SystemExit("%s: no summary with a \"%s\" object (run with %s)" % (path, OBJECT[criterion], FLAG[criterion]))
    return out


def _keys(w):
    """(experiment, dose, response, occurrence) of every point: replicates of one (experiment, dose, response) in order"""
    seen, keys = {}, []
    pts = w["points"]
    for e, d, y in zip(pts["experiment"], pts["dose"], pts["response"]):
        k = (int(e), float(d), float(y))
        seen[k] = seen.get(k, 0) + 1
        keys.append(k + (seen[k],))
    return keys


def compare(wa, wb, intersection=False, criterion="waic"):
    """two "waic" (or, criterion "loo", two "loo") objects -> dict of the comparison (or with "error" if the point sets differ and
    intersection is not asked, or a loo point has no elpd_loo)"""
    ka, kb = _keys(wa), _keys(wb)
    ia, ib = {k: i for i, k in enumerate(ka)}, {k: i for i, k in enumerate(kb)}
    common = [k for k in ka if k in ib]
    only_a, only_b = len(ka) - len(common), len(kb) - len(common)
    rec = {"n_points": len(common), "n_only_a": only_a, "n_only_b": only_b}
    if (only_a or only_b) and not intersection:
        rec["error"] = "point sets differ ({} only in A, {} only in B): use --intersection to compare the common points".format(only_a, only_b)
        return rec
    field = "elpd_loo" if criterion == "loo" else "elpd"
    if criterion == "loo":
        missing = [sum(1 for k in common if w["pointwise"]["elpd_loo"][i[k]] is None) for w, i in ((wa, ia), (wb, ib))]
        if any(missing):
            rec["error"] = ("points without an elpd_loo (not determined: raise --loo-tail-per-chain; or -inf): {} in A, {} in B"
                            .format(*missing))
            return rec
    ea = np.array([wa["pointwise"][field][ia[k]] for k in common], dtype=np.float64)
    eb = np.array([wb["pointwise"][field][ib[k]] for k in common], dtype=np.float64)
    kind_a = [wa["points"]["kind"][ia[k]] for k in common]
    kind_b = [wb["points"]["kind"][ib[k]] for k in common]
    mixed = [(x in CENSORED) != (y in CENSORED) for x, y in zip(kind_a, kind_b)]
    d = ea - eb
    n = len(d)
    diff = float(np.sum(d))
    se = float(np.sqrt(n * np.var(d, ddof=1))) if n > 1 else float("nan")
    pref = "A" if diff > 2 * se else "B" if diff < -2 * se else "neither"
    rec.update({"elpd_a": float(np.sum(ea)), "elpd_b": float(np.sum(eb)), "elpd_diff": diff, "se_diff": se, "preferred": pref,
                "n_mixed": int(sum(mixed))})
    if criterion == "loo":
        ka_ = [wa["pointwise"]["khat"][ia[k]] for k in common]
        kb_ = [wb["pointwise"]["khat"][ib[k]] for k in common]
        na = sum(1 for v in ka_ if v is None or v > wa["khat_threshold"])   # null: an infinite k-hat
        nb = sum(1 for v in kb_ if v is None or v > wb["khat_threshold"])
        rec.update({"n_khat_a": na, "n_khat_b": nb, "khat_flagged": bool(na or nb)})
    if any(mixed):
        rec["warning"] = ("{} points are a censored probability mass in one fit and a density in the other: their elpd are not "
                          "commensurable".format(int(sum(mixed))))
    return rec


def compare_logo(wa, wb, intersection=False):
    """two "loo_experiment" objects -> dict of the comparison over the experiments both hold (aligned by label)"""
    ia = {e["label"]: e for e in wa["experiments"]}
    ib = {e["label"]: e for e in wb["experiments"]}
    common = [k for k in ia if k in ib]
    only_a, only_b = len(ia) - len(common), len(ib) - len(common)
    rec = {"n_points": len(common), "n_only_a": only_a, "n_only_b": only_b, "n_mixed": 0}
    if (only_a or only_b) and not intersection:
        rec["error"] = "experiment sets differ ({} only in A, {} only in B): use --intersection to compare the common experiments".format(only_a, only_b)
        return rec
    if any(ia[k]["n_i"] != ib[k]["n_i"] for k in common):
        rec["error"] = "experiments with the same label hold different numbers of points: not the same data"
        return rec
    missing = [sum(1 for k in common if w[k]["elpd_i"] is None) for w in (ia, ib)]
    if any(missing) or not common:
        rec["error"] = "experiments without an elpd_i (not determined, or -inf): {} in A, {} in B".format(*missing) if common else "no common experiment"
        return rec
    ea = np.array([ia[k]["elpd_i"] for k in common], dtype=np.float64)
    eb = np.array([ib[k]["elpd_i"] for k in common], dtype=np.float64)
    d = ea - eb
    n = len(d)
    diff = float(np.sum(d))
    se = float(np.sqrt(n * np.var(d, ddof=1))) if n > 1 else float("nan")
    pref = "A" if diff > 2 * se else "B" if diff < -2 * se else "neither"
    na = sum(1 for k in common if ia[k]["khat_i"] is None or ia[k]["khat_i"] > wa["khat_threshold"])
    nb = sum(1 for k in common if ib[k]["khat_i"] is None or ib[k]["khat_i"] > wb["khat_threshold"])
    ga = sum(1 for k in common if ia[k]["quadrature_gap_max"] is None or ia[k]["quadrature_gap_max"] > 0.01)
    gb = sum(1 for k in common if ib[k]["quadrature_gap_max"] is None or ib[k]["quadrature_gap_max"] > 0.01)
    rec.update({"elpd_a": float(np.sum(ea)), "elpd_b": float(np.sum(eb)), "elpd_diff": diff, "se_diff": se, "preferred": pref,
                "n_khat_a": na, "n_khat_b": nb, "khat_flagged": bool(na or nb), "n_gap_a": ga, "n_gap_b": gb, "gap_flagged": bool(ga or gb)})
    return rec


def _num(v):
    return None if v is None or not np.isfinite(v) else v


def compare_sources(sources, names, intersection=False, criterion="waic"):
    out = []
    for i in range(len(sources)):
        for j in range(i + 1, len(sources)):
            for key in [k for k in sources[i] if k in sources[j]]:
                sa, sb = sources[i][key], sources[j][key]
                rec = (compare_logo(sa[OBJECT["logo"]], sb[OBJECT["logo"]], intersection) if criterion == "logo" else
                       compare(sa[criterion], sb[criterion], intersection, criterion))
                rec = {k: (_num(v) if isinstance(v, float) else v) for k, v in rec.items()}
                out.append(dict({"drug": key[0], "channel": key[1], "a": names[i], "b": names[j], "file_a": sa["_file"],
                                 "file_b": sb["_file"]}, **rec))
    return out


def table(rows, criterion="waic"):
    if criterion in ("loo", "logo"):
        return _loo_table(rows)
    lines = ["{:<28} {:>10} {:>8} {:>8} {:>6} {:>7}".format("pair (A vs B)", "elpd_diff", "se", "pref.", "n", "mixed")]
    for r in rows:
        name = "{} + {}".format(r["drug"], r["channel"])
        if "error" in r:
            lines.append("{:<28} {}".format(name, r["error"]))
            continue
        lines.append("{:<28} {:>10.2f} {:>8.2f} {:>8} {:>6} {:>7}".format(name, r["elpd_diff"], r["se_diff"] if r["se_diff"] is not None
                                                                       else float("nan"), r["preferred"], r["n_points"], r["n_mixed"]))
    return "\n".join(lines)


def _loo_table(rows):
    lines = ["{:<28} {:>10} {:>8} {:>8} {:>6} {:>7} {:>9}".format("pair (A vs B)", "elpd_diff", "se", "pref.", "n", "mixed", "k>thr A/B")]
    for r in rows:
        name = "{} + {}".format(r["drug"], r["channel"])
        if "error" in r:
            lines.append("{:<28} {}".format(name, r["error"]))
            continue
        lines.append("{:<28} {:>10.2f} {:>8.2f} {:>8} {:>6} {:>7} {:>9}".format(
            name, r["elpd_diff"], r["se_diff"] if r["se_diff"] is not None else float("nan"), r["preferred"], r["n_points"],
            r["n_mixed"], "{}/{}".format(r["n_khat_a"], r["n_khat_b"])))
    return "\n".join(lines)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="compare_models")
    ap.add_argument("summaries", nargs="+", help="<chain>_summary.json files written with --waic / --loo, or output directories")
    ap.add_argument("--intersection", action="store_true", help="compare the points two fits share when their point sets differ")
    ap.add_argument("--criterion", choices=["waic", "loo", "logo"], default="waic",
                    help="compare the pointwise elpd of WAIC (default), of PSIS-LOO (summaries written with --loo), or the per-experiment "
                         "elpd of the integrated leave-one-experiment-out (hierarchical summaries written with --leave-experiment-out)")
    a = ap.parse_args(argv)
    if len(a.summaries) < 2:
        raise SystemExit("compare_models needs at least two summaries or directories")
    rows = compare_sources([load_sources(p, a.criterion) for p in a.summaries], a.summaries, a.intersection, a.criterion)
    print(json.dumps({"comparisons": rows}))
    sys.stdout.flush()
    print(table(rows, a.criterion), file=sys.stderr)
    return rows


if __name__ == "__main__":
    main()
