"""The table of faulty C-ABI calls behind tests/test_abi_messages_host.py and tests/golden/make_golden_abi_messages.py (not a test
module): every entry of the nine init / accumulate / reduce families, one row per argument check and a few rows with two faults, which
pin the order of the checks.  All pointers are fake: every row must fail (or, for an accumulate, pass with num_rows = 0) before a launch.

run(lib) -> {case id: [return code, phf_last_error()]} for a library loaded by pyhillfit_amd._lib.load()."""
import ctypes as C

FAKE = 8                     # a pointer that is never dereferenced
BIG = 1 << 40
NEED_LESS_1 = "need - 1"     # replaced by the family's workspace_bytes of the default shape, minus one
INT_MAX = 2 ** 31 - 1


def _pointwise(lib_mod, num_problems=2, stride=5, ln_conc=FAKE):
    return lib_mod.PointwisePoints(num_problems, stride, ln_conc, FAKE, FAKE, FAKE)


def _points(lib_mod, num_pairs=2, stride=5, ln_conc=FAKE):
    return lib_mod.Points(num_pairs, stride, ln_conc, FAKE, FAKE, FAKE, FAKE, FAKE)


def _entries(m):
    """{entry: (workspace_bytes symbol and its arguments of the default shape, [(parameter, default), ...])}; m: pyhillfit_amd._lib"""
    P = C.byref
    pw, sl = _pointwise(m), _points(m)
    tail = [("ws", FAKE), ("wb", BIG), ("stream", None)]
    rows = [("rows", FAKE), ("n", 0)]
    window = [("first", 0), ("N", 100)]
    e = {}
    for fam, extra in (("diagnostics", [("K", 16)]), ("batch_means", []), ("comoments", [])):
        shape = [("Q", 2), ("cols", 3), ("C", 64), ("N", 100)] + extra
        need = ("phf_%s_workspace_bytes" % fam, [v for _, v in shape])
        e["phf_%s_workspace_bytes" % fam] = (need, shape)
        e["phf_%s_init" % fam] = (need, shape + tail)
        e["phf_%s_accumulate" % fam] = (need, rows + [("Q", 2), ("stride", 5), ("C", 64), ("cols", 3)] + window + extra + tail)
        e["phf_%s_reduce" % fam] = (need, shape + tail[:2] + [("out", FAKE), ("stream", None)])
    for fam, extra in (("waic", []), ("psis", [("tpc", 0)]), ("ppc", [])):
        shape = [("Q", 2), ("stride", 5), ("C", 64), ("N", 100)] + extra
        need = ("phf_%s_workspace_bytes" % fam, [v for _, v in shape])
        e["phf_%s_workspace_bytes" % fam] = (need, shape)
        e["phf_%s_init" % fam] = (need, shape + tail)
        stream_words = [("pid", FAKE), ("cid", 0), ("seed", 25)] if fam == "ppc" else []
        call = rows + [("Q", 2), ("stride", 4), ("C", 64)] + window + extra + stream_words + tail
        e["phf_%s_accumulate" % fam] = (need, [("pts", P(pw)), ("lik", 2), ("ne", 0)] + call)
        if fam != "ppc":
            e["phf_%s_accumulate_given" % fam] = (need, [("pts", P(pw))] + [(k, 5 if k == "stride" else v) for k, v in call])
    e["phf_waic_reduce"] = (e["phf_waic_init"][0], [("Q", 2), ("stride", 5), ("C", 64), ("N", 100)] + tail[:2] + [("out", FAKE), ("stream", None)])
    e["phf_ppc_reduce"] = (e["phf_ppc_init"][0], [("Q", 2), ("stride", 5), ("C", 64), ("N", 100)] + tail[:2] + [("out", FAKE), ("stream", None)])
    e["phf_psis_reduce"] = (e["phf_psis_init"][0], [("pts", P(pw)), ("Q", 2), ("C", 64), ("N", 100), ("tpc", 0)] + tail[:2]
                            + [("out", FAKE), ("tail_out", None), ("stream", None)])
    e["phf_psis_tail_length"] = (None, [("C", 64), ("N", 100)])
    e["phf_psis_tail_per_chain"] = (None, [("Q", 2), ("stride", 5), ("C", 64), ("N", 100), ("tpc", 0)])
    qshape = [("Q", 2), ("cols", 3), ("G", 4), ("B", 256)]
    qneed = ("phf_quantiles_workspace_bytes", [v for _, v in qshape])
    e["phf_quantiles_workspace_bytes"] = (qneed, qshape)
    e["phf_quantiles_init"] = (qneed, qshape + tail)
    e["phf_quantiles_accumulate"] = (qneed, rows + [("Q", 2), ("stride", 5), ("C", 64), ("cols", 3), ("G", 4), ("B", 256)] + window + tail)
    e["phf_quantiles_accumulate_curves"] = (qneed, rows + [("Q", 2), ("stride", 5), ("C", 64), ("model", 2), ("lnd", FAKE), ("cols", 3), ("G", 4),
                                                           ("B", 256)] + window + tail)
    e["phf_quantiles_accumulate_hier_curves"] = (qneed, rows + [("Q", 2), ("stride", 5), ("C", 64), ("lnd", FAKE), ("cols", 3), ("D", 2), ("B", 256)]
                                                 + window + [("pid", FAKE), ("cid", 0), ("seed", 25)] + tail)
    probs = (C.c_double * 3)(0.025, 0.5, 0.975)
    e["phf_quantiles_reduce"] = (qneed, qshape + [("probs", C.cast(probs, C.c_void_p)), ("P", 3)] + tail[:2] + [("out", FAKE), ("stream", None)])
    e["_keep"] = (probs, pw, sl)
    sshape = [("Q", 2), ("cols", 3), ("C", 64), ("N", 100), ("B", 256)]
    sneed = ("phf_sensitivity_workspace_bytes", [v for _, v in sshape])
    e["phf_sensitivity_workspace_bytes"] = (sneed, sshape)
    e["phf_sensitivity_init"] = (sneed, sshape + tail)
    e["phf_sensitivity_accumulate"] = (sneed, [("kind", 4), ("sl", None), ("hp", None), ("prior", None), ("pc", 3), ("lc", 4)] + rows
                                       + [("Q", 2), ("stride", 5), ("C", 64), ("cols", 3), ("delta", 0.01), ("B", 256)] + window + tail)
    e["phf_sensitivity_reduce"] = (sneed, sshape + tail[:2] + [("slots", FAKE), ("weights", FAKE), ("columns", FAKE), ("per_chain", None),
                                                               ("stream", None)])
    tshape = [("Q", 2), ("C", 64), ("N", 100)]
    tneed = ("phf_stepping_stone_workspace_bytes", [v for _, v in tshape])
    e["phf_stepping_stone_workspace_bytes"] = (tneed, tshape)
    e["phf_stepping_stone_init"] = (tneed, tshape + tail)
    e["phf_stepping_stone_accumulate"] = (tneed, [("pts", P(sl)), ("model", 2), ("pi", FAKE), ("delta", FAKE)] + rows
                                          + [("Q", 2), ("stride", 4), ("C", 64)] + window + tail)
    e["phf_stepping_stone_reduce"] = (tneed, tshape + tail[:2] + [("out", FAKE), ("stream", None)])
    e["phf_stepping_stone_reduce_joint"] = (tneed, [("P", 1), ("R", 2), ("C", 64), ("N", 100)] + tail[:2]
                                            + [("reduced", FAKE), ("out", FAKE), ("stream", None)])
    return e


# faults shared by the entries that take these parameters: (label, {parameter: value})
SHAPE = [("Q=0", {"Q": 0}), ("C=0", {"C": 0}), ("Q<0", {"Q": -3}), ("N=0", {"N": 0}), ("grid", {"Q": INT_MAX, "C": INT_MAX - 63})]    # C + 63 must not overflow
COLS = [("cols=0", {"cols": 0}), ("N=3", {"N": 3}), ("grid-cols", {"Q": INT_MAX, "cols": 1000})]
WS = [("ws=null", {"ws": None}), ("wb-small", {"wb": NEED_LESS_1}), ("ws=null+wb-small", {"ws": None, "wb": NEED_LESS_1})]
ROWS = [("n>N", {"n": 101}), ("first<0", {"first": -1, "n": 1}), ("n<0", {"n": -1}), ("past-end", {"first": 95, "n": 10}), ("stride-small", {"stride": 1}),
        ("rows=null", {"rows": None}), ("rows=null,n=1", {"rows": None, "n": 1}),
        ("Q=0+n>N", {"Q": 0, "n": 101}), ("n>N+stride-small", {"n": 101, "stride": 1}), ("stride-small+rows=null", {"stride": 1, "rows": None}),
        ("rows=null+wb-small", {"rows": None, "wb": NEED_LESS_1}), ("n>N+wb-small", {"n": 101, "wb": NEED_LESS_1})]
OUT = [("out=null", {"out": None}), ("out=null+wb-small", {"out": None, "wb": NEED_LESS_1})]


def _own(m):
    """faults of single entries: {entry: [(label, overrides)]}"""
    P = C.byref
    keep = []

    def pw(**kw):
        keep.append(_pointwise(m, **kw))
        return P(keep[-1])

    def sl(**kw):
        keep.append(_points(m, **kw))
        return P(keep[-1])

    lik = [("pts=null", {"pts": None}), ("pts-array-null", {"pts": pw(ln_conc=None)}), ("pts-rows", {"pts": pw(num_problems=3)}),
           ("pts-stride=0", {"pts": pw(stride=0)}), ("pts-rows+Q=0", {"pts": pw(num_problems=3), "Q": 0}),
           ("pts=null+n>N", {"pts": None, "n": 101})]
    codes = [("lik=0", {"lik": 0}), ("lik=4", {"lik": 4}), ("lik=5", {"lik": 5}), ("lik=3,ne=0", {"lik": 3, "ne": 0}),
             ("lik=3,ne=2,stride=8", {"lik": 3, "ne": 2, "stride": 8}), ("lik=0+stride-small", {"lik": 0, "stride": 1}), ("C=0+lik=0", {"C": 0, "lik": 0})]
    psis = [("N=1,C=1", {"N": 1, "C": 1}), ("tpc<0", {"tpc": -1}), ("S-too-large", {"N": 1 << 53}), ("M-too-large", {"N": 1 << 40}),
            ("tpc-holds-too-few", {"tpc": 1}), ("grid-k", {"N": 1 << 16, "C": 1 << 16, "tpc": 1 << 16})]    # k x chains = 2^32, M = 196608
    big = pw(num_problems=INT_MAX)
    psis_grid = {False: [("grid-problems", {"Q": INT_MAX}), ("tpc<0+grid-problems", {"Q": INT_MAX, "tpc": -1})],
                 True: [("grid-problems", {"Q": INT_MAX, "pts": big}), ("tpc<0+grid-problems", {"Q": INT_MAX, "pts": big, "tpc": -1}),
                        ("grid-problems+n>N", {"Q": INT_MAX, "pts": big, "n": 101})]}
    own = {e: [] for e in _entries(m) if e != "_keep"}
    for e in own:
        if e.startswith(("phf_waic_accumulate", "phf_psis_accumulate", "phf_ppc_accumulate", "phf_psis_reduce")):
            own[e] += lik
        if e in ("phf_waic_accumulate", "phf_psis_accumulate", "phf_ppc_accumulate"):
            own[e] += codes
        if e.startswith(("phf_waic_accumulate", "phf_ppc_accumulate")):
            own[e] += [("grid-problems", {"Q": INT_MAX, "pts": big}), ("grid-problems+lik=0", {"Q": INT_MAX, "pts": big, "lik": 0})]
        if e.startswith("phf_psis"):
            own[e] += psis + psis_grid["accumulate" in e or "reduce" in e]
        if e.startswith("phf_ppc"):
            own[e] += [("stride-big", {"stride": 513})] if "accumulate" not in e else []
    own["phf_ppc_accumulate"] += [("pid=null", {"pid": None}), ("total-rows-32-bit", {"N": (1 << 32) + 1}), ("pts-stride-big", {"pts": pw(stride=513)}),
                                  ("pts-stride-big+C=0", {"pts": pw(stride=513), "C": 0})]
    for e in own:
        if e.startswith(("phf_diagnostics", "phf_comoments")):
            own[e] += [("N=7", {"N": 7})]
    own["phf_diagnostics_workspace_bytes"] += [("K=0", {"K": 0})]
    own["phf_diagnostics_accumulate"] += [("K=0", {"K": 0}), ("K=0+N=7", {"K": 0, "N": 7})]
    own["phf_comoments_init"] += [("cols-big", {"cols": 1025})]
    own["phf_comoments_accumulate"] += [("cols-big", {"cols": 1025, "stride": 2000}), ("cols-big+N=7", {"cols": 1025, "N": 7})]
    q = [("G<0", {"G": -1}), ("cols=0,G=0", {"cols": 0, "G": 0}), ("B=100", {"B": 100}), ("B=32", {"B": 32}), ("B-big", {"B": 65536}),
         ("slots", {"Q": INT_MAX, "cols": 8})]
    for e in own:
        if e.startswith("phf_quantiles"):
            own[e] += q
    qrows = [("C=0", {"C": 0}), ("stride=0", {"stride": 0}), ("N=0", {"N": 0}), ("flat", {"n": 1 << 26, "C": 64, "N": 1 << 27}),
             ("rows=null,n=1+ws=null", {"rows": None, "n": 1, "ws": None})]
    own["phf_quantiles_accumulate"] += qrows + [("no-columns", {"cols": 0})]
    own["phf_quantiles_accumulate_curves"] += qrows + [("model=3", {"model": 3}), ("no-curve-points", {"G": 0}), ("lnd=null", {"lnd": None}),
                                                       ("model=3+lnd=null", {"model": 3, "lnd": None})]
    own["phf_quantiles_accumulate_hier_curves"] += qrows + [("D=0", {"D": 0}), ("D-big", {"D": (1 << 20) + 1}), ("lnd=null", {"lnd": None}),
                                                            ("pid=null", {"pid": None}), ("stride=3", {"stride": 3}), ("total-rows-32-bit", {"N": (1 << 32) + 1}),
                                                            ("D=0+Q=0", {"D": 0, "Q": 0})]
    own["phf_quantiles_reduce"] += [("P=0", {"P": 0}), ("P=65", {"P": 65}), ("probs=null", {"probs": None}), ("P=0+ws=null", {"P": 0, "ws": None})]
    bad = (C.c_double * 3)(0.025, 1.5, 0.975)
    keep.append(bad)
    own["phf_quantiles_reduce"] += [("prob>1", {"probs": C.cast(bad, C.c_void_p)})]
    s = [("cols=0", {"cols": 0}), ("B=100", {"B": 100}), ("B-big", {"B": 8192}), ("draws", {"N": 1 << 30, "C": 64}), ("grid-draw", {"Q": 1 << 24, "C": 1 << 20, "N": 1})]
    for e in own:
        if e.startswith("phf_sensitivity"):
            own[e] += s
    own["phf_sensitivity_accumulate"] += [
        ("kind=0", {"kind": 0}), ("kind=5", {"kind": 5}), ("delta=0", {"delta": 0.0}), ("delta-big", {"delta": 0.3}), ("stride=0", {"stride": 0}),
        ("given-column", {"pc": 5}), ("given-column<0", {"lc": -1}), ("kind=1,sl=null", {"kind": 1}), ("kind=1,pairs", {"kind": 1, "sl": sl(num_pairs=3)}),
        ("kind=2,stride-small", {"kind": 2, "sl": sl(), "cols": 1, "stride": 2}), ("kind=3,null", {"kind": 3}),
        ("kind=0+delta=0", {"kind": 0, "delta": 0.0}), ("delta=0+stride-small", {"delta": 0.0, "stride": 1}), ("ws=null+rows=null,n=1", {"ws": None, "rows": None, "n": 1})]
    own["phf_sensitivity_reduce"] += [("slots=null", {"slots": None}), ("weights=null", {"weights": None}), ("columns=null", {"columns": None}),
                                      ("ws=null+slots=null", {"ws": None, "slots": None})]
    own["phf_stepping_stone_accumulate"] += [
        ("pts=null", {"pts": None}), ("pts-empty", {"pts": sl(num_pairs=0)}), ("pts-array-null", {"pts": sl(ln_conc=None)}), ("model=3", {"model": 3}),
        ("model=1,stride=1", {"model": 1, "stride": 1}), ("pi=null", {"pi": None}), ("delta=null", {"delta": None}), ("pts=null+model=3", {"pts": None, "model": 3}),
        ("model=3+n>N", {"model": 3, "n": 101})]
    own["phf_stepping_stone_reduce_joint"] += [("P=0", {"P": 0}), ("R=0", {"R": 0}), ("P*R", {"P": 1 << 20, "R": 1 << 20}), ("reduced=null", {"reduced": None}),
                                               ("P=0+C=0", {"P": 0, "C": 0})]
    own["_keep"] = keep
    return own


SIZES = ("_workspace_bytes", "_tail_length", "_tail_per_chain")      # entries that return a size, 0 on a fault


def cases(m):
    """[(case id, entry, workspace_bytes call of the default shape, parameter names, arguments)] for pyhillfit_amd._lib `m`; the ctypes
    objects the arguments point into are kept alive in m"""
    entries, own = _entries(m), _own(m)
    m._abi_message_cases_keep = (entries.pop("_keep"), own.pop("_keep"))
    out = []
    for entry, (need, params) in entries.items():
        names = [k for k, _ in params]
        half_chains = entry.startswith(("phf_diagnostics", "phf_batch_means", "phf_comoments"))
        for label, over in SHAPE + (COLS if half_chains else []) + WS + (ROWS if "rows" in names else []) + OUT + own[entry]:
            if not set(over) <= set(names) or (entry.endswith("_given") and "stride-small" in label):
                continue                                   # the entry has no such parameter (given: the stride is the points')
            if label == "grid" and (entry.startswith(("phf_psis", "phf_quantiles", "phf_sensitivity")) or "pts" in names):
                continue                                   # an earlier check takes these values: such entries have grid rows of their own
            out.append(("%s[%s]" % (entry, label), entry, need, names, [over.get(k, v) for k, v in params]))
    return out


def run(lib, m):
    """{case id: [return code, message]}; the message is "" where the call succeeded (an accumulate of no rows)"""
    res = {}
    for cid, entry, need, names, args in cases(m):
        if NEED_LESS_1 in args:
            size = getattr(lib, need[0])(*need[1])
            assert size > 1, (cid, lib.phf_last_error())
            args = [size - 1 if a is NEED_LESS_1 else a for a in args]
        rc = int(getattr(lib, entry)(*[C.c_size_t(a) if k == "wb" else a for k, a in zip(names, args)]))
        failed = rc == 0 if entry.endswith(SIZES) else rc != 0
        assert rc == -1 or entry.endswith(SIZES) or (rc == 0 and "n" in names), "%s got past its checks with fake pointers" % cid
        res[cid] = [rc, lib.phf_last_error().decode() if failed else ""]
    return res
