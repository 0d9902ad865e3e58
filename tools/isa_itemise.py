#!/usr/bin/env python3
"""Itemised static instruction mix of the innermost loops (the MH iteration bodies: one basic-block loop per entry-count shape) of one
kernel in a hipcc -S listing — what the vector-ALU slots of an iteration are spent on BESIDES fp64 arithmetic.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math -S --cuda-device-only -o sl.s pyhillfit_amd/csrc/phf_single_level.hip
    python tools/isa_itemise.py sl.s mh_advance_kernelILi2ELb0ELi2E            (produced profiles/r05/c3_valu_itemised.txt)

    python tools/isa_itemise.py sl.s mh_advance_kernelILi2ELb0ELi2E crumb [reference.s]
                                                                               ("crumb": weight the bodies by the Crumb set's pairs; reference.s:
                                                                               an earlier listing that names the bodies where the LDS reads cannot)

    python tools/isa_itemise.py sl.s mh_advance_kernelILi2ELb0ELi2E uniform [reference.s]
                                                                               (listing only, "round 11": per body the vector instructions whose
                                                                               result is the same in all lanes or a constant — uniform_report)

A loop = a backward branch whose span holds no other backward branch; classes by opcode (and, for Philox, by its constants).  A region
that a forward s_cbranch_vccz skips and that reads LDS (the accept test's logarithm) or holds six or more selects (the guarded Cholesky
factor of the steady bodies) is a rare path and is listed apart, not counted."""
import collections
import re
import sys

CLASSES = [
    ("fp64 arithmetic (fma, mul, add: what the PMC's flop counters see)", r"v_(fma|fmac|mul|add)_f64"),
    ("fp64 estimates (v_rcp_f64, v_rsq_f64: quarter rate)", r"v_(rcp|rsq|sqrt)_f64"),
    ("fp64 other: min / max (clamps)", r"v_(min|max)_f64"),
    ("fp64 other: compares", r"v_cmp\w*_f64"),
    ("fp64 other: ldexp, conversions", r"v_(ldexp_f64|cvt_f64_\w+|cvt_\w+_f64|frexp\w*_f64|trunc_f64|rndne_f64)"),
    ("Philox: 32 x 32 -> 64 multiplies", r"v_(mad_u64_u32|mul_hi_u32|mul_lo_u32)"),
    ("Philox / bit logic: 3-input xor, xor, and-or, bfi", r"v_(bitop3_b32|xor_b32|and_or_b32|bfi_b32|or3_b32|xad_u32)"),
    ("selects (v_cndmask_b32: two per double)", r"v_cndmask_b32"),
    ("moves (v_mov_b32 / _b64, v_accvgpr, lane ops)", r"v_(mov_b32|mov_b64|accvgpr_\w+|readlane\w*|writelane\w*|readfirstlane\w*|pk_mov_b32)"),
    ("integer / address arithmetic (table indices, exponent fields)", r"v_(and_b32|or_b32|not_b32|lshl\w*|lshr\w*|ashr\w*|add\w*_u32|add_co\w*|addc\w*|sub\w*_u32|subrev\w*|mul_u32_u24|mad_u32_u24|min_u32|max_u32|min_i32|max_i32|lshl_add_u64|bfe_\w+|cvt_\w*32\w*|cmp\w*_[ui]32|cmp\w*_[ui]64|alignbit\w*|perm_b32|add3_u32|lshl_or_b32|med3\w*)"),
]
THREE_INPUT = "bit logic: three-input and-or / bit select (mantissa re-bias, sign transfer; not Philox)"


# Issue cost in cycles per wavefront instruction with two or more wavefronts per SIMD, measured (tools/isa_instr_cost.py,
# profiles/r05/gfx950_instruction_costs.txt): quarter-rate estimates 16; the simple 32-bit VOP1 / VOP2 operations 2 — when encoded _e32 and
# without a scalar-register operand (with one they measure 4) —; everything else, every VOP3 encoding included, 4.
FAST_E32 = r"v_(mov_b32|add_u32|sub_u32|subrev_u32|and_b32|or_b32|xor_b32|not_b32|lshrrev_b32|ashrrev_i32|accvgpr_read_b32|accvgpr_write_b32|fma_f32|add_f32|mul_f32)_e32"


def issue_cycles(line):
    op = line.split()[0]
    if re.match(r"v_(rcp|rsq|sqrt)_f64", op):
        return 16
    if re.match(r"v_(exp|log|rcp|rsq|sqrt|sin|cos)_f32", op):
        return 8                      # fp32 transcendental (the accept test's v_exp_f32): twice a plain operation — not measured here
    if op.startswith("v_accvgpr") or re.fullmatch(FAST_E32, op):
        operands = line.split(None, 1)[1] if " " in line else ""
        if not re.search(r"\bs\d+|\bs\[|\bvcc|\bexec|\bm0", operands):
            return 2
    return 4


# pairs of the Crumb set per (uncensored entries, censored entries, runs the shared-denominator body of its shape) after merging
# replicates (pyhillfit_amd.doseresponse.pack_single_level; the masks the kernel offers: phf_single_level.hip, run_block).  A listing
# without shared-denominator bodies counts a shape's sharing pairs on its plain body.
SHAPE_WEIGHTS = [((4, 1, 1), 45), ((4, 0, 0), 41), ((4, 2, 1), 25), ((4, 4, 1), 22), ((4, 3, 1), 13), ((3, 4, 1), 9), ((3, 4, 0), 2),
                 ((3, 3, 1), 6), ((3, 3, 0), 1), ((2, 4, 1), 6), ((2, 4, 0), 3), ((1, 4, 1), 3), ((1, 4, 0), 3), ((2, 3, 1), 3),
                 ((2, 3, 0), 2), ((2, 2, 1), 2), ((2, 2, 0), 3), ((3, 2, 1), 4), ((3, 1, 0), 3), ((1, 3, 0), 3), ((2, 1, 1), 3),
                 ((2, 0, 0), 1), ((0, 4, 0), 3), ((0, 2, 0), 1), ((5, 0, 0), 2), ((5, 1, 0), 1)]


def _vgprs(operand):
    m = re.fullmatch(r"v(\d+)", operand)
    if m:
        return range(int(m.group(1)), int(m.group(1)) + 1)
    m = re.fullmatch(r"v\[(\d+):(\d+)\]", operand)
    return range(int(m.group(1)), int(m.group(2)) + 1) if m else range(0)


def distinct_lds_bytes(body):
    """how many different LDS bytes the ds_read instructions of a body fetch: per (address register, how often it has been written so far)
    the union of the byte ranges read — a table word read again (a reload instead of a live register), or an entry fetched as
    ds_read2_b64 pairs instead of 16-byte reads, counts once"""
    version = collections.Counter()
    seen = collections.defaultdict(set)
    for l in body:
        parts = l.replace(",", " ").split()
        if l.startswith("ds_read"):
            kind = parts[0][len("ds_read"):]
            key = (parts[2], version[parts[2]])
            if kind.startswith("2"):                                 # ds_read2[st64]_b32 / _b64: two elements at offset0, offset1 (in elements)
                size = 8 if kind.endswith("b64") else 4
                step = size * (64 if "st64" in kind else 1)
                for name in ("offset0", "offset1"):
                    m = re.search(name + r":(\d+)", l)
                    start = (int(m.group(1)) if m else 0) * step
                    seen[key].update(range(start, start + size))
            else:
                size = {"_b32": 4, "_b64": 8, "_b96": 12, "_b128": 16}[kind]
                m = re.search(r"offset:(\d+)", l)
                start = int(m.group(1)) if m else 0
                seen[key].update(range(start, start + size))
        if not re.match(r"(ds_write|global_store|buffer_store|scratch_store|s_|v_cmp)", l) and len(parts) > 1:
            for r in _vgprs(parts[1]):
                version["v%d" % r] += 1
    return sum(len(v) for v in seen.values())


def shape_by_lds(body):
    nbytes = distinct_lds_bytes(body)
    shared = int(any(l.startswith("ds_write") for l in body))
    return next(((ko, kc, shared) for ko in range(0, 6) for kc in range(0, 5) if 200 + 8 * ko + 88 * kc == nbytes), None)


def shape_key(body):
    """what a body keeps from build to build: its fp64 fma / mul / add, estimates and ldexp (the twin fixes that sequence) and whether it
    writes LDS slots"""
    return tuple(sum(1 for l in body if re.match(p, l)) for p in (r"v_(fma|fmac|mul|add)_f64", r"v_(rcp|rsq)_f64", r"v_ldexp_f64")) + (
        int(any(l.startswith("ds_write") for l in body)),)


def reference_shapes(path, want):
    """shape_key -> shape of the iteration bodies of an earlier listing whose LDS reads still name every shape (rounds 5 to 9): for
    listings whose reads no longer do (fourth argument)"""
    src = open(path).read().split("\n")
    starts = [i for i, l in enumerate(src) if re.match(r"_Z\w+:", l)]
    found = {}
    for si, s0 in enumerate(starts):
        if want not in src[s0].split(":", 1)[0]:
            continue
        labels, ins = {}, []
        for l in src[s0 + 1:starts[si + 1] if si + 1 < len(starts) else len(src)]:
            l = l.strip()
            m = re.match(r"(\.LBB\d+_\d+):", l)
            if m:
                labels[m.group(1)] = len(ins)
            elif l.startswith(".Lfunc_end"):
                break
            elif l and not l.startswith(";") and not l.startswith("."):
                ins.append(l)
        back = [(labels[m.group(1)], i) for i, l in enumerate(ins) for m in [re.match(r"s_cbranch_\w+ (\.LBB\d+_\d+)", l)]
                if m and m.group(1) in labels and labels[m.group(1)] <= i]
        for a, b in back:
            if b - a > 300 and not any(a <= c and d <= b and (c, d) != (a, b) for c, d in back):
                body = ins[a:b + 1]
                found.setdefault(shape_key(body), set()).add(shape_by_lds(body))
    return {k: next(iter(v)) for k, v in found.items() if len(v) == 1 and None not in v}


def rare_regions(ins, labels, a, b):
    """instruction indices of body [a..b] that a forward s_cbranch_vccz skips and that read LDS or hold six or more selects (main)"""
    skip = set()
    for i in range(a, b):
        m = re.match(r"s_cbranch_vccz (\.LBB\d+_\d+)", ins[i])
        if m and m.group(1) in labels and i < labels[m.group(1)] <= b:
            region = range(i + 1, labels[m.group(1)])
            if any(ins[j].startswith("ds_read") for j in region) or sum(ins[j].startswith("v_cndmask") for j in region) >= 6:
                skip.update(region)
    return skip


def _operands(line):
    parts = line.split(None, 1)
    return [o.strip() for o in parts[1].split(",")] if len(parts) > 1 else []


def _vector_registers(operand):
    """the VGPRs and AGPRs an operand names, as ("v" | "a", number)"""
    regs = set()
    for kind, one, lo, hi in re.findall(r"\b([va])(?:(\d+)\b|\[(\d+):(\d+)\])", operand):
        regs.update((kind, r) for r in (range(int(one), int(one) + 1) if one else range(int(lo), int(hi) + 1)))
    return regs


def _destinations(line):
    """how many leading operands an instruction WRITES: none for stores, LDS writes, scalar instructions and the e32 compares (vcc is
    implied there but written first in the text, and names no vector register anyway); two for the carry-out and 64-bit multiply-add forms"""
    op = line.split()[0]
    if re.match(r"(ds_write|global_store|buffer_store|scratch_store|global_atomic|s_|v_cmpx)", op):
        return 0
    if re.match(r"v_(mad_[ui]64_[ui]32|add_co|sub_co|subrev_co|addc_co|subb_co|subbrev_co|div_scale)", op):
        return 2
    return 1


def uniform_report(ins, labels, inner, name_of):
    """Per iteration body: the VALU instructions none of whose vector-register sources is written anywhere inside the loop (rare paths
    included) — every such source is loop invariant, so the result can vary from iteration to iteration only through scalar registers,
    which hold one value for the whole wavefront, or not at all (a constant).  An instruction that accumulates into its destination
    (v_fmac, v_mac, v_writelane) reads it.  These are candidates, not verdicts: a loop-invariant VGPR may still differ from lane to lane
    (then the result is not wave-uniform and the instruction is simply hoistable or needed), and a move under the accept mask writes a
    constant into SOME lanes.  One step further, marked "derived": walking the body in order, a register whose current value was written
    from scalar registers, constants and such registers alone — by a vector instruction, or by a global_load at such an address (the
    gamma table's entry) — holds a wave-uniform value, and counts as no varying source for the instructions behind it, up to its next
    write by anything else.  (A loop-invariant VGPR passes nothing on — it may hold the chain's number — unless the nearest instruction
    in front of the loop that writes it is a move of a constant or of a scalar register: the zero offset of the gamma load.)  What is
    decided about each is in DESIGN.md section 3, "round 11"."""
    for a, b in sorted(inner, key=lambda ab: (sum(1 for l in ins[ab[0]:ab[1] + 1] if l.startswith("v_")), ab)):
        written = set()
        for l in ins[a:b + 1]:
            ops = _operands(l)
            for o in ops[:_destinations(l)]:
                written |= _vector_registers(o)
        rare = rare_regions(ins, labels, a, b)
        found = []
        derived = set()                                        # registers whose current value comes from SGPRs, constants and such registers alone
        pending = {r for l in ins[a:b + 1] for o in _operands(l)[_destinations(l):] for r in _vector_registers(o)} - written
        for i in range(a - 1, max(a - 20000, -1), -1):          # loop-invariant sources: what set them in front of the loop
            if not pending:
                break
            ops = _operands(ins[i])
            hit = pending & (set().union(*[_vector_registers(o) for o in ops[:_destinations(ins[i])]]) if _destinations(ins[i]) else set())
            if hit:
                pending -= hit
                if re.match(r"v_mov_b(32|64)", ins[i]) and not _vector_registers(ops[1]):
                    derived |= hit
        for i in range(a, b + 1):
            l = ins[i]
            ops = _operands(l)
            nd = _destinations(l)
            dst = set().union(*[_vector_registers(o) for o in ops[:nd]]) if nd else set()
            sources = ops[nd:]
            if re.match(r"v_(fmac|mac|pk_fmac|writelane)", l):
                sources = sources + ops[:1]
            vsrc = set().union(*[_vector_registers(o) for o in sources]) if sources else set()
            if (l.startswith("v_") or l.startswith("global_load")) and not (vsrc & written) - derived:
                if l.startswith("v_"):
                    scalar = any(re.search(r"\b(s\d+|s\[|vcc|exec|m0|ttmp)", o) for o in sources)
                    kind = ("invariant VGPRs + SGPR" if vsrc and scalar else "invariant VGPRs only" if vsrc else "SGPR only" if scalar else "constant")
                    found.append((i, kind + (", derived" if vsrc & derived else ""), l))
            if (l.startswith("v_") or l.startswith("global_load")) and vsrc <= derived:
                derived |= dst
            else:
                derived -= dst
        counted = [f for f in found if f[0] not in rare]
        shape = name_of(ins[a:b + 1])
        print("\n  body [%d..%d]%s: %d candidates, %d issue cycles (another %d on a rare path)" % (
            a, b, "" if shape is None else " = %d uncensored + %d censored entries%s" % (shape[0], shape[1], ", shared denominators" if shape[2] else ""),
            len(counted), sum(issue_cycles(l) for _, _, l in counted), len(found) - len(counted)))
        for i, kind, l in found:
            print("     +%-4d %-33s %s%s" % (i - a, kind, " ".join(l.split()), "   (rare path)" if i in rare else ""))


def main():
    if len(sys.argv) > 3 and sys.argv[3] == "uniform":
        return main_uniform()
    src = open(sys.argv[1]).read().split("\n")
    want = sys.argv[2]
    reference = reference_shapes(sys.argv[4], want) if len(sys.argv) > 4 else {}
    starts = [i for i, l in enumerate(src) if re.match(r"_Z\w+:", l)]
    for si, s0 in enumerate(starts):
        name = src[s0].split(":", 1)[0]
        if want not in name:
            continue
        end = starts[si + 1] if si + 1 < len(starts) else len(src)
        labels, ins = {}, []
        for l in src[s0 + 1:end]:
            l = l.strip()
            m = re.match(r"(\.LBB\d+_\d+):", l)
            if m:
                labels[m.group(1)] = len(ins)
                continue
            if l.startswith(".Lfunc_end"):
                break
            if not l or l.startswith(";") or l.startswith("."):
                continue
            ins.append(l)
        back = []
        for i, l in enumerate(ins):
            # conditional branches only: an out-of-line block behind the loop (the sample store, the temperature != 1 block of the
            # steady bodies) returns into the body with an s_branch, which is no loop
            m = re.match(r"s_cbranch_\w+ (\.LBB\d+_\d+)", l)
            if m:
                lab = m.group(1)
                if lab in labels and labels[lab] <= i:
                    back.append((labels[lab], i))
        inner = [(a, b) for a, b in back if not any(a <= c and d <= b and (c, d) != (a, b) for c, d in back)]
        inner = [(a, b) for a, b in inner if b - a > 300]                  # the iteration bodies (the point loops of the generic body are short)
        print("%s: %d instructions, %d iteration bodies" % (name, len(ins), len(inner)))
        rows = []
        rare = {}
        for a, b in inner:
            # rare paths: regions a forward wave-uniform branch skips that read LDS — the accept test's logarithm (phf_mh_accept_u32 runs it
            # only when some lane is next to its threshold, at most one iteration of a wavefront in 128) — or that hold six or more selects —
            # the guarded Cholesky factor of the steady bodies (chol_packed_steady: only when some lane has a non-positive pivot):
            # listed apart, not counted below
            skip = set()
            for i in range(a, b):
                m = re.match(r"s_cbranch_vccz (\.LBB\d+_\d+)", ins[i])
                if m and m.group(1) in labels and i < labels[m.group(1)] <= b:
                    region = range(i + 1, labels[m.group(1)])
                    if any(ins[j].startswith("ds_read") for j in region) or sum(ins[j].startswith("v_cndmask") for j in region) >= 6:
                        skip.update(region)
            rare[a] = sorted(skip)
            body = [l for i, l in enumerate(ins[a:b + 1], a) if i not in skip]
            c = collections.Counter()
            for l in body:
                op = l.split()[0]
                if not op.startswith("v_"):
                    c["(not VALU) " + ("s_nop" if op == "s_nop" else "scalar" if op.startswith("s_") else "LDS" if op.startswith("ds_") else
                                       "scratch" if op.startswith("scratch_") else "global memory" if op.startswith("global_") or op.startswith("buffer_") else op)] += 1
                    continue
                if op.startswith("v_bitop3_b32") and "bitop3:0x96" not in l:
                    c[THREE_INPUT] += 1                               # (Philox's is the three-input xor, table 0x96)
                    continue
                for cname, pat in CLASSES:
                    if re.fullmatch(pat + r"(_e32|_e64|_dpp|_sdwa)?", op):
                        c[cname] += 1
                        break
                else:
                    c["other VALU: " + op] += 1
            valu = sum(v for k_, v in c.items() if not k_.startswith("(not VALU)"))
            fp = sum(1 for l in body if re.match(r"v_(fma|fmac|mul|add)_f64", l.split()[0]))
            cyc = collections.Counter()
            for l in body:
                if l.startswith("v_"):
                    cyc["fp64 fma / mul / add" if re.match(r"v_(fma|fmac|mul|add)_f64", l) else "quarter-rate estimates" if issue_cycles(l) == 16 else
                        "2-cycle 32-bit operations" if issue_cycles(l) == 2 else "other 4-cycle instructions"] += issue_cycles(l)
            c["(issue cycles)"] = cyc
            rows.append((valu, fp, a, b, c))
        # which entry-count shape a body is (single-level kernels): LDS reads = 13 + uncensored entries + 6 x censored entries
        # (one 2^(j/64) read per entry; five 16-byte reads of the log Phi table per censored entry; 13 for the draws and the logarithms;
        # a censored entry that shares its Hill denominator reads it from its LDS slot instead of the 2^(j/64) table), and LDS writes
        # (the uncensored entries' denominators to their slots) only in the shared-denominator bodies
        # Counted in BYTES, each different byte once (distinct_lds_bytes): since round 10 the compiler reads some table words again where it
        # used to keep them in registers, and fetches some entries as ds_read2_b64 pairs, so the number of read instructions no longer tells.
        # 12 16-byte reads and one word for the draws and logarithms, one word per entry, 80 bytes of log Phi table per censored entry.
        # Where even that fails (a table word read again through another address register), a reference listing given as fourth argument
        # names the body: the one of its bodies with the same fp64 arithmetic count and the same use of the LDS slots.
        shapes = {}
        for valu, fp, a, b, c in rows:
            shapes[a] = reference.get(shape_key(ins[a:b + 1])) if reference else shape_by_lds(ins[a:b + 1])
        weights = {}
        if len(sys.argv) > 3 and sys.argv[3] == "crumb":
            have = set(shapes.values())
            for (ko, kc, sh), n in SHAPE_WEIGHTS:
                key = (ko, kc, sh) if (ko, kc, sh) in have else (ko, kc, 0)
                weights[key] = weights.get(key, 0) + n
        averages = [("", lambda s_: True, {}, {}, [0]),
                    (" of the shapes 1..4 uncensored x 0..4 censored", lambda s_: 1 <= s_[0] <= 4, {}, {}, [0])]
        for valu, fp, a, b, c in sorted(rows, key=lambda r: r[:4]):
            cyc = c.pop("(issue cycles)")
            shape = shapes[a]
            w = weights.get(shape, 0)
            print("\n  body [%d..%d]%s: %d instructions, %d VALU of which %d fp64 fma / mul / add" % (
                a, b, "" if shape is None else " = %d uncensored + %d censored entries%s (%d of the 210 Crumb pairs)" % (
                    shape[0], shape[1], ", shared denominators" if shape[2] else "", w), b - a + 1, valu, fp))
            for k_, v in sorted(c.items(), key=lambda kv: (kv[0].startswith("(not VALU)"), -kv[1])):
                print("     %5d  %s" % (v, k_))
            print("     issue cycles of the vector pipe per wavefront: %d = %s" % (sum(cyc.values()), ", ".join("%d %s" % (v, k_) for k_, v in cyc.most_common())))
            if rare[a]:
                print("     not counted above: a rare path of %d instructions, %d VALU" % (len(rare[a]), sum(1 for i in rare[a] if ins[i].startswith("v_"))))
            for _, keep, tot, cyc_tot, wsum in averages:
                if shape is None or not keep(shape):
                    continue
                for k_, v in c.items():
                    tot[k_] = tot.get(k_, 0) + v * w
                for k_, v in cyc.items():
                    cyc_tot[k_] = cyc_tot.get(k_, 0) + v * w
                wsum[0] += w
        for what, _, tot, cyc_tot, wsum in averages:
            wsum = wsum[0]
            if not wsum:
                continue
            print("\n  AVERAGE over the %d Crumb pairs%s whose shape has a straight-line body (weights = pairs per body):" % (wsum, what))
            valu = sum(v for k_, v in tot.items() if not k_.startswith("(not VALU)")) / wsum
            print("     %7.1f  VALU in all" % valu)
            for k_, v in sorted(tot.items(), key=lambda kv: (kv[0].startswith("(not VALU)"), -kv[1])):
                print("     %7.1f  %s" % (v / wsum, k_))
            print("     issue cycles of the vector pipe per wavefront and iteration (measured cost per instruction: tools/isa_instr_cost.py): %.0f" % (sum(cyc_tot.values()) / wsum))
            for k_, v in sorted(cyc_tot.items(), key=lambda kv: -kv[1]):
                print("     %7.0f  %s" % (v / wsum, k_))


def main_uniform():
    src = open(sys.argv[1]).read().split("\n")
    want = sys.argv[2]
    reference = reference_shapes(sys.argv[4], want) if len(sys.argv) > 4 else {}
    starts = [i for i, l in enumerate(src) if re.match(r"_Z\w+:", l)]
    for si, s0 in enumerate(starts):
        name = src[s0].split(":", 1)[0]
        if want not in name:
            continue
        labels, ins = {}, []
        for l in src[s0 + 1:starts[si + 1] if si + 1 < len(starts) else len(src)]:
            l = l.strip()
            m = re.match(r"(\.LBB\d+_\d+):", l)
            if m:
                labels[m.group(1)] = len(ins)
            elif l.startswith(".Lfunc_end"):
                break
            elif l and not l.startswith(";") and not l.startswith("."):
                ins.append(l)
        back = [(labels[m.group(1)], i) for i, l in enumerate(ins) for m in [re.match(r"s_cbranch_\w+ (\.LBB\d+_\d+)", l)]
                if m and m.group(1) in labels and labels[m.group(1)] <= i]
        inner = [(a, b) for a, b in back if b - a > 300 and not any(a <= c and d <= b and (c, d) != (a, b) for c, d in back)]
        print("%s: %d instructions, %d iteration bodies; wave-uniform / constant candidates per body" % (name, len(ins), len(inner)))
        uniform_report(ins, labels, inner, (lambda body: reference.get(shape_key(body))) if reference else shape_by_lds)


if __name__ == "__main__":
    main()
