"""Instruction counts of a kernel's basic blocks in the gfx950 ISA, compiled on the host (no GPU).

    python tools/isa_rows.py                       # k_factor7<60, false>: compile gadfly_hip.hip and count
    python tools/isa_rows.py --asm out.s           # count an existing `hipcc --cuda-device-only -S` listing
    python tools/isa_rows.py --kernel k_factor7 --rows 40 --rowstore
    python tools/isa_rows.py --kernel k_factorw --rows 44 --sample   # the sampling instance (gf_sample_fused)
    python tools/isa_rows.py --steady              # k_factor7<60, false, false, true>: its full row loop, AND
                                                   # k_steady_tail<60>, k_steady_finish<60>: the block loop, per 64-row
                                                   # block and per row; k_steady_finish's full block by phase
                                                   # (z = u + Q s, the state update, the join) with its dependent chains,
                                                   # without and with GF_SWEEP_AXIS_PROVEN (k_steady_finish<60, proven>)
    python tools/isa_rows.py --asm out.s --rank1   # k_steady_rank1: every block of its row loop
    python tools/isa_rows.py --asm out.s --compare parent.s    # which kernels' instructions or descriptors (.amdhsa_*:
                                                   # registers, LDS, scratch) differ between two listings

Prints every basic block of the row loop (the innermost range closed by a backward branch around the block with the
most FP64 FMAs: the sweep's update and mat-vec) with its vector (VALU), LDS, scalar and branch instruction counts.
Blocks that hold an exponential or a sincos (fm_exp / fm_sincos end in v_ldexp_f64) are marked `exp`: the reset
row's decay and the generator's anchors.  VALU counts every v_* opcode
(v_readlane / v_readfirstlane / v_permlane* included, as SQ_INSTS_VALU counts them); LDS counts ds_*, `spill`
scratch_* (register spills), `mov64` 64-bit register copies, `movb32` 32-bit moves.  Matrix instructions (v_mfma_*) are
a class of their own, `MFMA`, and not in VALU: they issue to the matrix pipe.  k_steady_finish forms u = H y in a group
phase in front of every 16 blocks (the blocks that hold its MFMAs, outside the block loop): reported per group and as
its share per block.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "gadfly_amd", "csrc", "gadfly_hip.hip")


def compile_asm(out):
    cmd = ["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-o", out, SRC]
    subprocess.check_call(cmd, stderr=subprocess.DEVNULL)


def kernel_tag(kernel, rows, rowstore, sample, steady=False, proven=False):
    # mangled: ..._19k_factor7ILi60ELb0ELb0ELb0EEEv...  (template <int ROWS, bool ROWSTORE, bool SAMPLE, bool STEADY>); k_factorw has a
    # second integer (its sweep waves) and k_factor3 / k_factorw no ROWSTORE.  The whole argument list is matched.
    mid = r"Li\d+E" if kernel == "k_factorw" else (f"Lb{int(rowstore)}E" if rowstore is not None else "")
    smp = f"Lb{int(sample)}E" if kernel in ("k_factor3", "k_factor7", "k_factorw") else ""
    if kernel == "k_factor7":
        smp += f"Lb{int(steady)}E"
    if kernel == "k_steady_finish":             # template <int ROWS, bool PROVEN> (GF_SWEEP_AXIS_PROVEN)
        smp += f"Lb{int(proven)}E"
    return re.compile(f"{len(kernel)}{kernel}ILi{rows}E{mid}{smp}E")


def kernel_body(lines, kernel, rows, rowstore, sample=False, steady=False, proven=False):
    tag = kernel_tag(kernel, rows, rowstore, sample, steady, proven)
    start = None
    for i, ln in enumerate(lines):
        if start is None and re.match(r"^_Z\S+:", ln) and tag.search(ln.split(":")[0]):
            start = i
        elif start is not None and ln.startswith(".Lfunc_end"):
            return lines[start:i]
    raise SystemExit(f"kernel {kernel}<{rows}> not found in the listing")


def blocks(body):
    """Basic blocks in listing order: name, instruction opcodes, branch targets."""
    out, cur = [], {"name": "entry", "ins": [], "targets": []}
    out.append(cur)
    for ln in body:
        s = ln.strip()
        m = re.match(r"^(\.LBB\d+_\d+|; %bb\.\d+):?", s) if not ln.startswith("\t") else None
        if m:
            cur = {"name": m.group(1).lstrip("; "), "ins": [], "targets": []}
            out.append(cur)
            continue
        if not s or s.startswith(";") or s.startswith("."):
            continue
        op = s.split()[0]
        cur["ins"].append(op)
        if op.startswith("s_cbranch") or op == "s_branch":
            cur["targets"].append(s.split()[1])
    return out


def row_loop(bl, reg):
    """Smallest [header, latch] range of blocks closed by a backward branch that contains block `reg`."""
    idx = {b["name"]: i for i, b in enumerate(bl)}
    best = None
    for j, b in enumerate(bl):
        for tgt in b["targets"]:
            i = idx.get(tgt)
            if i is not None and i <= reg <= j and (best is None or j - i < best[1] - best[0]):
                best = (i, j)
    return best


def counts(ins):
    c = {"valu": 0, "fma": 0, "lds": 0, "salu": 0, "mov64": 0, "movb32": 0, "ldexp": 0, "branch": 0, "scratch": 0,
         "mfma": 0, "gload": 0}
    for op in ins:
        if op.startswith("v_mfma"):
            c["mfma"] += 1
        elif op.startswith("global_load"):
            c["gload"] += 1
        elif op.startswith("v_"):
            c["valu"] += 1
            c["fma"] += op.startswith(("v_fma_f64", "v_fmac_f64"))
            c["mov64"] += op in ("v_mov_b64", "v_mov_b64_e32", "v_pk_mov_b32", "v_lshl_add_u64")
            c["movb32"] += op.startswith("v_mov_b32")
            c["ldexp"] += op.startswith("v_ldexp_f64")
        elif op.startswith("ds_"):
            c["lds"] += 1
        elif op.startswith("scratch_"):
            c["scratch"] += 1
        elif op.startswith("s_cbranch") or op == "s_branch":
            c["branch"] += 1
        elif op.startswith("s_"):
            c["salu"] += 1
    return c


def steady_tail(lines, rows, kernel="k_steady_tail", proven=False):
    """k_steady_tail<rows> / k_steady_finish<rows>: the block loop (the smallest loop around the block with the most FMAs: p and H p) and
    the loops inside it (the s update, two rows per step, unrolled).  Instructions per 64-row block = the block loop's
    own instructions + each inner loop's body times its trips for 64 rows."""
    bl = blocks(kernel_body(lines, kernel, rows, None, proven=proven))
    tag = kernel_tag(kernel, rows, None, False, proven=proven)
    vgpr = next((ln.split(",")[-1].strip() for ln in lines if ".num_vgpr," in ln and tag.search(ln)), "?")
    total = counts([op for b in bl for op in b["ins"]])
    print(f"{kernel}<{rows}{', proven' if proven else ''}>: {len(bl)} blocks, {total['valu']} VALU, {total['lds']} LDS, "
          f"{total['scratch']} scratch (spill) in all; {vgpr} VGPRs")
    reg = max(range(len(bl)), key=lambda i: counts(bl[i]["ins"])["fma"])
    i0, i1 = row_loop(bl, reg)
    idx = {b["name"]: i for i, b in enumerate(bl)}
    inner = sorted({(idx[t], j) for j in range(i0, i1 + 1) for t in bl[j]["targets"]
                    if t in idx and i0 <= idx[t] <= j and not (idx[t] <= reg <= j)})
    inner = [r for r in inner if not any(o != r and o[0] <= r[0] and r[1] <= o[1] for o in inner)]
    keys = ("valu", "lds", "salu", "branch")
    dyn = dict.fromkeys(keys, 0.0)
    in_inner = set()
    print(f"block loop: blocks {bl[i0]['name']} .. {bl[i1]['name']}")
    sized = [(counts([op for k in range(a0, a1 + 1) for op in bl[k]["ins"]]), a0, a1) for a0, a1 in inner]
    main_fma = max((c["fma"] for c, _, _ in sized), default=0)
    for c, a0, a1 in sized:
        # a two-row step is 6 FMAs + 2 multiplies; the loop with the most FMAs is the unrolled one, the others are
        # its remainder (not taken in a full block of 64 rows)
        rows_per_trip = max(c["fma"] // 3, 1)
        trips = 64.0 / rows_per_trip if c["fma"] == main_fma else 0.0
        print(f"  s loop {bl[a0]['name']} .. {bl[a1]['name']}: {c['valu']} VALU ({c['fma']} fma), {c['lds']} LDS, "
              f"{c['salu']} SALU per trip of {rows_per_trip} rows, {trips:.0f} trips in a full block")
        for k in keys:
            dyn[k] += c[k] * trips
        in_inner.update(range(a0, a1 + 1))
    c = counts([op for k in range(i0, i1 + 1) if k not in in_inner for op in bl[k]["ins"]])
    print(f"  outside the s loop: {c['valu']} VALU ({c['fma']} fma), {c['lds']} LDS, {c['salu']} SALU per block")
    for k in keys:
        dyn[k] += c[k]
    print(f"  per full 64-row block: {dyn['valu']:.0f} VALU, {dyn['lds']:.0f} LDS, {dyn['salu']:.0f} SALU, "
          f"{dyn['branch']:.0f} branches;  per row: {dyn['valu'] / 64:.2f} VALU, {dyn['lds'] / 64:.2f} LDS")
    in_loop = counts([op for k in range(i0, i1 + 1) for op in bl[k]["ins"]])["mfma"]
    group = [k for k, b in enumerate(bl) if counts(b["ins"])["mfma"] and not i0 <= k <= i1]
    if in_loop:
        print(f"  {in_loop} MFMA inside the block loop")
    if group:
        g = counts([op for k in group for op in bl[k]["ins"]])
        print(f"  group phase (blocks {', '.join(bl[k]['name'] for k in group)}, once per 16 blocks): {g['mfma']} MFMA, "
              f"{g['valu']} VALU, {g['lds']} LDS, {g['gload']} global loads, {g['salu']} SALU;  per block: "
              f"{g['mfma'] / 16:.2f} MFMA, {g['valu'] / 16:.1f} VALU, {g['lds'] / 16:.1f} LDS")
        print(f"  per full 64-row block with its share of the group phase: {dyn['valu'] + g['valu'] / 16:.0f} VALU, "
              f"{g['mfma'] / 16:.2f} MFMA, {dyn['lds'] + g['lds'] / 16:.0f} LDS")


def _regs(operand):
    """The 32-bit vector registers an operand names: v5 -> {5}, v[4:5] -> {4, 5}, -v[4:5] -> {4, 5}; none for s, literals."""
    m = re.match(r"^[-|]*v\[(\d+):(\d+)\]", operand)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.match(r"^[-|]*v(\d+)\b", operand)
    return {int(m.group(1))} if m else set()


def finish_phases(lines, rows, kernel="k_steady_finish", proven=False):
    """The full block of the finishing launch (one basic block: the one with the most FMAs) by phase: z = u + Q s up to
    the store of z (ds_write_b64), the state update up to the join (its first v_permlane32_swap), and the rest.  Per
    phase: vector instructions, FP64 FMAs and multiplies, LDS reads, s_waitcnt, the longest chain of dependent FP64
    instructions, and the FMAs issued directly behind an FP64 instruction that writes the accumulator they add to."""
    body = kernel_body(lines, kernel, rows, None, proven=proven)
    cur, best = [], []
    for ln in body + [".LBB_end:"]:
        s = ln.strip()
        if not ln.startswith("\t") and re.match(r"^(\.LBB\w+|; %bb\.\d+):?", s):
            if sum(x[0].startswith(("v_fma_f64", "v_fmac_f64")) for x in cur) > \
                    sum(x[0].startswith(("v_fma_f64", "v_fmac_f64")) for x in best):
                best = cur
            cur = []
        elif s and not s.startswith((";", ".")):
            parts = s.split(None, 1)
            cur.append((parts[0], [o.strip() for o in parts[1].split(",")] if len(parts) > 1 else []))
    cut1 = next((i for i, x in enumerate(best) if x[0] == "ds_write_b64"), len(best))
    cut2 = next((i for i, x in enumerate(best) if x[0].startswith("v_permlane32_swap")), len(best))
    print(f"{kernel}<{rows}{', proven' if proven else ''}>, the full block ({len(best)} instructions, {sum(x[0].startswith('v_') for x in best)} "
          f"vector) by phase:")
    for name, part in (("z = u + Q s", best[:cut1]), ("state update", best[cut1:cut2]), ("join and loop", best[cut2:])):
        depth, deepest, behind, prev = {}, 0, 0, set()
        for op, args in part:
            f64 = op.startswith(("v_fma_f64", "v_fmac_f64", "v_mul_f64", "v_add_f64"))
            if not f64:
                if op.startswith("v_"):         # (a wait or an LDS read between two FMAs takes no VALU slot)
                    prev = set()
                continue
            dst = _regs(args[0])
            src = set().union(*[_regs(a) for a in args[1:]]) | (dst if op.startswith("v_fmac") else set())
            d = 1 + max((depth.get(r, 0) for r in src), default=0)
            for r in dst:
                depth[r] = d
            deepest = max(deepest, d)
            acc = dst if op.startswith("v_fmac") else _regs(args[-1])
            behind += bool(acc & prev) and op.startswith(("v_fma_f64", "v_fmac_f64"))
            prev = dst
        c = counts([op for op, _ in part])
        mul = sum(op.startswith("v_mul_f64") for op, _ in part)
        print(f"  {name:14s}: {c['valu']:3d} VALU ({c['fma']} fma, {mul} mul), {sum(op.startswith('ds_read') for op, _ in part):2d} "
              f"LDS reads, {sum(op == 's_waitcnt' for op, _ in part):2d} s_waitcnt; longest dependent FP64 chain {deepest}, "
              f"{behind} FMAs directly behind the write of their accumulator")


def functions(lines, twice=None, desc=None):
    """name -> instruction lines of every function of a listing, with the per-function label numbers taken out (a
    function added in front renumbers the labels of all that follow).  `twice`, if given, collects the names that
    occur more than once (listings of several translation units, concatenated); `desc`, if given, every kernel's
    descriptor: the .amdhsa_* lines of its .amdhsa_kernel block (register counts, LDS and scratch bytes)."""
    out, name, body = {}, None, []
    for ln in lines:
        if name is None:
            m = re.match(r"^(_Z\S+):", ln)
            if m:
                name, body = m.group(1), []
        elif ln.startswith(".Lfunc_end"):
            if twice is not None and name in out:
                twice.append(name)
            out[name], name = body, None
        else:
            s = ln.split(";")[0].strip()
            if s and (not s.startswith(".") or s.startswith(".LBB")):     # instructions and block labels
                body.append(re.sub(r"\.LBB\d+_", ".LBB_", s))
            elif desc is not None and s.startswith(".amdhsa_") and not s.startswith(".amdhsa_kernel"):
                desc.setdefault(name, []).append(" ".join(s.split()))
    return out


def compare(lines, other):
    """Which kernels' instructions differ between two listings (registers included: the operands are compared), and
    which kernels' descriptors (register counts, LDS and scratch bytes: the same instructions can run under others)."""
    twice_a, twice_b, desc_a, desc_b = [], [], {}, {}
    a, b = functions(lines, twice_a, desc_a), functions(other, twice_b, desc_b)
    changed = sorted(k for k in a.keys() & b.keys() if a[k] != b[k])
    desc_changed = sorted(k for k in a.keys() & b.keys() if desc_a.get(k) != desc_b.get(k))
    print(f"{len(a)} functions in this listing, {len(b)} in the other; {len(a.keys() & b.keys())} in both, "
          f"{len(changed)} of them differ; {len(desc_a)} kernel descriptors here, {len(desc_b)} in the other, "
          f"{len(desc_changed)} differ")
    for k in sorted(twice_a):
        print(f"  twice in this listing: {k}")
    for k in sorted(twice_b):
        print(f"  twice in the other: {k}")
    for k in changed:
        print(f"  differs: {k}")
    for k in desc_changed:
        print(f"  descriptor differs: {k}")
    for k in sorted(a.keys() - b.keys()):
        print(f"  only here: {k} ({len(a[k])} lines)")
    for k in sorted(b.keys() - a.keys()):
        print(f"  only in the other: {k}")


def rank1(lines):
    """k_steady_rank1: every block of its row loop (the loop around the block with the half-wave tree: row_bcast:15)."""
    start = next(i for i, ln in enumerate(lines) if re.match(r"^_Z\S*14k_steady_rank1\S*:", ln))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    body = lines[start:end]
    bl = blocks(body)
    vgpr = next((ln.split(",")[-1].strip() for ln in lines if ".num_vgpr," in ln and "k_steady_rank1" in ln), "?")
    total = counts([op for b in bl for op in b["ins"]])
    print(f"k_steady_rank1: {len(bl)} blocks, {total['valu']} VALU, {total['lds']} LDS, {total['scratch']} scratch "
          f"(spill) in all; {vgpr} VGPRs")
    # five DPP steps of one double per row: a block with 10 n of them holds n rows (an unrolled body)
    tree = [i for i, b in enumerate(bl) if b["ins"].count("v_mov_b32_dpp") and b["ins"].count("v_mov_b32_dpp") % 10 == 0]
    if len(tree) == 1:
        i0, i1 = row_loop_outer(bl, tree[0])
    else:                                       # the block loop: the smallest loop around every block that holds rows
        idx = {b["name"]: i for i, b in enumerate(bl)}
        loops = [(idx[t], j) for j, b in enumerate(bl) for t in b["targets"]
                 if t in idx and idx[t] <= tree[0] and j >= tree[-1]]
        i0, i1 = min(loops, key=lambda r: r[1] - r[0])
    print(f"row loop: blocks {bl[i0]['name']} .. {bl[i1]['name']} (`tree`: the half-wave sums; `rows`: trees in the block)")
    print(f"{'block':>14} {'VALU':>5} {'fma':>4} {'dpp':>4} {'SALU':>5} {'br':>3} {'store':>5} {'load':>5} {'rows':>4}  role")
    for k in range(i0, i1 + 1):
        b = bl[k]
        if not b["ins"]:
            continue
        c = counts(b["ins"])
        fma = sum(op.startswith(("v_fma_f64", "v_fmac_f64", "v_mul_f64", "v_add_f64")) for op in b["ins"])
        rows = b["ins"].count("v_mov_b32_dpp") // 10 if k in tree else 0
        print(f"{b['name']:>14} {c['valu']:5d} {fma:4d} {b['ins'].count('v_mov_b32_dpp'):4d} {c['salu']:5d} "
              f"{c['branch']:3d} {sum(op.startswith('global_store') for op in b['ins']):5d} {c['gload']:5d} "
              f"{rows or '':>4}  {'tree' if k in tree else ''}")
    for k in tree:
        c, rows = counts(bl[k]["ins"]), bl[k]["ins"].count("v_mov_b32_dpp") // 10
        if i0 <= k <= i1 and rows > 1:
            print(f"  {bl[k]['name']}: {rows} rows; per row {c['valu'] / rows:.1f} VALU, {c['salu'] / rows:.1f} SALU, "
                  f"{c['branch'] / rows:.2f} branches")


def row_loop_outer(bl, reg):
    """Largest [header, latch] range closed by a backward branch to the header of the loop that contains `reg`."""
    idx = {b["name"]: i for i, b in enumerate(bl)}
    head = max(i for i in range(reg + 1) if any(idx.get(t) == i for j in range(reg, len(bl)) for t in bl[j]["targets"]))
    latch = max(j for j in range(reg, len(bl)) if any(idx.get(t) == head for t in bl[j]["targets"]))
    return head, latch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank1", action="store_true", help="k_steady_rank1: the blocks of its row loop")
    ap.add_argument("--compare", help="a second listing: name the kernels whose instructions differ from it")
    ap.add_argument("--asm", help="existing device assembly listing (default: compile gadfly_hip.hip)")
    ap.add_argument("--kernel", default="k_factor7")
    ap.add_argument("--rows", type=int, default=60)
    ap.add_argument("--rowstore", action="store_true", help="the ROWSTORE = true instance (k_factor7 only)")
    ap.add_argument("--sample", action="store_true", help="the SAMPLE = true instance (the sampling sweeps)")
    ap.add_argument("--steady", action="store_true", help="the STEADY = true instance (k_factor7 only), and the block loops of k_steady_tail / k_steady_finish")
    ap.add_argument("--all", action="store_true", help="also print blocks outside loops")
    a = ap.parse_args()
    asm = a.asm
    if asm is None:
        asm = os.path.join(tempfile.mkdtemp(prefix="isa_rows_"), "gadfly_hip.s")
        compile_asm(asm)
    lines = open(asm).read().splitlines()
    if a.compare:
        compare(lines, open(a.compare).read().splitlines())
    if a.rank1:
        rank1(lines)
    if a.compare or a.rank1:
        return 0
    rowstore =(a.rowstore if a.kernel == "k_factor7" else None)
    body = kernel_body(lines, a.kernel, a.rows, rowstore, a.sample, a.steady)
    tag = kernel_tag(a.kernel, a.rows, rowstore, a.sample, a.steady)
    bl = blocks(body)
    vgpr = next((ln.split(",")[-1].strip() for ln in lines
                 if ".num_vgpr," in ln and tag.search(ln)), "?")
    total = counts([op for b in bl for op in b["ins"]])
    print(f"{a.kernel}<{a.rows}{'' if rowstore is None else ', ' + str(rowstore).lower()}>"
          f"{' (sampling)' if a.sample else ''}: {len(bl)} blocks, "
          f"{total['valu']} VALU, {total['lds']} LDS, {total['scratch']} scratch (spill) in all; {vgpr} VGPRs")
    reg = max(range(len(bl)), key=lambda i: counts(bl[i]["ins"])["fma"])
    i0, i1 = row_loop(bl, reg) if not a.all else (0, len(bl) - 1)
    print(f"row loop: blocks {bl[i0]['name']} .. {bl[i1]['name']}; `regular` = the block with the mat-vec's FMAs, "
          f"`exp` = a block holding fm_exp / fm_sincos (v_ldexp_f64)")
    print(f"{'block':>14} {'VALU':>5} {'fma':>4} {'LDS':>4} {'SALU':>5} {'br':>3} {'mov64':>5} {'movb32':>6} {'spill':>5}  role")
    def show(k0, k1, regular):
        for k in range(k0, k1 + 1):
            b = bl[k]
            if not b["ins"]:
                continue
            c = counts(b["ins"])
            role = "regular" if k == regular else ("exp" if c["ldexp"] else "")
            print(f"{b['name']:>14} {c['valu']:5d} {c['fma']:4d} {c['lds']:4d} {c['salu']:5d} {c['branch']:3d} "
                  f"{c['mov64']:5d} {c['movb32']:6d} {c['scratch']:5d}  {role}")

    show(i0, i1, reg)
    if a.steady and not a.all:
        steady_tail(lines, a.rows)
        for proven in (False, True):            # without and with GF_SWEEP_AXIS_PROVEN
            steady_tail(lines, a.rows, "k_steady_finish", proven)
            finish_phases(lines, a.rows, proven=proven)
    return 0


if __name__ == "__main__":
    sys.exit(main())
