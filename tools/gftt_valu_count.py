#!/usr/bin/env python3
"""gftt_valu_count.py [--keep out.s] [--asm in.s] [--hist] -- static VALU counts
of the GFTT eigenvalue walk (klt_gftt.hip), no GPU needed.

Compiles klt_gftt.hip to gfx950 assembly with the Makefile's own command line
(taken from a dry run of make, the object's `-c -o` replaced by device-only `-S`)
and prints, for the compact 8-bit instance (gftt_eig_kernel<true>, the frame
loop's):

  * steady-row blocks: every basic block that holds exactly one v_sqrt_f32 and
    nine v_cvt_f64_f32 (one walked row's arithmetic, straight line), its VALU
    count and, with --hist, its opcode histogram;
  * steady loops: every innermost loop whose body holds more than one such
    block (TBDK_GFTT_EIG_PREF_C rows a turn): the VALU instructions of the
    whole body, each block counted once, per turn and per row, and the
    v_readfirstlane among them.  A loop nested in the body (the per-descriptor
    loop the compiler wraps round a buffer access whose descriptor it takes for
    per-lane data) is counted as one pass, which is what it runs when the
    descriptor is in fact the same in every lane;
  * generic-row blocks: every basic block with a v_sqrt_f32 and no
    v_cvt_f64_f32 (the run-time-flag row: its row sums sit in a block of their
    own, under a branch), and the loops of exactly one row round them, counted
    as above;
  * every eigenvalue instance's VGPRs.

VALU = every instruction whose mnemonic starts with v_.  A counter only.
"""
import argparse
import collections
import os
import re
import shlex
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opencv_amd", "csrc")
BRANCH = re.compile(r"^(s_cbranch_\w+|s_branch)\s+(\S+)")
KEY = "gftt_eig_kernelILb1E"


def compile_asm(out):
    dry = subprocess.check_output(["make", "-n", "-B", "-C", CSRC, "../../build/tbdk/klt_gftt.o"], text=True)
    line = next(ln for ln in dry.splitlines() if "klt_gftt.hip" in ln and " -c " in ln)
    cmd, skip = [], False
    for tok in shlex.split(line):
        if skip:
            skip = False
        elif tok == "-o":
            skip = True
        elif tok != "-c":
            cmd.append(tok)
    subprocess.check_call(cmd + ["--cuda-device-only", "-S", "-o", out], cwd=CSRC)


def functions(path):
    """{symbol: [instruction / label lines]} and {symbol: vgpr count} of the eigenvalue kernels"""
    fns, vgprs, cur, kernel = {}, {}, None, ""
    for raw in open(path):
        ln = raw.strip()
        m = re.match(r"^(_Z\w+):", ln)
        if m and "gftt_eig" in m.group(1):
            cur = m.group(1)
            fns[cur] = []
            continue
        if cur and ln.startswith(".Lfunc_end"):
            cur = None
            continue
        m = re.match(r"^\.amdhsa_next_free_vgpr\s+(\d+)", ln)
        if m and kernel in fns:
            vgprs[kernel] = int(m.group(1))
        m = re.match(r"^\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            kernel = m.group(1)
        if cur is not None and ln:
            fns[cur].append(ln)
    return fns, vgprs


def blocks(lines):
    """basic blocks [(name, labels, instructions)], split at labels, at the
    compiler's block comments and after every branch"""
    out, name, labels, ins = [], "entry", [], []

    def flush():
        nonlocal labels, ins
        if labels or ins:
            out.append((name, labels, ins))
        labels, ins = [], []

    for ln in lines:
        m = re.match(r"^(\.LBB\w+):", ln)
        c = re.match(r"^; (%bb\.\d+):", ln)
        if m or c:
            if ins:
                flush()
            if m:
                labels.append(m.group(1))
            name = m.group(1) if m else c.group(1)
            continue
        if ln.startswith(";") or ln.startswith("."):
            continue
        ins.append(ln.split(";")[0].strip())
        if BRANCH.match(ins[-1]):
            flush()
            name += "+"
    flush()
    return out


def count(ins, prefix="v_"):
    return sum(1 for i in ins if i.startswith(prefix))


def hist(ins):
    h = collections.Counter(i.split()[0] for i in ins if i.startswith("v_"))
    return ", ".join(f"{n} {op}" for op, n in sorted(h.items(), key=lambda kv: (-kv[1], kv[0])))


def analyse(lines):
    bl = blocks(lines)
    at = {lb: i for i, (_, lbs, _) in enumerate(bl) for lb in lbs}
    sq = [count(ins, "v_sqrt_f32") for _, _, ins in bl]
    cv = [count(ins, "v_cvt_f64_f32") for _, _, ins in bl]
    steady = [i for i in range(len(bl)) if sq[i] == 1 and cv[i] == 9]
    generic = [i for i in range(len(bl)) if sq[i] >= 1 and cv[i] == 0]
    # loops: a branch back to a label at or before its own block; the body is
    # the run of blocks from the label to the branch
    loops = []
    for i, (_, _, ins) in enumerate(bl):
        m = BRANCH.match(ins[-1]) if ins else None
        if m and m.group(2) in at and at[m.group(2)] <= i:
            loops.append((at[m.group(2)], i))

    def body(lo, hi):
        ins = [x for _, _, b in bl[lo:hi + 1] for x in b]
        return {"header": bl[lo][1][0], "valu": count(ins), "rfl": count(ins, "v_readfirstlane"),
                "rows": sum(sq[lo:hi + 1]), "steady": sum(1 for i in steady if lo <= i <= hi)}

    def innermost(want):
        sel = [(lo, hi) for lo, hi in loops if want(body(lo, hi))]
        return [body(lo, hi) for lo, hi in sel
                if not any((a, b) != (lo, hi) and lo <= a and b <= hi for a, b in sel)]

    return {"steady": [(bl[i][0], count(bl[i][2]), hist(bl[i][2])) for i in steady],
            "generic": [(bl[i][0], count(bl[i][2])) for i in generic],
            "steady_loops": innermost(lambda b: b["rows"] > 1 and b["steady"] == b["rows"]),
            "row_loops": innermost(lambda b: b["rows"] == 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keep", help="keep the assembly at this path")
    ap.add_argument("--asm", help="count an existing assembly file instead of compiling")
    ap.add_argument("--hist", action="store_true", help="print the opcode histogram of every steady-row block")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        path = args.asm or args.keep or os.path.join(tmp, "klt_gftt.s")
        if not args.asm:
            compile_asm(os.path.abspath(path))
        fns, vgprs = functions(path)
    name = next(f for f in fns if KEY in f)
    r = analyse(fns[name])
    print(f"{name}: {vgprs.get(name)} VGPRs")
    print("  steady-row blocks (one v_sqrt_f32, nine v_cvt_f64_f32): " +
          " ".join(f"{n}: {v}" for n, v, _ in r["steady"]) + " VALU")
    if args.hist:
        for n, v, h in r["steady"]:
            print(f"    {n}: {h}")
    for b in r["steady_loops"]:
        print(f"  steady loop {b['header']}: {b['valu']} VALU a turn of {b['rows']} rows = {b['valu'] / b['rows']:.1f} a row, "
              f"{b['rfl']} of them v_readfirstlane")
    print("  generic-row blocks (v_sqrt_f32, no v_cvt_f64_f32): " + " ".join(f"{n}: {v}" for n, v in r["generic"]) + " VALU")
    for b in r["row_loops"]:
        kind = "steady" if b["steady"] else "generic"
        print(f"  one-row loop {b['header']} ({kind}): {b['valu']} VALU a row, {b['rfl']} of them v_readfirstlane")
    rows = {}
    for k, v in vgprs.items():
        m = re.search(r"gftt_(eig_kernel|eig_masked_kernel|eigpx_kernel)ILb(\d)E(?:Lb(\d)ELi(\d)E)?", k)
        if not m:
            continue
        masked = m.group(1) == "eig_masked_kernel" or m.group(3) == "1"
        px = {None: "u8", "1": "u16", "2": "f32"}[m.group(4)]
        rows[(px, "compact" if m.group(2) == "1" else "plane", "masked" if masked else "plain")] = v
    print("  VGPRs: " + "; ".join(f"{' '.join(k)}: {v}" for k, v in sorted(rows.items())))
    return 0 if vgprs.get(name, 999) <= 128 else 1


if __name__ == "__main__":
    sys.exit(main())
