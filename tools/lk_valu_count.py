#!/usr/bin/env python3
"""lk_valu_count.py [--win W] [--keep out.s] -- static VALU counts of the
several-points-per-wave PyrLK kernel (klt_lk_multi.hip), no GPU needed.

Compiles klt_lk_multi.hip to gfx950 assembly with the Makefile's own command
line (taken from a dry run of make, the object's `-c -o` replaced by device-only
`-S`) and prints, for the window-W forward Scharr-on-the-fly instance
(lk_multi_kernel<W, W, true, false>, default W = 21):

  * setup: the VALU instructions of each arm of the level setup's window block
    (plain, masked, integer origin), found by the marker comments the arms'
    source rows pass through (klt_lk_multi_body.inc; EXTRA=-DTBDK_LK_INT_ORIGIN=0
    in the environment builds the kernel without the integer-origin arm); with
    no marker in the assembly, the basic block with the most v_dot2* (and the
    runner-up when that holds at least half as many).  Work the compiler moves
    below the arms' join is in no arm's count: with two arms the 42 VALU that
    turn the I sums into ic (mask and subtract per row) sat there, with three
    they are inside the plain and the masked arm;
  * step / solo step: the VALU instructions on the cheapest way (by VALU count)
    from a block that holds v_add_u32_dpp (the b-sum scans) once round and back
    to it, not through the setup: the Newton step of all the wave's points (the
    way with the most v_dot2*) and the one-point step (the fewest);
  * the VGPR count of every lk_multi instance in the file (exit status 1 when
    the measured instance needs more than 128: 4 waves per SIMD).

VALU = every instruction whose mnemonic starts with v_.  A branch on exec is
counted as not taken: the masked region it would skip (the update of the points
still stepping) belongs to the step.  A counter only.
"""
import argparse
import heapq
import os
import re
import shlex
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opencv_amd", "csrc")
ARMS = {"; plain row": "plain arm", "; masked row": "masked arm", "; integer-origin row": "integer-origin arm"}
BRANCH = re.compile(r"^(s_cbranch_\w+|s_branch)\s+(\S+)")


def compile_asm(out):
    dry = subprocess.check_output(["make", "-n", "-B", "-C", CSRC, "../../build/tbdk/klt_lk_multi.o"], text=True)
    line = next(ln for ln in dry.splitlines() if "klt_lk_multi.hip" in ln and " -c " in ln)
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
    """{symbol: [instruction / label lines]} and {symbol: vgpr count}"""
    fns, vgprs, cur, kernel = {}, {}, None, ""
    for raw in open(path):
        ln = raw.strip()
        m = re.match(r"^(_Z\w+):", ln)
        if m and "lk_multi" in m.group(1):
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
    """basic blocks: [(labels, instructions)], split at labels, at the
    compiler's block comments and after every branch"""
    out, labels, ins, marks = [], [], [], set()

    def flush():
        nonlocal labels, ins, marks
        if labels or ins:
            out.append((labels, ins, marks))
        labels, ins, marks = [], [], set()

    for ln in lines:
        m = re.match(r"^(\.LBB\w+):", ln)
        if m or ln.startswith("; %bb."):
            if ins:
                flush()
            if m:
                labels.append(m.group(1))
            continue
        if ln in ARMS:
            marks.add(ARMS[ln])
        if ln.startswith(";") or ln.startswith("."):
            continue
        ins.append(ln.split(";")[0].strip())
        if BRANCH.match(ins[-1]):
            flush()
    flush()
    return out


def count(ins, prefix="v_"):
    return sum(1 for i in ins if i.startswith(prefix))


def analyse(lines):
    bl = blocks(lines)
    n = len(bl)
    at = {lb: i for i, (lbs, _, _) in enumerate(bl) for lb in lbs}
    succ = [[] for _ in range(n)]
    for i, (_, ins, _) in enumerate(bl):
        m = BRANCH.match(ins[-1]) if ins else None
        # a branch on exec only skips a masked region no lane needs: the count
        # follows the region (the fall-through)
        if m and m.group(2) in at and not m.group(1).startswith("s_cbranch_exec"):
            succ[i].append(at[m.group(2)])
        if not (m and m.group(1) == "s_branch") and not (ins and ins[-1].startswith("s_endpgm")) and i + 1 < n:
            succ[i].append(i + 1)
    valu = [count(ins) for _, ins, _ in bl]
    dot2 = [count(ins, "v_dot2") for _, ins, _ in bl]
    dpp = [sum(1 for i in ins if i.startswith("v_add_u32_dpp")) for _, ins, _ in bl]

    # setup: the block(s) with the most v_dot2*
    order = sorted(range(n), key=lambda i: -dot2[i])
    setup = [order[0]] + [i for i in order[1:2] if 2 * dot2[i] >= dot2[order[0]]]
    marked = [i for i in range(n) if bl[i][2]]
    if marked:
        setup = marked

    # one step = the cheapest way (by VALU count) from a block that holds the
    # b-sum scans round the Newton loop and back to it, not through the setup
    steps = {}
    for t in range(n):
        if not dpp[t] or t in setup:
            continue
        best, heap = {}, []
        for s in succ[t]:
            if s not in setup and (s not in best or valu[s] < best[s][0]):
                best[s] = (valu[s], [s])
                heapq.heappush(heap, (valu[s], s, [s]))
        while heap:
            c, x, path = heapq.heappop(heap)
            if c > best[x][0] or x == t:
                continue
            for s in succ[x]:
                if s not in setup and (s not in best or c + valu[s] < best[s][0]):
                    best[s] = (c + valu[s], path + [s])
                    heapq.heappush(heap, (c + valu[s], s, path + [s]))
        if t in best:
            c, path = best[t]
            d2 = sum(dot2[i] for i in path)
            if d2 and (d2 not in steps or c < steps[d2]["valu"]):
                f64 = sum(1 for i in path for x in bl[i][1] if x.startswith("v_") and "f64" in x.split()[0])
                steps[d2] = {"valu": c, "dot2": d2, "f64": f64, "dpp": sum(dpp[i] for i in path),
                             "blocks": [(bl[i][0] or ["(fallthrough)"])[0] for i in path]}
    # a step's b sums are two scans of six DPP adds each: a way round with more
    # goes through another level's setup (its G sums), not round the Newton loop
    steps = [s for s in steps.values() if s["dpp"] == 12]
    steps.sort(key=lambda s: -s["dot2"])
    return {"setup": [{"block": (bl[i][0] or ["(fallthrough)"])[0], "valu": valu[i], "dot2": dot2[i],
                       "arm": ", ".join(sorted(bl[i][2]))} for i in setup],
            "steps": steps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--win", type=int, default=21)
    ap.add_argument("--keep", help="keep the assembly at this path")
    ap.add_argument("--asm", help="count an existing assembly file instead of compiling")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        path = args.asm or args.keep or os.path.join(tmp, "klt_lk_multi.s")
        if not args.asm:
            compile_asm(os.path.abspath(path))
        fns, vgprs = functions(path)
    key = f"lk_multi_kernelILi{args.win}ELi{args.win}ELb1ELb0E"
    name = next(f for f in fns if key in f)
    r = analyse(fns[name])
    print(f"{name}: {vgprs.get(name)} VGPRs")
    for s in r["setup"]:
        print(f"  setup{', ' + s['arm'] if s['arm'] else ''} (block {s['block']}): {s['valu']} VALU ({s['dot2']} v_dot2*)")
    for k, s in enumerate(r["steps"]):
        tag = "step (all points)" if k == 0 else "solo step" if k == len(r["steps"]) - 1 else "step (other)"
        print(f"  {tag}: {s['valu']} VALU on the cheapest way round ({s['dot2']} v_dot2*, {s['f64']} f64, "
              f"{s['dpp']} dpp adds) via {' '.join(s['blocks'])}")
    # every instance's VGPRs, by window: forward planes / Scharr on the fly / dense / backward
    rows = {}
    for k, v in vgprs.items():
        m = re.search(r"lk_multi(_back)?_kernelILi(\d+)ELi\d+E(?:Lb(\d)ELb(\d))?", k)
        col = "back" if m.group(1) else "dense" if m.group(4) == "1" else "fly" if m.group(3) == "1" else "planes"
        rows.setdefault(int(m.group(2)), {})[col] = v
    print("  VGPRs by window (planes fly dense back): " +
          "; ".join(f"{w}: " + " ".join(str(rows[w].get(c, "-")) for c in ("planes", "fly", "dense", "back"))
                    for w in sorted(rows)))
    # exit status: the measured instance within the 4-waves-per-SIMD budget
    return 0 if vgprs.get(name, 999) <= 128 else 1


if __name__ == "__main__":
    sys.exit(main())
