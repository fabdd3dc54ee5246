#!/usr/bin/env python3
"""Static figures of the approach walks' free-flight step (profiles/experiments/approach_step.txt).

Compiles the integrator's units to gfx950 assembly with the Makefile's flags (no GPU needed) and prints
  - the vector instructions per free-flight step in the walk loops of approach_k<RngPhiloxR<7>>,
    approach_local_k<RngPhiloxR<7>, true> and approach_local_tab_k<RngPhiloxR<7>>,
  - per kernel of both units: vector instructions, VGPRs, occupancy, scratch,
parent against this build.  The parent's figures come from a checkout given with --parent (compiled in the same run) or, without
one, from the record in profiles/experiments/approach_step.txt.

A walk loop is found by its shape, not by what it contains: among the innermost loops of the kernel (a backward branch with no
other loop inside) the one with the most vector instructions.  The loops the kernel keeps for sequential streams and for majorants
with a minus sign are shorter copies of the same step.  A loop unrolled by hand or by pragma makes VP_WALK_UNROLL steps per
iteration (the define in csrc/vp_integrator.h; 1 where it is absent): the count is divided by it.

  python scripts/approach_step_isa.py [--parent DIR] [--dev] [--exact-only] [--json] [--keep DIR]
"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "cuda-volpath_amd"
UNITS = ("vp_kernels", "vp_kernels_fast")
WALKS = (("approach_k", "approach_k<RngPhiloxR<7>>"),
         ("approach_local_k", "approach_local_k<RngPhiloxR<7>, true>"),
         ("approach_local_tab_k", "approach_local_tab_k<RngPhiloxR<7>>"))
RECORD = os.path.join(ROOT, "profiles", "experiments", "approach_step.txt")


def makefile_flags(tree):
    """HIPCC, HIPFLAGS as the Makefile of `tree` states them (ARCH = gfx950)."""
    text = open(os.path.join(tree, PKG, "Makefile")).read().replace("\\\n", " ")
    m = re.search(r"^HIPFLAGS\s*=\s*(.*)$", text, re.M)
    if not m:
        raise RuntimeError("no HIPFLAGS in the Makefile")
    flags = m.group(1).replace("$(ARCH)", os.environ.get("ARCH", "gfx950")).split()
    m = re.search(r"^HIPCC\s*\?=\s*(\S+)", text, re.M)
    hipcc = os.environ.get("HIPCC") or (m.group(1) if m else "hipcc")
    return hipcc, flags


def compile_unit(tree, unit, out, dev):
    hipcc, flags = makefile_flags(tree)
    cmd = [hipcc] + flags + (["-DVP_DEV_BUILD"] if dev else []) + ["--cuda-device-only", "-S", os.path.join("csrc", unit + ".hip"), "-o", out]
    subprocess.run(cmd, cwd=os.path.join(tree, PKG), check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    if not os.path.exists(tool):
        tool = shutil.which("c++filt")
    if not tool:
        return dict((n, n) for n in names)
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, out))


def parse(path):
    """{mangled kernel name: {"insts": [(mnemonic, operands)], "labels": {label: index}, vgpr, occupancy, scratch}}"""
    kernels, cur, name = {}, None, None
    start = re.compile(r"^(\w+):\s*; @(\w+)")
    label = re.compile(r"^(\.LBB\d+_\d+):")
    res = re.compile(r"^; (NumVgprs|Occupancy|ScratchSize):\s*(\d+)")
    for line in open(path):
        m = start.match(line)
        if m and m.group(1) == m.group(2):
            name, cur = m.group(1), {"insts": [], "labels": {}}
            continue
        if cur is not None:
            if line.startswith(".Lfunc_end"):
                kernels[name], cur = cur, None
                continue
            m = label.match(line)
            if m:
                cur["labels"][m.group(1)] = len(cur["insts"])
            elif line.startswith("\t") and not line.startswith("\t.") and not line.startswith("\t;"):
                parts = line.split(";")[0].split(None, 1)
                if parts:
                    cur["insts"].append((parts[0], parts[1].strip() if len(parts) > 1 else ""))
            continue
        m = res.match(line)
        if m and name in kernels:
            kernels[name].setdefault({"NumVgprs": "vgpr", "Occupancy": "occupancy", "ScratchSize": "scratch"}[m.group(1)], int(m.group(2)))
    # only kernels have the resource lines
    return dict((k, v) for k, v in kernels.items() if "occupancy" in v)


def is_vector(mnemonic):
    return mnemonic.startswith("v_")


def innermost_loops(k):
    """[(first instruction, last instruction, vector instructions)] of the loops of the kernel that enclose no other loop.

    From the control-flow graph, not from the layout (the blocks of a loop need not be contiguous, its latch need not be its
    header): a loop is a strongly connected component; the loops inside it are those of the component without its entry blocks."""
    insts, labels = k["insts"], k["labels"]
    leaders = {0} | set(labels.values())
    for j, (mn, _) in enumerate(insts):
        if mn.startswith("s_cbranch") or mn in ("s_branch", "s_endpgm", "s_setpc_b64"):
            leaders.add(j + 1)
    starts = sorted(x for x in leaders if x < len(insts))
    block_of = {}
    for n, st in enumerate(starts):
        for j in range(st, starts[n + 1] if n + 1 < len(starts) else len(insts)):
            block_of[j] = n
    succ = dict((n, set()) for n in range(len(starts)))
    for n, st in enumerate(starts):
        end = (starts[n + 1] if n + 1 < len(starts) else len(insts)) - 1
        mn, ops = insts[end]
        if mn.startswith("s_cbranch") or mn == "s_branch":
            t = labels.get(ops.split()[0] if ops else "")
            if t is not None and t in block_of:
                succ[n].add(block_of[t])
        if mn not in ("s_branch", "s_endpgm", "s_setpc_b64") and n + 1 < len(starts):
            succ[n].add(n + 1)

    def components(nodes):
        """Tarjan, iterative; the components of the graph restricted to `nodes` that hold a cycle."""
        index, low, on, stack, out, count = {}, {}, set(), [], [], [0]
        for root in nodes:
            if root in index:
                continue
            work = [(root, iter(sorted(succ[root] & nodes)))]
            index[root] = low[root] = count[0]; count[0] += 1; stack.append(root); on.add(root)
            while work:
                v, it = work[-1]
                for w in it:
                    if w not in index:
                        index[w] = low[w] = count[0]; count[0] += 1; stack.append(w); on.add(w)
                        work.append((w, iter(sorted(succ[w] & nodes))))
                        break
                    if w in on:
                        low[v] = min(low[v], index[w])
                else:
                    work.pop()
                    if work:
                        low[work[-1][0]] = min(low[work[-1][0]], low[v])
                    if low[v] == index[v]:
                        comp = set()
                        while True:
                            w = stack.pop(); on.discard(w); comp.add(w)
                            if w == v:
                                break
                        if len(comp) > 1 or v in succ[v]:
                            out.append(comp)
        return out

    def innermost(nodes):
        found = []
        for comp in components(nodes):
            entries = set(n for n in comp if any(n in succ[p] for p in succ if p not in comp)) or {min(comp)}
            found += innermost(comp - entries) or [comp]
        return found

    loops = []
    for comp in innermost(set(succ)):
        idx = [j for j in range(len(insts)) if block_of[j] in comp]
        loops.append((min(idx), max(idx), sum(is_vector(insts[j][0]) for j in idx)))
    return sorted(loops)


def walk_unroll(tree):
    m = re.search(r"^#define\s+VP_WALK_UNROLL\s+(\d+)", open(os.path.join(tree, PKG, "csrc", "vp_integrator.h")).read(), re.M)
    return int(m.group(1)) if m else 1


def figures(tree, dev, keep=None, units=UNITS):
    """{"walks": {kernel: vector instructions per step}, "kernels": {unit: {name: [v-insts, vgpr, occupancy, scratch]}}}"""
    tmp = keep or tempfile.mkdtemp(prefix="approach_isa_")
    os.makedirs(tmp, exist_ok=True)
    out = {"walks": {}, "loops": {}, "kernels": {}}
    try:
        for unit in units:
            asm = os.path.join(tmp, unit + ".s")
            compile_unit(tree, unit, asm, dev)
            ks = parse(asm)
            names = demangle(sorted(ks))
            out["kernels"][unit] = {}
            for mangled, k in ks.items():
                nice = re.sub(r"\((vp::)?(fast::)?SceneDev.*$|\(.*$", "", re.sub(r"^void ", "", names[mangled]))
                nice = re.sub(r"\s+>", ">", nice.replace("vp::fast::", "").replace("vp::", ""))
                out["kernels"][unit][nice] = [sum(is_vector(mn) for mn, _ in k["insts"]), k.get("vgpr", -1), k["occupancy"], k.get("scratch", 0)]
                if unit == UNITS[0]:
                    for short, full in WALKS:
                        if nice == full:
                            loops = sorted(v for _, _, v in innermost_loops(k))
                            out["loops"][short] = loops
                            out["walks"][short] = loops[-1] / walk_unroll(tree) if loops else None
    finally:
        if not keep:
            shutil.rmtree(tmp, ignore_errors=True)
    return out


def recorded_parent():
    """The parent's walk-loop counts from the record: lines `  <kernel> ... parent N`."""
    walks = {}
    if os.path.exists(RECORD):
        for line in open(RECORD):
            m = re.match(r"^\s*walk loop of (\w+)\s.*?parent\s+(\d+(?:\.\d+)?)\b", line)
            if m:
                walks[m.group(1)] = float(m.group(2))
    return walks


def fmt(v):
    return "-" if v is None else ("%g" % v)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", help="a checkout of the parent commit: compiled in the same run")
    ap.add_argument("--dev", action="store_true", help="-DVP_DEV_BUILD: the bench workloads' kernels only (faster)")
    ap.add_argument("--exact-only", action="store_true", help="the exact unit alone (the walk loops are counted there)")
    ap.add_argument("--json", action="store_true", help="one JSON object instead of the table")
    ap.add_argument("--keep", help="keep this build's assembly in DIR")
    a = ap.parse_args()
    units = UNITS[:1] if a.exact_only else UNITS
    new = figures(ROOT, a.dev, a.keep, units)
    if a.parent:
        par = figures(os.path.abspath(a.parent), a.dev, None, units)
        src = "compiled from " + a.parent
    else:
        par = {"walks": recorded_parent(), "loops": {}, "kernels": {}}
        src = "recorded in profiles/experiments/approach_step.txt"
    if a.json:
        print(json.dumps({"parent": par, "new": new, "parent_source": src}))
        return 0
    print("STATIC FIGURES (Makefile flags%s, hipcc -S --cuda-device-only; gfx950; parent: %s)" % (", -DVP_DEV_BUILD" if a.dev else "", src))
    print("vector instructions per free-flight step (innermost loops of the kernel: v-insts per iteration)")
    for short, full in WALKS:
        print("  walk loop of %-22s %-44s parent %-6s this build %-6s  loops: parent %s  this build %s"
              % (short, full, fmt(par["walks"].get(short)), fmt(new["walks"].get(short)), par["loops"].get(short, "-"), new["loops"].get(short)))
    for unit in units:
        nk, pk = new["kernels"][unit], par["kernels"].get(unit, {})
        print("%s.hip: %d kernels   (v-insts / VGPR / occupancy / scratch bytes per lane)" % (unit, len(nk)))
        for name in sorted(nk):
            n, p = nk[name], pk.get(name)
            mark = "" if p is None or p == n else ("   <-- occupancy or scratch moved" if p[2:] != n[2:] else "   *")
            print("  %-110s %-24s %-24s%s" % (name[:110], "-" if p is None else "%d / %d / %d / %d" % tuple(p), "%d / %d / %d / %d" % tuple(n), mark))
        gone = sorted(set(pk) - set(nk))
        if gone:
            print("  only in the parent: " + ", ".join(gone))
    return 0


if __name__ == "__main__":
    sys.exit(main())
