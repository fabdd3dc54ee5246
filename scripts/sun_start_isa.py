#!/usr/bin/env python3
"""Static figures of the sun shadow ray's start in render_k's collision block (profiles/experiments/sun_start_constants.txt).

Compiles the integrator's units to gfx950 assembly with the Makefile's flags and -Rpass-analysis=kernel-resource-usage (no GPU
needed) and prints, parent against this build,
  - for the C2, c3ref and C3 instances of the exact unit: the vector instructions of the collision block from its entry to the hit
    test of the sun ray's box test, with the v_div_scale / v_sqrt / v_rcp among them -- all of them (the static count) and along
    the cheapest and the dearest way through the region's wave-uniform branches (every operand constant / none);
  - for every render_k instance of both units: VGPRs, spills (SGPR + VGPR), scratch, LDS bytes and occupancy from the remarks;
    instances whose occupancy fell or whose spills or scratch grew are marked, and so are those whose occupancy rose.

The region is found by shape.  hg_eval_row's constant 4 pi (0x41490fdb) occurs once in an instance with the collision tables, in
the collision block before the shadow ray starts; the two sched_barriers behind it in layout order are the sun ray's box test
(intersect_box / sun_start, axis by axis).  The region runs from the last write of exec before the constant (the block's entry:
`st == EV_SCATTER`) to the first write of exec behind the second barrier (the hit test).  The shadow state's stores behind the hit
test are moves and LDS writes that this change does not touch; they are not counted.  The wave-uniform branches between the two
bounds make a graph without loops whose blocks may lie anywhere in the kernel: the cheapest and dearest ways are its shortest and
longest paths by vector instructions, the static count is that of every block on some way.  On the sun bench.py renders with a
wave takes the cheapest way plus one division (x): 11 vector instructions, 2 v_div_scale and 1 v_rcp more.

  python scripts/sun_start_isa.py --parent DIR [--dev] [--keep DIR [--reuse]]
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import approach_step_isa as A   # noqa: E402  (the Makefile's flags, the demangler)

ROOT = A.ROOT
INSTANCES = (("C2", "render_k<0, RngPhiloxR<7>, true, false, 0, true, false, 0, false, false, false, false>"),
             ("c3ref", "render_k<1, RngPhiloxR<7>, true, false, 0, true, false, 0, false, false, false, false>"),
             ("C3", "render_k<1, RngPhiloxR<7>, true, false, 2, true, false, 0, false, false, false, false>"))
FOUR_PI = "0x41490fdb"
DEAR = ("v_div_scale", "v_sqrt", "v_rcp")


def compile_unit(tree, unit, out, dev, reuse=False):
    """assembly to `out`, the resource-usage remarks (kept beside it) returned as text"""
    if reuse and os.path.exists(out) and os.path.exists(out + ".remarks"):
        return open(out + ".remarks").read()
    hipcc, flags = A.makefile_flags(tree)
    cmd = [hipcc] + flags + (["-DVP_DEV_BUILD"] if dev else []) + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                                                                   os.path.join("csrc", unit + ".hip"), "-o", out]
    r = subprocess.run(cmd, cwd=os.path.join(tree, A.PKG), stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    if r.returncode:
        sys.stderr.write(r.stderr[-4000:])
        raise RuntimeError("compilation failed: " + unit)
    open(out + ".remarks", "w").write(r.stderr)
    return r.stderr


def nice(name):
    name = re.sub(r"\((vp::)?(fast::)?SceneDev.*$|\(.*$", "", re.sub(r"^void ", "", name))
    return re.sub(r"\s+>", ">", name.replace("vp::fast::", "").replace("vp::", ""))


def resources(remarks):
    """{demangled kernel: dict(vgpr, spill, scratch, lds, occupancy)} from the remarks"""
    out, cur = {}, None
    keys = {"VGPRs": "vgpr", "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "occupancy", "SGPRs Spill": "sspill", "VGPRs Spill": "vspill",
            "LDS Size [bytes/block]": "lds"}
    for line in remarks.split("\n"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z /\[\]]+): (\d+)", line)
        if m and cur is not None and m.group(1).strip() in keys:
            cur[keys[m.group(1).strip()]] = int(m.group(2))
    names = A.demangle(sorted(out))
    return dict((nice(names[k]), v) for k, v in out.items())


def kernel_text(path, mangled):
    lines, take = [], False
    for line in open(path):
        if line.startswith(mangled + ":"):
            take = True
            continue
        if take:
            if line.startswith(".Lfunc_end"):
                break
            lines.append(line.rstrip("\n"))
    return lines


def mangled_names(path):
    names = [m.group(1) for m in (re.match(r"^(_Z\w+):\s*; @", l) for l in open(path)) if m]
    return A.demangle(names)


def writes_exec(mn, ops):
    return "saveexec" in mn or (mn.startswith("s_") and ops.split(",")[0].strip() == "exec")


def region(lines):
    """(instructions [(mnemonic, operands)], labels {label: index}, first, last): the kernel and the bounds of the sun ray's start in
    it, or None where the shape is not found"""
    insts, labels = [], {}
    for l in lines:
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            labels[m.group(1)] = len(insts)
            continue
        if "; sched_barrier" in l:
            insts.append(("sched_barrier", ""))
            continue
        if l.startswith("\t") and not l.startswith("\t.") and not l.startswith("\t;"):
            parts = l.split(";")[0].split(None, 1)
            if parts:
                insts.append((parts[0], parts[1].strip() if len(parts) > 1 else ""))
    at = [i for i, (mn, ops) in enumerate(insts) if FOUR_PI in ops.lower()]
    if len(at) != 1:
        return None
    bars = [i for i in range(at[0], len(insts)) if insts[i][0] == "sched_barrier"][:2]
    if len(bars) < 2:
        return None
    first = max(i for i in range(at[0]) if writes_exec(*insts[i])) + 1
    last = min(i for i in range(bars[1], len(insts)) if writes_exec(*insts[i]))
    return insts, labels, first, last


def paths(found):
    """(static, cheapest, dearest): each (v-insts, (div_scale, sqrt, rcp)).  The ways from `first` to `last` through the kernel's
    control-flow graph -- a general sequence may be laid out anywhere, the end of the function included -- by vector instructions;
    static: the instructions of every block that lies on such a way."""
    insts, labels, first, last = found
    leaders = sorted({0, first, last} | set(labels.values()) |
                     {j + 1 for j, (mn, _) in enumerate(insts) if mn.startswith("s_cbranch") or mn in ("s_branch", "s_endpgm", "s_setpc_b64")})
    leaders = [x for x in leaders if x < len(insts)]
    nxt_leader = dict(zip(leaders, leaders[1:] + [len(insts)]))
    zero = (0, (0, 0, 0))
    add = lambda a, b: (a[0] + b[0], tuple(a[1][k] + b[1][k] for k in range(3)))
    per = dict((b, (sum(mn.startswith("v_") for mn, _ in insts[b:nxt_leader[b]]),
                    tuple(sum(mn.startswith(p) for mn, _ in insts[b:nxt_leader[b]]) for p in DEAR))) for b in leaders)
    memo, active, used = {}, set(), set()

    def succ(b):
        mn, ops = insts[nxt_leader[b] - 1]
        # every lane of the region is active: s_cbranch_execnz is taken, s_cbranch_execz is not
        out = []
        if mn == "s_branch" or mn == "s_cbranch_execnz" or (mn.startswith("s_cbranch") and mn != "s_cbranch_execz"):
            t = labels.get(ops.split()[0])
            if t is not None:
                out.append(t)
        if mn not in ("s_branch", "s_cbranch_execnz", "s_endpgm", "s_setpc_b64") and nxt_leader[b] < len(insts):
            out.append(nxt_leader[b])
        return out

    def ways(b):
        if b == last:
            return (zero, zero)
        if b in memo:
            return memo[b]
        if b in active:
            return None   # a way back into the kernel's loop: not a way to the hit test
        active.add(b)
        nxt = [w for w in (ways(t) for t in succ(b)) if w is not None]
        active.discard(b)
        memo[b] = (add(per[b], min((w[0] for w in nxt), key=lambda x: x[0])), add(per[b], max((w[1] for w in nxt), key=lambda x: x[0]))) if nxt else None
        if memo[b]:
            used.add(b)
        return memo[b]

    w = ways(first)
    if w is None:
        return None
    static = zero
    for b in used:
        static = add(static, per[b])
    return static, w[0], w[1]


def figures(tree, dev, keep, tag, reuse=False):
    tmp = keep or tempfile.mkdtemp(prefix="sun_start_isa_")
    os.makedirs(tmp, exist_ok=True)
    out = {"region": {}, "resources": {}}
    for unit in A.UNITS:
        asm = os.path.join(tmp, "%s_%s.s" % (tag, unit))
        out["resources"][unit] = dict((k, v) for k, v in resources(compile_unit(tree, unit, asm, dev, reuse)).items() if k.startswith("render_k<"))
        if unit == A.UNITS[0]:
            names = mangled_names(asm)
            for short, full in INSTANCES:
                hit = [m for m, d in names.items() if nice(d) == full]
                found = region(kernel_text(asm, hit[0])) if hit else None
                out["region"][short] = paths(found) if found else None
    return out


def fmt_region(r):
    if r is None:
        return "not found"
    return "   ".join("%s %d v-insts (%d div_scale, %d sqrt, %d rcp)" % (what, x[0], x[1][0], x[1][1], x[1][2]) for what, x in zip(("static", "cheapest way", "dearest way"), r))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", required=True, help="a checkout of the parent commit: compiled in the same run")
    ap.add_argument("--dev", action="store_true", help="-DVP_DEV_BUILD: the bench workloads' kernels only (faster)")
    ap.add_argument("--keep", help="keep the assembly in DIR")
    ap.add_argument("--reuse", action="store_true", help="with --keep: take the assembly and remarks already in DIR instead of compiling")
    a = ap.parse_args()
    sys.setrecursionlimit(20000)   # (the walk through the control-flow graph is recursive)
    par = figures(os.path.abspath(a.parent), a.dev, a.keep, "parent", a.reuse and bool(a.keep))
    new = figures(ROOT, a.dev, a.keep, "new", a.reuse and bool(a.keep))
    print("STATIC FIGURES (Makefile flags%s, hipcc -S --cuda-device-only -Rpass-analysis=kernel-resource-usage; gfx950)" % (", -DVP_DEV_BUILD" if a.dev else ""))
    print("collision block, entry to the hit test of the sun ray's box test (exact unit)")
    for short, full in INSTANCES:
        print("  %-6s %s" % (short, full))
        print("         parent      %s" % fmt_region(par["region"].get(short)))
        print("         this build  %s" % fmt_region(new["region"].get(short)))
    worse = gained = 0
    for unit in A.UNITS:
        nk, pk = new["resources"][unit], par["resources"][unit]
        print("%s.hip: %d render_k instances   (VGPRs / spills / scratch bytes per lane / LDS bytes / occupancy)" % (unit, len(nk)))
        for name in sorted(nk):
            n, p = nk[name], pk.get(name)
            f = lambda r: "-" if r is None else "%d / %d / %d / %d / %d" % (r["vgpr"], r["sspill"] + r["vspill"], r["scratch"], r["lds"], r["occupancy"])
            bad = p is not None and (n["occupancy"] < p["occupancy"] or n["sspill"] + n["vspill"] > p["sspill"] + p["vspill"] or n["scratch"] > p["scratch"])
            more = p is not None and n["occupancy"] > p["occupancy"]
            worse += bad
            gained += more
            print("  %-104s %-28s %-28s%s" % (name[:104], f(p), f(n), "   <-- LOST A WAVE OR GAINED A SPILL" if bad else
                                              ("   <-- RUNS ONE MORE WAVE" if more else ("" if p == n else "   *"))))
        gone = sorted(set(pk) - set(nk))
        if gone:
            print("  only in the parent: " + ", ".join(gone))
    print("instances that lost a wave or gained a spill or scratch: %d" % worse)
    print("instances whose occupancy rose (nothing but registers may have held them where they were: check what the host launches): %d" % gained)
    missing = [short for short, _ in INSTANCES for side in (par, new) if side["region"].get(short) is None]
    if missing:
        print("the region was NOT FOUND in: " + ", ".join(sorted(set(missing))) + " -- the figures above are incomplete")
        return 2
    return 1 if worse else 0


if __name__ == "__main__":
    sys.exit(main())
