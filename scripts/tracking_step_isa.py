#!/usr/bin/env python3
"""Static figures of render_k's tracking step (profiles/experiments/fast_state_masks.txt).

Compiles the exact unit to gfx950 assembly with the Makefile's flags (no GPU needed) and prints, for the instance BASELINE
config 2 runs -- render_k<0, RngPhiloxR<7>, true, false, 0, true, false, 0, false...>: global majorant, achromatic, Philox2x32-7 --
  - the vector instructions between consecutive cell loads (global_load_dwordx2: the eight texels of a uchar cell are one load) of
    the tracking loop's unrolled steps, and the scalar instructions beside them,
  - the kernel's vector and scalar registers, occupancy and scratch,
parent against this build.  The parent comes from a checkout given with --parent (compiled in the same run) or from assembly
kept by an earlier run (--parent-asm).  The count is static: every instruction between two loads, the end-of-flight branch that few
steps take included; what a fetching step executes is read from the assembly (profiles/experiments/fast_state_masks.txt).

The copies are found by their shape, not by what they contain: the cell loads of the kernel in layout order, and among the gaps
between consecutive ones the VP_STEPS_PER_PASS - 1 that lie inside one loop iteration, i.e. the most frequent gap length (the
unrolled copies are the same code).  The script counts opcodes by their first letters (v_ / s_); it searches for nothing else.

  python scripts/tracking_step_isa.py [--parent DIR | --parent-asm FILE] [--asm FILE] [--full] [--keep DIR]
"""
import argparse
import collections
import os
import re
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import approach_step_isa as isa   # noqa: E402  (the compile line, the assembly parser and the demangler)

ROOT = isa.ROOT
INSTANCE = re.compile(r"render_k<0, (vp::)?RngPhiloxR<7>, true, false, 0, true, false, 0(, false)*>")
CELL_LOAD = "global_load_dwordx2"

def step_figures(asm):
    ks = isa.parse(asm)
    names = isa.demangle(sorted(ks))
    hits = [m for m in ks if INSTANCE.search(names[m])]
    if len(hits) != 1:
        raise RuntimeError("expected one instance of BASELINE config 2, found %d" % len(hits))
    k = ks[hits[0]]
    insts = k["insts"]
    loads = [j for j, (mn, _) in enumerate(insts) if mn == CELL_LOAD]
    firsts = loads
    gaps = []
    for a, b in zip(firsts, firsts[1:]):
        v = sum(1 for mn, _ in insts[a:b] if mn.startswith("v_"))
        s = sum(1 for mn, _ in insts[a:b] if mn.startswith("s_"))
        gaps.append((v, s))
    common = collections.Counter(v for v, _ in gaps).most_common(1)[0] if gaps else (None, 0)
    return {"name": names[hits[0]][:100], "fetches": len(firsts), "gaps": gaps, "per_copy": common[0], "copies": common[1],
            "scalar_per_copy": [s for v, s in gaps if v == common[0]][:1],
            "vinsts": sum(1 for mn, _ in insts if mn.startswith("v_")), "vgpr": k.get("vgpr"), "occupancy": k["occupancy"],
            "scratch": k.get("scratch", 0)}


def compiled(tree, dev, keep):
    tmp = keep or tempfile.mkdtemp(prefix="tracking_isa_")
    os.makedirs(tmp, exist_ok=True)
    asm = os.path.join(tmp, "vp_kernels.s")
    isa.compile_unit(tree, "vp_kernels", asm, dev)
    return asm


def show(tag, f):
    print("%-10s %s" % (tag, f["name"]))
    print("           fetches in the kernel %d; vector (scalar) instructions between consecutive ones: %s"
          % (f["fetches"], " ".join("%d(%d)" % g for g in f["gaps"])))
    print("           per unrolled copy: %s vector instructions (%d equal gaps), %s scalar"
          % (f["per_copy"], f["copies"], f["scalar_per_copy"][0] if f["scalar_per_copy"] else "-"))
    print("           kernel: %d vector instructions, %s VGPR, occupancy %d, scratch %d" % (f["vinsts"], f["vgpr"], f["occupancy"], f["scratch"]))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", help="a checkout of the parent commit: compiled in the same run")
    ap.add_argument("--parent-asm", help="the parent's assembly of csrc/vp_kernels.hip, kept by an earlier run")
    ap.add_argument("--asm", help="this build's assembly, kept by an earlier run (default: compile)")
    ap.add_argument("--full", action="store_true", help="every instance (default: -DVP_DEV_BUILD, the bench workloads' kernels: faster)")
    ap.add_argument("--keep", help="keep this build's assembly in DIR")
    a = ap.parse_args()
    print("TRACKING STEP, STATIC (Makefile flags%s, hipcc -S --cuda-device-only; gfx950)" % ("" if a.full else ", -DVP_DEV_BUILD"))
    par = a.parent_asm or (compiled(os.path.abspath(a.parent), not a.full, None) if a.parent else None)
    if par:
        show("parent", step_figures(par))
    show("this build", step_figures(a.asm or compiled(ROOT, not a.full, a.keep)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
