"""registers, scratch and occupancy of the binary16 kernel instances beside their float twins, and of every other kernel against another
checkout (no GPU needed):

    python scripts/half_volume_resources.py [--parent DIR_OF_ANOTHER_CHECKOUT] [--log FILE ...] [--parent-log FILE ...] [--groups | --group-layers | --list REGEX]

Compiles csrc/vp_kernels.hip and csrc/vp_kernels_fast.hip for gfx950 with -Rpass-analysis=kernel-resource-usage (minutes), or reads
the remarks of such a compilation from --log / --parent-log.  A binary16 instance is one whose last template argument, HALF, is true;
its twin is the same instance with HALF false.  Instances of the other checkout are matched by name with a trailing `false` dropped
(render_k, danger_k, opacity_k and test_density_k gained the HALF argument)."""
import argparse
import collections
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-fast-math",
         "-fno-slp-vectorize", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"]
KEYS = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]")


def remarks(root):
    pkg = os.path.join(root, "cuda-volpath_amd")
    procs = [subprocess.Popen(["/opt/rocm/bin/hipcc", *FLAGS, "-c", "csrc/" + f, "-o", os.path.join(tempfile.gettempdir(), f + ".kres.o")], cwd=pkg,
                              stderr=subprocess.PIPE, text=True) for f in ("vp_kernels.hip", "vp_kernels_fast.hip")]
    return "".join(p.communicate()[1] for p in procs)


def parse(text):
    rows, cur = collections.OrderedDict(), None
    for line in text.splitlines():
        m = re.search(r"remark:\s+(.*?) \[-Rpass", line)
        if not m:
            continue
        t = m.group(1).strip()
        if t.startswith("Function Name:"):
            cur = rows.setdefault(t.split(":", 1)[1].strip(), {})
        elif cur is not None and ":" in t:
            k, v = t.rsplit(":", 1)
            cur[k.strip()] = v.strip()
    names = list(rows)
    plain = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    out = collections.OrderedDict()
    for n, d in zip(names, plain):
        d = re.sub(r"^void ", "", d).replace("vp::", "")
        depth = 0
        for i in range(len(d) - 1, -1, -1):          # drop the argument list
            depth += (d[i] == ")") - (d[i] == "(")
            if d[i] == "(" and depth == 0:
                d = d[:i]
                break
        # render_k's twelfth argument (LYR: a layers instance) is not part of the name here, so that HALF
        # stays the last one: a plain instance drops it, a layers instance is listed as render_k[layers]<...>
        # (the thirteenth, GRP: a light-groups instance, section 2.7, likewise -- render_k[groups]<...>)
        # (both, a group-layers instance, section 2.10: render_k[group-layers]<...>)
        if "render_k<" in d and d.count(",") == 12:
            d, grp = d.rsplit(", ", 1)
            d = (d if grp == "false>" else d.replace("render_k<", "render_k[groups]<")) + ">"
        if "render_k" in d and d.count(",") == 11:
            d, lyr = d.rsplit(", ", 1)
            if lyr != "false>":
                d = d.replace("render_k[groups]<", "render_k[group-layers]<") if "render_k[groups]<" in d else d.replace("render_k<", "render_k[layers]<")
            d += ">"
        out[d] = rows[n]
    return out


def fmt(v):
    return "VGPR %3s SGPR %3s spill s/v %s/%s scratch %s occ %s LDS %s" % (v["VGPRs"], v["TotalSGPRs"], v["SGPRs Spill"], v["VGPRs Spill"],
                                                                        v["ScratchSize [bytes/lane]"], v["Occupancy [waves/SIMD]"], v["LDS Size [bytes/block]"])


ap = argparse.ArgumentParser()
ap.add_argument("--parent", default=None)
ap.add_argument("--log", nargs="*", default=None)
ap.add_argument("--parent-log", nargs="*", default=None)
ap.add_argument("--groups", action="store_true", help="list the light-groups instances of render_k beside their plain twins instead of the binary16 ones")
ap.add_argument("--list", default=None, metavar="REGEX", help="list the kernels whose name matches instead (e.g. 'reduce_': the add-kernels of a staged launch)")
ap.add_argument("--group-layers", action="store_true", help="list the group-layers instances of render_k beside their groups and layers siblings")
a = ap.parse_args()
new = parse("".join(open(f, errors="replace").read() for f in a.log) if a.log else remarks(ROOT))
old = None
if a.parent_log or a.parent:
    old = parse("".join(open(f, errors="replace").read() for f in a.parent_log) if a.parent_log else remarks(a.parent))
half = [n for n in new if re.search(r", true>$", n) and re.sub(r", true>$", ", false>", n) in new and ("render_k" in n or re.search(r"_k<false, true>$", n))]
print(f"# {len(new)} kernels" + (f" ({len(old)} in the other checkout)" if old else "") + f", {len(half)} binary16 instances")
if old:
    changed = 0
    for n, v in new.items():
        o = old.get(n) or old.get(re.sub(r", false>$", ">", n))
        if o is not None and any(o.get(k) != v.get(k) for k in KEYS):
            changed += 1
            print("# CHANGED", n, "|", fmt(o), "->", fmt(v))
    print(f"# instances of the other checkout whose registers, spills, scratch, occupancy or LDS changed: {changed}")
if a.list:
    hits = [n for n in new if re.search(a.list, n)]
    for n in hits:
        print(f"{n} | {fmt(new[n])}" + ("" if old is None or n in old else "   NEW"))
    spills = sum(int(new[n]["ScratchSize [bytes/lane]"]) > 0 or int(new[n]["VGPRs Spill"]) > 0 or int(new[n]["SGPRs Spill"]) > 0 for n in hits)
    print(f"# {len(hits)} kernels match {a.list!r}; with scratch or spills: {spills}")
    raise SystemExit(0)
if a.groups:
    short = lambda v: "VGPR %3s SGPR %3s spill %s/%s scratch %s occ %s" % (v["VGPRs"], v["TotalSGPRs"], v["SGPRs Spill"], v["VGPRs Spill"], v["ScratchSize [bytes/lane]"],
                                                                           v["Occupancy [waves/SIMD]"])
    grp = [n for n in new if n.startswith("render_k[groups]<")]
    more = lower = 0
    for n in grp:
        v, t = new[n], new[n.replace("render_k[groups]<", "render_k<")]
        more += int(v["VGPRs"]) > int(t["VGPRs"]) or int(v["ScratchSize [bytes/lane]"]) > int(t["ScratchSize [bytes/lane]"])
        lower += int(v["Occupancy [waves/SIMD]"]) < int(t["Occupancy [waves/SIMD]"])
        print(f"{n} | {short(v)} | plain twin {short(t)}")
    print(f"# {len(grp)} groups instances; with more registers or scratch than the plain twin: {more}; with a lower occupancy: {lower}")
    raise SystemExit(0)
if a.group_layers:
    short = lambda v: "VGPR %3s SGPR %3s spill %s/%s scratch %s occ %s" % (v["VGPRs"], v["TotalSGPRs"], v["SGPRs Spill"], v["VGPRs Spill"], v["ScratchSize [bytes/lane]"],
                                                                           v["Occupancy [waves/SIMD]"])
    both = [n for n in new if n.startswith("render_k[group-layers]<")]
    spills = lower = more = 0
    for n in both:
        v, g, l = new[n], new[n.replace("[group-layers]", "[groups]")], new[n.replace("[group-layers]", "[layers]")]
        spills += int(v["ScratchSize [bytes/lane]"]) > 0 or int(v["VGPRs Spill"]) > 0 or int(v["SGPRs Spill"]) > 0
        lower += int(v["Occupancy [waves/SIMD]"]) < int(g["Occupancy [waves/SIMD]"])
        more += int(v["VGPRs"]) > int(g["VGPRs"])
        print(f"{n} | {short(v)} | groups sibling {short(g)} | layers sibling {short(l)}")
    print(f"# {len(both)} group-layers instances; with scratch or spills: {spills}; with a lower occupancy than the groups sibling: {lower}; with more VGPRs than it: {more}")
    raise SystemExit(0)
more, occ = 0, 0
for n in half:
    v, t = new[n], new[re.sub(r", true>$", ", false>", n)]
    worse = int(v["VGPRs"]) > int(t["VGPRs"]) or int(v["ScratchSize [bytes/lane]"]) > int(t["ScratchSize [bytes/lane]"]) or int(v["VGPRs Spill"]) > int(t["VGPRs Spill"])
    more += worse
    occ += int(v["Occupancy [waves/SIMD]"]) < int(t["Occupancy [waves/SIMD]"])
    print(f"{n} {fmt(v)} | float twin {fmt(t)}" + ("   MORE" if worse else ""))
print(f"# binary16 instances with more registers, scratch or spills than the float twin: {more} of {len(half)}; with a lower occupancy: {occ}")
