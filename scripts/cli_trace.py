#!/usr/bin/env python3
"""cli_trace.py -- a CPU-only differential of the volpath_render driver (cuda-volpath_amd/host/main.cpp) against another revision of it.

    python scripts/cli_trace.py [--rev HEAD] [--out profiles/experiments/cli_refactor_trace.txt] [--jobs 8] [--keep DIR]

It builds scripts/cli_trace_stub.c as a stand-in libvolpath_hip.so (every library call logs its name and arguments and fills what it
writes from a hash of them; no GPU), builds volpath_render twice against it -- from the working tree's host/main.cpp and from
`git show REV:cuda-volpath_amd/host/main.cpp`, each in a scratch directory of its own whose $ORIGIN rpath finds the stub and the real
libvolpath_host.so -- and runs both over a generated matrix of command lines at --julia 8 --size 16 8 --spp 4:

  * every flag alone, with valid operands and, once each, an invalid or a missing one;
  * every unordered pair of the mode flags (MODE below);
  * the README's command lines, scaled down (a tiny cloud.bin is written for the --bin ones);
  * every command line the CPU tests named test_cli_* give to volpath_render (recorded by running them with this file as a pytest
    plugin that notes subprocess.run's argv), with the scale-down flags in front.

Per command line it compares the exit status, stderr, stdout (the numbers of the two timing lines and the process id in RCCL's own
messages masked), the call log and every file written.  The call log is compared after one normalisation: a device buffer is named by its first use in a call other than vp_malloc /
vp_memset / vp_free instead of by the ordinal of its vp_malloc, and each block of consecutive vp_malloc / vp_memset / vp_free lines is
sorted -- the ORDER in which neighbouring buffers are allocated, zeroed and freed is not behaviour; which buffers, their sizes, what is
zeroed, where the block stands among the other calls and every operand of every other call are.  The count of command lines whose raw
logs differ is reported beside it.

Not covered: distinct-device --gpus (the RCCL path needs devices) and --rccl-selftest."""
import argparse
import hashlib
import itertools
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AMD = os.path.join(ROOT, "cuda-volpath_amd")
MAIN = "cuda-volpath_amd/host/main.cpp"
SMALL = ["--julia", "8", "--size", "16", "8", "--spp", "4"]

# the mode flags, each with valid operands
MODE = [["--noise", "0.5"], ["--noise-out", "n.hdr"], ["--denoise"], ["--denoise-features"], ["--denoise-cross"], ["--resid-out", "r.hdr"],
        ["--denoise-var"], ["--var-out", "v.hdr"],
        ["--denoise-select"], ["--select-out", "s.hdr"],
        ["--layers-out", "L"], ["--over", "0.1", "0.2", "0.3"], ["--layers-denoise"], ["--groups-out", "G"], ["--sun-gain", "1.5", "1", "0.5"],
        ["--sky-gain", "0.5", "1", "2"], ["--groups-denoise"], ["--plane-noise", "0.5", "0.25"], ["--plane-noise-out", "N"], ["--planes-out", "P"],
        ["--planes-denoise"], ["--planes-noise", "0.5", "0.25", "0.1"], ["--planes-noise-out", "M"], ["--features-out", "F"], ["--aa", "2"],
        ["--batch", "2"], ["--spp", "16"], ["--gpus", "2", "--devices", "0,0"], ["--arith", "fast", "--rng", "philox"], ["--tracking", "scalar"],
        ["--env", "mis"], ["--estimator", "global"], ["--out", "x.hdr"]]
# the other flags, each with valid operands
OTHER = [["--julia", "6"], ["--bin", "cloud.bin"], ["--bin", "missing.bin"], ["--vdb", "missing.vdb"], ["--volume-format", "f32"], ["--volume-format", "u8"],
         ["--bin", "cloud.bin", "--volume-format", "f16"], ["--size", "9", "7"], ["--spp", "12"], ["--preset", "3"], ["--density", "200"], ["--g", "0.3"],
         ["--estimator", "bounded"], ["--estimator", "decomp"], ["--brick", "4"], ["--rng", "philox7"], ["--rng", "samplerh"], ["--tracking", "multichannel"],
         ["--env", "passive"], ["--arith", "exact"], ["--aa", "1"], ["--aa", "4"], ["--aa", "8"], ["--min-spp", "2"], ["--round", "1"], ["--denoise-radius", "3"],
         ["--denoise-patch", "2"], ["--denoise-k", "0.3"], ["--denoise-var-radius", "2"], ["--denoise-var-patch", "1"], ["--denoise-var-k", "0.3"], ["--denoise-select-radius", "4"], ["--denoise-select-patch", "2"], ["--denoise-select-smooth", "2"], ["--denoise-select-blend", "0"], ["--denoise-sigma-alpha", "0.5"], ["--denoise-sigma-depth", "0.5"], ["--feature-step", "0.01"],
         ["--depth-tau", "1.5"], ["--sun", "0.3", "0.4"], ["--batch", "3"], ["--out", "x.ppm"], ["--gpus", "3", "--devices", "0,0,0"], ["--devices", "1"],
         ["--help"]]
# invalid operands, once each; quirks: an unknown --estimator, --rng, --tracking or --env value silently means the default
INVALID = [["--noise", "-1"], ["--noise", "x"], ["--noise", "nan"], ["--plane-noise", "0.5", "-1"], ["--plane-noise", "0.5"], ["--planes-noise", "0.1", "0.1", "nan"],
           ["--planes-noise", "0.1", "0.1", "--planes-out"], ["--over", "1", "2", "inf"], ["--over", "1", "2"], ["--sun-gain", "a", "b", "c"], ["--sky-gain", "1", "1", "1e99"],
           ["--denoise-radius", "11"], ["--denoise-radius", "-1"], ["--denoise-patch", "4"], ["--denoise-k", "0"], ["--denoise-k", "inf"], ["--denoise-var-radius", "11"], ["--denoise-var-patch", "4"], ["--denoise-var-k", "0"], ["--denoise-select-radius", "11"], ["--denoise-select-patch", "4"], ["--denoise-select-smooth", "4"], ["--denoise-select-blend", "-1"],
           ["--denoise-sigma-alpha", "0"], ["--denoise-sigma-depth", "-1"], ["--feature-step", "0"], ["--depth-tau", "nan"], ["--aa", "3"], ["--arith", "quick"],
           ["--volume-format", "u16"], ["--estimator", "best"], ["--rng", "mt"], ["--tracking", "ratio"], ["--env", "both"], ["--preset", "13"], ["--gpus", "0"],
           ["--gpus", "2"], ["--gpus", "2", "--devices", "0"], ["--bogus"], ["--noise", "0.5", "--min-spp", "1"], ["--noise", "0.5", "--round", "0"],
           ["--layers-out", "L", "--plane-noise", "0.5", "0.5", "--min-spp", "1"], ["--planes-out", "P", "--planes-noise", "0.5", "0.5", "0.5", "--round", "0"],
           ["--arith", "fast"], ["--arith", "fast", "--rng", "philox", "--estimator", "bounded"]]
# triples and longer: the documented modes whose flags only work together
TOGETHER = [["--layers-out", "L", "--over", "0.1", "0.2", "0.3", "--plane-noise", "0.5", "0.25", "--plane-noise-out", "N", "--spp", "16", "--min-spp", "4", "--round", "4"],
            ["--groups-out", "G", "--plane-noise", "0.5", "0.25", "--plane-noise-out", "N", "--groups-denoise"],
            ["--over", "0", "0", "0", "--layers-denoise", "--plane-noise", "0.5", "0.25"],
            ["--planes-out", "P", "--planes-noise", "0.5", "0.25", "0.1", "--planes-noise-out", "M", "--sun-gain", "1.5", "1", "0.5", "--over", "0.1", "0.2", "0.3"],
            ["--planes-out", "P", "--planes-noise", "0.5", "0.25", "0.1", "--planes-denoise", "--out", "x.hdr"],
            ["--noise", "0.5", "--denoise", "--noise-out", "n.hdr", "--spp", "16"], ["--noise", "0.5", "--denoise", "--denoise-features", "--estimator", "global"],
            ["--denoise-cross", "--denoise-features", "--resid-out", "r.hdr", "--batch", "3", "--spp", "12"],
            ["--denoise-cross", "--denoise-features", "--aa", "2"], ["--denoise-cross", "--aa", "2", "--out", "x.hdr"],
            ["--gpus", "2", "--devices", "0,0", "--features-out", "F", "--aa", "2", "--spp", "14"], ["--spp", "14"], ["--spp", "14", "--batch", "5"],
            ["--bin", "cloud.bin", "--volume-format", "f32", "--gpus", "2", "--devices", "0,0"],
            ["--cross-noise", "0.5", "--cross-noise-out", "c.hdr", "--spp", "16", "--min-spp", "4", "--round", "4"],
            ["--cross-noise", "0.5", "--denoise-select", "--denoise-features", "--spp", "16"], ["--cross-noise", "0.5", "--aa", "2", "--round", "4", "--spp", "16"],
            ["--cross-noise", "0.5", "--noise", "0.5"], ["--cross-noise", "0.5", "--gpus", "2", "--devices", "0,0"], ["--cross-noise", "-1"],
            ["--layers-out", "L", "--layers-denoise-cross", "--plane-cross-noise", "0.5", "0.25", "--plane-cross-noise-out", "N", "--spp", "16"],
            ["--groups-out", "G", "--groups-denoise-cross", "--plane-cross-noise", "0.5", "0.25", "--plane-denoise-var"],
            ["--planes-out", "P", "--planes-denoise-cross", "--planes-cross-noise", "0.5", "0.25", "0.1", "--plane-cross-noise-out", "M", "--spp", "16"],
            ["--planes-out", "P", "--planes-denoise-cross", "--plane-cross-noise", "0.5", "0.25"], ["--planes-out", "P", "--planes-cross-noise", "0.5", "0.25", "0.1"],
            ["--cross-noise", "0.5", "--planes-out", "P", "--planes-denoise-cross"], ["--cross-noise-out", "c.hdr"], ["--plane-cross-noise-out", "N"]]


# ---- the pytest plugin half: note what the test_cli_* tests give to volpath_render
def pytest_configure(config):
    record = os.environ.get("CLI_TRACE_RECORD")
    if not record:
        return
    run = subprocess.run

    def noting(args, *a, **kw):
        if isinstance(args, (list, tuple)) and args and os.path.basename(str(args[0])) == "volpath_render":
            with open(record, "a") as f:
                f.write("\t".join(str(x) for x in args[1:]) + "\n")
        return run(args, *a, **kw)
    subprocess.run = noting


def recorded_lines(tmp):
    record = os.path.join(tmp, "recorded.txt")
    env = dict(os.environ, CLI_TRACE_RECORD=record, PYTHONPATH=os.path.dirname(os.path.abspath(__file__)) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests"), "-m", "not gpu", "-k", "test_cli", "-q", "-p", "cli_trace", "-p", "no:cacheprovider"],
                       cwd=ROOT, env=env, capture_output=True, text=True)
    if not os.path.exists(record):
        raise SystemExit("recording the test_cli_* command lines failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
    lines = [ln.rstrip("\n").split("\t") if ln.strip() else [] for ln in open(record)]
    tail = re.findall(r"\d+ (?:passed|failed|error)", r.stdout)
    return lines, ", ".join(tail) if tail else "?"


def readme_lines():
    out = []
    for ln in open(os.path.join(ROOT, "README.md")):
        if not ln.startswith("cuda-volpath_amd/volpath_render "):
            continue
        args = ln.split("   #")[0].split()[1:]
        small = []
        it = iter(args)
        for a in it:
            if a == "--julia":
                next(it)
                small += ["--julia", "8"]
            elif a == "--size":
                next(it), next(it)
                small += ["--size", "16", "8"]
            elif a in ("--spp", "--batch", "--min-spp", "--round"):
                small += [a, str(min(int(next(it)), {"--spp": 16, "--batch": 3, "--min-spp": 4, "--round": 4}[a]))]
            else:
                small.append(a)
        out.append(small)
    return out


def matrix(tmp):
    lines = [SMALL + f for f in [[]] + MODE + OTHER + INVALID + TOGETHER]
    lines += [SMALL + f[:1] for f in MODE + OTHER if len(f) > 1]                    # the operand is missing
    lines += [SMALL + a + b for a, b in itertools.combinations(MODE, 2)]
    readme = readme_lines()
    rec, tests = recorded_lines(tmp)
    lines += readme + [SMALL + r for r in rec]
    seen, uniq = set(), []
    for ln in lines:
        if tuple(ln) not in seen:
            seen.add(tuple(ln))
            uniq.append(ln)
    return uniq, len(readme), len(rec), tests


# ---- building
def sh(cmd, **kw):
    r = subprocess.run(cmd, capture_output=True, text=True, **kw)
    if r.returncode:
        raise SystemExit("failed: %s\n%s%s" % (" ".join(cmd), r.stdout, r.stderr))
    return r.stdout


def build(tmp, rev):
    host_so = os.path.join(AMD, "libvolpath_host.so")
    if not os.path.exists(host_so):
        sh(["make", "-C", AMD, "libvolpath_host.so"])
    inc = ["-I" + os.path.join(AMD, "host"), "-I" + os.path.join(ROOT, "include")]
    cxx = ["g++", "-O2", "-std=c++17", "-fPIC", "-fopenmp", "-ffp-contract=off"]
    sh(cxx + inc + ["-I/opt/rocm/include", "-Wno-unused-result", "-c", os.path.join(AMD, "host", "multigpu.cpp"), "-o", os.path.join(tmp, "multigpu.o")])
    exes = {}
    for name, text in (("tree", open(os.path.join(ROOT, MAIN)).read()), ("rev", sh(["git", "-C", ROOT, "show", rev + ":" + MAIN]))):
        d = os.path.join(tmp, name)
        os.mkdir(d)
        open(os.path.join(d, "main.cpp"), "w").write(text)
        shutil.copy(host_so, d)
        sh(["cc", "-O2", "-std=c11", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "scripts", "cli_trace_stub.c"), "-o",
            os.path.join(d, "libvolpath_hip.so"), "-lm"])
        sh(cxx + inc + ["-o", os.path.join(d, "volpath_render"), os.path.join(d, "main.cpp"), os.path.join(tmp, "multigpu.o"), "-L" + d, "-lvolpath_host", "-lvolpath_hip",
                        "-L/opt/rocm/lib", "-lamdhip64", "-ldl", "-Wl,-rpath,$ORIGIN", "-Wl,-rpath,/opt/rocm/lib"])
        exes[name] = os.path.join(d, "volpath_render")
    return exes


def cloud_bin(path):
    """a tiny dense volume for the --bin lines, where the host library's own writer is at hand"""
    sys.path.insert(0, AMD)
    try:
        import numpy as np
        from volpath import host
        host.dump_dense(path, np.linspace(0, 1, 6 * 5 * 4, dtype=np.float32).reshape(4, 5, 6))
        return True
    except Exception:
        return False


# ---- running and comparing
MEMORY = ("vp_malloc", "vp_memset", "vp_free")
TIMING = re.compile(r"^\S+ M samples / s(.*), \S+ s$")
RCCL_PID = re.compile(r"^\S+:\d+:\d+ \[")      # RCCL's own messages begin host:pid:tid
RENDERS = re.compile(r"^(render_kernel|vp_render_frames|vp_render_adaptive)", re.M)


def normalise(log):
    lines = log.splitlines()
    names = {}
    for ln in lines:
        if not ln.startswith(MEMORY):
            for d in re.findall(r"\bd\d+\b", ln):
                names.setdefault(d, "b%d" % len(names))
    lines = [re.sub(r"\bd\d+\b", lambda m: names.get(m.group(0), "unused"), ln) for ln in lines]
    out, block = [], []
    for ln in lines + [""]:
        if ln.startswith(MEMORY):
            block.append(ln)
        else:
            out += sorted(block) + [ln]
            block = []
    return "\n".join(out)


def run_one(exe, args, work, cloud):
    os.mkdir(work)
    if cloud:
        shutil.copy(cloud, os.path.join(work, "cloud.bin"))
    log = os.path.join(work, "calls.log")
    try:
        r = subprocess.run([exe] + args, cwd=work, env=dict(os.environ, CLI_TRACE_LOG=log), capture_output=True, text=True, timeout=300)
        status, out, err = r.returncode, r.stdout, r.stderr
    except subprocess.TimeoutExpired:
        status, out, err = "timeout", "", ""
    raw = open(log).read() if os.path.exists(log) else ""
    files = {}
    for n in sorted(os.listdir(work)):
        if n not in ("calls.log", "cloud.bin"):
            files[n] = hashlib.sha256(open(os.path.join(work, n), "rb").read()).hexdigest()
    shutil.rmtree(work)
    out = "\n".join(RCCL_PID.sub("#:#:# [", TIMING.sub(r"# M samples / s\1, # s", ln)) for ln in out.splitlines())
    return dict(status=status, stdout=out, stderr=err, log=normalise(raw), files=files, raw=raw)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rev", default="HEAD")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "experiments", "cli_refactor_trace.txt"))
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--keep", help="scratch directory to build and run in (kept); default: a temporary one")
    a = ap.parse_args()
    tmp = a.keep or tempfile.mkdtemp(prefix="cli_trace_")
    os.makedirs(tmp, exist_ok=True)
    exes = build(tmp, a.rev)
    cloud = os.path.join(tmp, "cloud.bin")
    cloud = cloud if cloud_bin(cloud) else None
    lines, n_readme, n_rec, tests = matrix(tmp)

    def both(job):
        i, args = job
        return args, run_one(exes["tree"], args, os.path.join(tmp, "t%d" % i), cloud), run_one(exes["rev"], args, os.path.join(tmp, "r%d" % i), cloud)
    with ThreadPoolExecutor(a.jobs) as pool:
        results = list(pool.map(both, enumerate(lines)))
    keys = ("status", "stderr", "stdout", "log", "files")
    diffs = [(args, [k for k in keys if t[k] != r[k]]) for args, t, r in results if any(t[k] != r[k] for k in keys)]
    by_status = {}
    for _, t, _ in results:
        by_status[t["status"]] = by_status.get(t["status"], 0) + 1
    rev = sh(["git", "-C", ROOT, "rev-parse", "--short", a.rev]).strip()
    rep = ["cli_trace.py: host/main.cpp of the working tree against %s, both built against scripts/cli_trace_stub.c (no GPU)" % rev,
           "command lines:                    %d (%d of them the README's scaled down, %d recorded from the CPU tests named test_cli_*: %s; --bin lines %s)"
           % (len(lines), n_readme, n_rec, tests, "with a 6 x 5 x 4 cloud.bin" if cloud else "without a volume file"),
           "  by exit status:                 " + ", ".join("%s: %d" % kv for kv in sorted(by_status.items(), key=str)),
           "  that reach the render:          %d" % sum(bool(RENDERS.search(t["raw"])) for _, t, _ in results),
           "  that write at least one file:   %d" % sum(bool(t["files"]) for _, t, _ in results),
           "differences (exit status, stderr, stdout with the timing numbers masked, normalised call log, files): %d" % len(diffs),
           "  raw call logs that differ (allocation order inside a block of vp_malloc / vp_memset / vp_free, buffer ordinals): %d"
           % sum(t["raw"] != r["raw"] for _, t, r in results)]
    rep += ["  DIFFERENT %s: %s" % (", ".join(what), " ".join(args)) for args, what in diffs]
    open(a.out, "w").write("\n".join(rep) + "\n")
    print("\n".join(rep))
    if not a.keep:
        shutil.rmtree(tmp)
    return 1 if diffs else 0


if __name__ == "__main__":
    sys.exit(main())
