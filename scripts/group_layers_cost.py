"""What a group-layers launch (vp_render_frames_group_layers) costs against one light-groups call, against the
groups call plus the layers call it replaces, what its _stats form costs against the plain form, and whether the feature cost the
beauty render anything (development tool; the bench is bench.py):

    python scripts/group_layers_cost.py c2,c4f [--frames 1024] [--repeat 3] [--parent-tree DIR [--own-first]] [--out FILE]

A workload is a bench workload of volpath/scene.py at the bench's size.  The candidates -- vp_render_frames_groups,
vp_render_frames_group_layers, vp_render_frames_layers, vp_render_frames_group_layers_stats -- alternate `repeat` times inside one
process; every time is given as min / median / max over the repeats, and the spread of the alternation is the noise floor of the
comparison.  Kernel time is the library's HIP-event time of the render launches (vp_render_time_ms: without the reduces), wall time is
taken around a synchronise (with them).  With --parent-tree (a built cuda-volpath_amd directory of the parent commit: its library and
its Python package) that build's vp_render_frames and this build's run in child processes in alternation (parent, this build, parent,
this build; --own-first: this build first): the two builds are compared child against child, and the difference between the parent's
two runs, as measured here, is the margin.  The accumulator hashes must agree."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("VOLPATH_TREE") or os.path.join(ROOT, "cuda-volpath_amd"))   # (VOLPATH_TREE: the child of --parent-tree)
import numpy as np  # noqa: E402
import volpath as vp  # noqa: E402
from volpath import scene  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("workloads")
ap.add_argument("--frames", type=int, default=1024)
ap.add_argument("--repeat", type=int, default=3)
ap.add_argument("--parent-tree", default=None)
ap.add_argument("--out", default=None)
ap.add_argument("--own-first", action="store_true", help="the children in the order this build, parent, this build, parent")
ap.add_argument("--plain-child", action="store_true", help=argparse.SUPPRESS)   # the child process of --parent-tree
args = ap.parse_args()
out_file = open(args.out, "a") if args.out else None
KEY = (0x9E3779B9, 0x85EBCA6B)


def say(*a):
    line = " ".join(str(v) for v in a)
    print(line, flush=True)
    if out_file:
        out_file.write(line + "\n"); out_file.flush()


def mmm(v):
    v = list(v)
    return "%.2f / %.2f / %.2f" % (min(v), statistics.median(v), max(v))


def spread(v):
    v = list(v)
    return 100.0 * (max(v) - min(v)) / statistics.median(v)


def timed(fn):
    """(wall ms around a synchronise, kernel ms by HIP events)"""
    vp.synchronize(); vp.render_time_ms()
    t = time.perf_counter()
    fn()
    vp.synchronize()
    wall = (time.perf_counter() - t) * 1e3
    ms, _ = vp.render_time_ms()
    return wall, ms


def sha(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()[:12]


def beauty_child(spec, tree):
    """vp_render_frames of a build of the library, `repeat` times, in a child process: [(wall, kernel)], hash"""
    env = dict(os.environ, VOLPATH_TREE=os.path.abspath(tree))
    env.pop("VOLPATH_LIB", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), spec, "--frames", str(args.frames), "--repeat", str(args.repeat), "--plain-child"],
                       env=env, capture_output=True, text=True)
    if r.returncode:
        raise RuntimeError("child with %s failed: %s" % (tree, r.stderr[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


vp.set_device(0)
sky = scene.default_sunsky()
for spec in args.workloads.split(","):
    P, info = scene.setup(spec, rng_mode=int(os.environ.get("VP_PERF_RNG", vp.RNG_PHILOX7)), key=KEY, last_frame=args.frames, sunsky=sky)
    W, H, N = P.width, P.height, args.frames
    buf = vp.DeviceBuffer(W, H)
    vp.prepare(P); vp.reserve_frames(P, N)
    vp.render_frames(buf.ptr, 0, 2, P); vp.synchronize()

    if args.plain_child:
        t = []
        for _ in range(args.repeat):
            buf.reset()
            t.append(timed(lambda: vp.render_frames(buf.ptr, 0, N, P)))
        print(json.dumps({"times": t, "hash": sha(buf.download())}))
        continue
    b1, b2 = vp.DeviceBuffer(W, H), vp.DeviceBuffer(W, H)
    recs = [vp.StatsBuffer(W, H) for _ in range(3)]

    def run(call, bufs, stats=()):
        for b in tuple(bufs) + tuple(stats):
            b.reset()
        return timed(lambda: call(*[b.ptr for b in tuple(bufs) + tuple(stats)], 0, N, P))

    cands = {"groups": lambda: run(vp.render_frames_groups, (buf, b1)),
             "group_layers": lambda: run(vp.render_frames_group_layers, (buf, b1, b2)),
             "layers": lambda: run(vp.render_frames_layers, (buf, b1)),
             "group_layers_stats": lambda: run(vp.render_frames_group_layers_stats, (buf, b1, b2), recs)}
    vp.reserve_frames_groups(P, N)
    for c in cands.values():
        c()                                                  # once unmeasured
    say(f"== {spec}: {W}x{H}, {N} frames per call, {args.repeat} repeats (min / median / max)")
    say(f"staged frames per launch: {vp.groups_frames_per_launch(P, 1)} with one plane (beauty, layers), {vp.groups_frames_per_launch(P, 2)} with two (groups, group layers)")
    t, img = {k: [] for k in cands}, {}
    for _ in range(args.repeat):
        for k, c in cands.items():
            t[k].append(c())
            img[k] = (buf.download(), b1.download(), b2.download())
    gl, st, gr, ly = img["group_layers"], img["group_layers_stats"], img["groups"], img["layers"]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(gl, st)), "the _stats form's accumulators are not the plain form's"
    assert gl[2].tobytes() == ly[1].tobytes(), "trans is not the layers call's"
    assert gl[0][..., 3].tobytes() == gl[1][..., 3].tobytes() == ly[0][..., 3].tobytes(), "the three w differ"
    for k, names in (("groups", "vp_render_frames_groups"), ("group_layers", "vp_render_frames_group_layers"), ("layers", "vp_render_frames_layers"),
                     ("group_layers_stats", "vp_render_frames_group_layers_stats")):
        say(f"{k:18s} {names:36s} wall ms {mmm(x[0] for x in t[k])}   kernel ms {mmm(x[1] for x in t[k])}   planes {' '.join(sha(a) for a in img[k][:2 if k in ('groups', 'layers') else 3])}")
    med = lambda k, j: statistics.median(x[j] for x in t[k])
    say(f"group layers against one groups call, medians: kernel {100.0 * (med('group_layers', 1) / med('groups', 1) - 1):+.2f} %, wall "
        f"{100.0 * (med('group_layers', 0) / med('groups', 0) - 1):+.2f} %; noise floor (max - min over median of the alternation): groups kernel "
        f"{spread(x[1] for x in t['groups']):.2f} %, group layers kernel {spread(x[1] for x in t['group_layers']):.2f} %")
    say(f"group layers against the pair it replaces (a groups call plus a layers call), medians: kernel "
        f"{100.0 * (med('group_layers', 1) / (med('groups', 1) + med('layers', 1)) - 1):+.2f} %, wall "
        f"{100.0 * (med('group_layers', 0) / (med('groups', 0) + med('layers', 0)) - 1):+.2f} %")
    say(f"_stats against plain, whole call (wall), medians: {100.0 * (med('group_layers_stats', 0) / med('group_layers', 0) - 1):+.2f} % "
        f"(kernel {100.0 * (med('group_layers_stats', 1) / med('group_layers', 1) - 1):+.2f} %); spreads of the wall times: plain "
        f"{spread(x[0] for x in t['group_layers']):.2f} %, _stats {spread(x[0] for x in t['group_layers_stats']):.2f} %")
    if args.parent_tree:
        own_tree = os.path.join(ROOT, "cuda-volpath_amd")
        order = (own_tree, args.parent_tree) * 2 if args.own_first else (args.parent_tree, own_tree) * 2
        runs = [beauty_child(spec, tree) for tree in order]
        if args.own_first:
            runs = [runs[1], runs[0], runs[3], runs[2]]      # (listed parent first all the same)
            say("children ran in the order: this build, parent, this build, parent")
        kmed = [statistics.median(x[1] for x in r["times"]) for r in runs]
        same = len({r["hash"] for r in runs}) == 1
        for who, r in zip(("parent", "own   ", "parent", "own   "), runs):
            say(f"{who} vp_render_frames (child process)  wall ms {mmm(x[0] for x in r['times'])}   kernel ms {mmm(x[1] for x in r['times'])}   image {r['hash']}")
        if not same:
            say("IMAGES DIFFER")
        kp = statistics.median(x[1] for r in (runs[0], runs[2]) for x in r["times"])
        ko = statistics.median(x[1] for r in (runs[1], runs[3]) for x in r["times"])
        margin = 100.0 * abs(kmed[0] - kmed[2]) / kp
        diff = 100.0 * (ko / kp - 1)
        say(f"this build's beauty render against the parent's, kernel medians, child against child: {diff:+.2f} %; margin (the parent's two runs against each "
            f"other) {margin:.2f} %; spread of all the parent's times {spread(x[1] for r in (runs[0], runs[2]) for x in r['times']):.2f} %, of this build's "
            f"{spread(x[1] for r in (runs[1], runs[3]) for x in r['times']):.2f} %: " + ("inside the margin" if abs(diff) <= margin else "OUTSIDE the margin"))
    for b in [buf, b1, b2] + recs:
        b.free()
