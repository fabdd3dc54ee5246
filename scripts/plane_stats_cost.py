"""What the per-plane statistics (vp_render_frames_groups_stats / vp_render_frames_layers_stats) cost against
the plain plane calls, and whether the feature cost the beauty render anything (development tool; the bench is bench.py):

    python scripts/plane_stats_cost.py c2,c4f [--frames 1024] [--repeat 3] [--parent-tree DIR] [--out FILE]

A workload is a bench workload of volpath/scene.py at the bench's size.  For groups and for layers the plain call and the _stats call
alternate `repeat` times inside one process; every time is given as min / median / max over the repeats, and the spread of the
alternation is the noise floor of the comparison.  The time that matters is the WHOLE CALL, a host clock from before the call to after
vp_synchronize: the reduce that folds the records runs outside the library's HIP-event time of the render launches
(vp_render_time_ms), which is printed beside it and should not move -- the render launches are the same kernels.  The accumulators of
the two calls are compared by hash.  The code predicts one more cost only: per pixel and launch two 24-byte record read-modify-writes,
per staged sample two binary64 multiply-adds in the reduce; the launches per call are printed so that the first can be counted.
With --parent-tree (a built cuda-volpath_amd directory of the parent commit: its library and its Python package) that build's
vp_render_frames runs in child processes before and after, and so does this build's, in the same way (parent, this build, the
alternations, this build, parent): the two builds are compared child against child, and the spread of those children is the margin."""
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
    """(wall ms from before the call to after a synchronise, kernel ms of the render launches by HIP events, launches)"""
    vp.synchronize(); vp.render_time_ms()
    t = time.perf_counter()
    fn()
    vp.synchronize()
    wall = (time.perf_counter() - t) * 1e3
    ms, launches = vp.render_time_ms()
    return wall, ms, launches


def sha(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()[:12]


def beauty_child(spec, tree):
    """vp_render_frames of a build of the library, `repeat` times, in a child process: [(wall, kernel, launches)], hash"""
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
    second, rec = vp.DeviceBuffer(W, H), (vp.StatsBuffer(W, H), vp.StatsBuffer(W, H))
    vp.reserve_frames_groups(P, N)
    say(f"== {spec}: {W}x{H}, {N} frames per call, {args.repeat} repeats (min / median / max)")
    say(f"staged frames per launch: {vp.groups_frames_per_launch(P, 1)} with one plane (layers), {vp.groups_frames_per_launch(P, 2)} with two (groups)")
    own_tree = os.path.join(ROOT, "cuda-volpath_amd")
    before = beauty_child(spec, args.parent_tree) if args.parent_tree else None
    own_before = beauty_child(spec, own_tree) if args.parent_tree else None
    for kind, plain_fn, stats_fn in (("groups", vp.render_frames_groups, vp.render_frames_groups_stats), ("layers", vp.render_frames_layers, vp.render_frames_layers_stats)):
        def plain():
            buf.reset(); second.reset()
            return timed(lambda: plain_fn(buf.ptr, second.ptr, 0, N, P))

        def stats():
            buf.reset(); second.reset(); rec[0].reset(); rec[1].reset()
            return timed(lambda: stats_fn(buf.ptr, second.ptr, rec[0].ptr, rec[1].ptr, 0, N, P))

        plain_fn(buf.ptr, second.ptr, 0, 2, P)                                   # warm both shapes of the call: its kernels are loaded
        stats_fn(buf.ptr, second.ptr, rec[0].ptr, rec[1].ptr, 0, 2, P); vp.synchronize()
        a, b = [], []
        for _ in range(args.repeat):
            a.append(plain()); ha = sha(buf.download()) + " " + sha(second.download())
            b.append(stats()); hb = sha(buf.download()) + " " + sha(second.download())
        r0, r1 = rec[0].download(), rec[1].download()
        assert (r0["n"] == N).all() and (r1["n"] == N).all(), "a record did not receive every frame"
        say(f"{kind}  plain call   wall ms {mmm(x[0] for x in a)}   render kernel ms {mmm(x[1] for x in a)}   launches {a[0][2]}   planes {ha}")
        say(f"{kind}  _stats call  wall ms {mmm(x[0] for x in b)}   render kernel ms {mmm(x[1] for x in b)}   launches {b[0][2]}   planes {hb}"
            + ("" if ha == hb else "   PLANES DIFFER") + f"   records {sha(r0)} {sha(r1)}")
        wa, wb = statistics.median(x[0] for x in a), statistics.median(x[0] for x in b)
        ka, kb = statistics.median(x[1] for x in a), statistics.median(x[1] for x in b)
        say(f"{kind}  _stats against plain, medians: wall {wb - wa:+.2f} ms ({100.0 * (wb / wa - 1):+.2f} %), render kernel {100.0 * (kb / ka - 1):+.2f} %;"
            f" wall minus render kernel (reduces, memsets, host): plain {wa - ka:.2f} ms, _stats {wb - kb:.2f} ms;"
            f" noise floor (max - min over median of the alternation): plain wall {spread(x[0] for x in a):.2f} %, _stats wall {spread(x[0] for x in b):.2f} %")
    own_after = beauty_child(spec, own_tree) if args.parent_tree else None
    after = beauty_child(spec, args.parent_tree) if args.parent_tree else None
    if before:
        t, o = before["times"] + after["times"], own_before["times"] + own_after["times"]
        kp, ko = statistics.median(x[1] for x in t), statistics.median(x[1] for x in o)
        wp, wo = statistics.median(x[0] for x in t), statistics.median(x[0] for x in o)
        same = before["hash"] == after["hash"] == own_before["hash"] == own_after["hash"]
        say(f"parent  vp_render_frames (child processes before and after)  wall ms {mmm(x[0] for x in t)}   kernel ms {mmm(x[1] for x in t)}   image {before['hash']}")
        say(f"own     vp_render_frames (this build, child processes before and after)  wall ms {mmm(x[0] for x in o)}   kernel ms {mmm(x[1] for x in o)}"
            f"   image {own_before['hash']}" + ("" if same else "   IMAGES DIFFER"))
        say(f"this build's beauty render against the parent's, child against child, medians: kernel {100.0 * (ko / kp - 1):+.2f} %, wall {100.0 * (wo / wp - 1):+.2f} % "
            f"(kernel spreads: parent {spread(x[1] for x in t):.2f} %, this build {spread(x[1] for x in o):.2f} %)")
    buf.free(); second.free(); rec[0].free(); rec[1].free()
