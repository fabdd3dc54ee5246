"""What a light-groups launch (vp_render_frames_groups) costs against the beauty render and against the two
beauty renders the separation took before, and whether the feature cost the beauty render anything (development tool; the bench is
bench.py):

    python scripts/groups_cost.py c2,c4f [--frames 1024] [--repeat 3] [--parent-tree DIR] [--out FILE]

A workload is a bench workload of volpath/scene.py at the bench's size.  vp_render_frames and vp_render_frames_groups alternate
`repeat` times inside one process; every time is given as min / median / max over the repeats, and the spread of the alternation is
the noise floor of the comparison.  Kernel time is the library's HIP-event time of the render launches (vp_render_time_ms: without the
reduces), wall time is taken around a synchronise (with them).  A groups call of more frames than a launch holds in two planes is cut
into several launches; the frames per launch with one plane and with two are printed.  With --parent-tree (a built cuda-volpath_amd
directory of the parent commit: its library and its Python package) that build's vp_render_frames runs in child processes before and
after, and so does this build's, in the same way (parent, this build, the alternation, this build, parent): the two builds are
compared child against child, and the spread of those children is the margin.  The accumulator hashes must agree."""
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


def parent_child(spec, tree):
    """vp_render_frames of another build of the library, `repeat` times, in a child process: [(wall, kernel)], hash"""
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

    def plain():
        buf.reset()
        return timed(lambda: vp.render_frames(buf.ptr, 0, N, P))

    if args.plain_child:
        t = [plain() for _ in range(args.repeat)]
        print(json.dumps({"times": t, "hash": sha(buf.download())}))
        continue
    skyb = vp.DeviceBuffer(W, H)

    def groups():
        buf.reset(); skyb.reset()
        return timed(lambda: vp.render_frames_groups(buf.ptr, skyb.ptr, 0, N, P))

    vp.reserve_frames_groups(P, N)
    vp.render_frames_groups(buf.ptr, skyb.ptr, 0, 2, P); vp.synchronize()
    say(f"== {spec}: {W}x{H}, {N} frames per call, {args.repeat} repeats (min / median / max)")
    say(f"staged frames per launch: {vp.groups_frames_per_launch(P, 1)} with one plane (vp_render_frames), {vp.groups_frames_per_launch(P, 2)} with two (vp_render_frames_groups)")
    own_tree = os.path.join(ROOT, "cuda-volpath_amd")
    before = parent_child(spec, args.parent_tree) if args.parent_tree else None
    own_before = parent_child(spec, own_tree) if args.parent_tree else None
    a, b = [], []
    for _ in range(args.repeat):
        a.append(plain()); ha = buf.download()
        b.append(groups()); su, sk = buf.download(), skyb.download()
    own_after = parent_child(spec, own_tree) if args.parent_tree else None
    after = parent_child(spec, args.parent_tree) if args.parent_tree else None
    assert np.array_equal(su[..., 3], ha[..., 3]) and np.array_equal(sk[..., 3], ha[..., 3]), "a group's w is not the beauty w"
    rel = np.abs(su[..., :3].astype(np.float64) + sk[..., :3] - ha[..., :3]).max() / max(float(ha[..., :3].max()), 1e-30)
    say(f"beauty  vp_render_frames         wall ms {mmm(x[0] for x in a)}   kernel ms {mmm(x[1] for x in a)}   image {sha(ha)}")
    say(f"groups  vp_render_frames_groups  wall ms {mmm(x[0] for x in b)}   kernel ms {mmm(x[1] for x in b)}   sun {sha(su)} sky {sha(sk)}"
        f"   max |sun + sky - beauty| / max beauty {rel:.2e}")
    ka, kb = statistics.median(x[1] for x in a), statistics.median(x[1] for x in b)
    wa, wb = statistics.median(x[0] for x in a), statistics.median(x[0] for x in b)
    say(f"groups against this build's beauty render, medians: kernel {100.0 * (kb / ka - 1):+.2f} %, wall {100.0 * (wb / wa - 1):+.2f} %;"
        f" against twice the beauty render (the separation by two renders): kernel {100.0 * (kb / (2 * ka) - 1):+.2f} %, wall {100.0 * (wb / (2 * wa) - 1):+.2f} %;"
        f" noise floor (max - min over median of the alternation): beauty kernel {spread(x[1] for x in a):.2f} %, groups kernel {spread(x[1] for x in b):.2f} %")
    if before:
        t = before["times"] + after["times"]
        kp = statistics.median(x[1] for x in t)
        say(f"parent  vp_render_frames (child processes before and after)  wall ms {mmm(x[0] for x in t)}   kernel ms {mmm(x[1] for x in t)}"
            f"   image {before['hash']}" + ("" if before["hash"] == after["hash"] == sha(ha) else "   IMAGES DIFFER"))
        o = own_before["times"] + own_after["times"]
        ko = statistics.median(x[1] for x in o)
        say(f"own     vp_render_frames (this build, child processes before and after)  wall ms {mmm(x[0] for x in o)}   kernel ms {mmm(x[1] for x in o)}"
            f"   image {own_before['hash']}" + ("" if own_before["hash"] == own_after["hash"] == sha(ha) else "   IMAGES DIFFER"))
        say(f"this build's beauty render against the parent's, kernel medians: child against child {100.0 * (ko / kp - 1):+.2f} % "
            f"(spreads: parent {spread(x[1] for x in t):.2f} %, this build {spread(x[1] for x in o):.2f} %); the alternating process against the parent's children {100.0 * (ka / kp - 1):+.2f} %")
    buf.free(); skyb.free()
