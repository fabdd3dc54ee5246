"""What the half-buffer render of a plane call costs against the mode's _stats call, and what the cross-filter on planes returns beside
the self-guided per-plane vp_denoise (development tool; the bench is bench.py):

    python scripts/plane_halves_cost.py c2,c4f [--modes layers,groups,group_layers] [--frames 1024] [--repeat 5] [--quality-frames 16]
                                        [--ref-frames 1024] [--params 5:1:0.45,10:3:0.45] [--parent-tree DIR] [--out FILE]

A workload is a bench workload of volpath/scene.py at its own image size (c2: 800 x 600, c4f: 1280 x 720); the stream is Philox2x32-7.

  cost     per mode, the mode's _stats call and vp_render_frames_planes_halves_stats on the same --frames frames: ONE CHILD PROCESS PER
           READING, the two calls alternated --repeat times.  Every time is min / median / max over the readings: the WHOLE CALL (a host
           clock from before the call to after vp_synchronize, which includes the reduce) and the render launches' kernel time
           (vp_render_time_ms).  The yardstick is the _stats call of the same build; the margin is the spread of the alternation's own
           readings -- (max - min) over the median --, and the line says on which side of it the difference lies.  Wall minus render
           kernel is the reduce's share (with the host's part of the call).
  returns  --quality-frames frames of a group-layers render: relative L2 of each plane's RGB mean and of one relit composite against
           the mean of --ref-frames frames under OTHER keys, for the plain mean, vp_denoise self-guided per plane (--planes-denoise),
           the cross-filter of each plane's two halves (--planes-denoise-cross) and that with the variance stage (--plane-denoise-var).

With --parent-tree (a built cuda-volpath_amd directory of the parent commit: its library and its Python package) that build's
vp_render_frames runs in child processes, alternated with this build's: the two builds are compared child against child, and the
spread of the parent's children is the margin."""
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
ap.add_argument("--modes", default="layers,groups,group_layers")
ap.add_argument("--frames", type=int, default=1024)
ap.add_argument("--repeat", type=int, default=5)
ap.add_argument("--quality-frames", type=int, default=16)
ap.add_argument("--ref-frames", type=int, default=1024)
ap.add_argument("--params", default="5:1:0.45,10:3:0.45")
ap.add_argument("--parent-tree", default=None)
ap.add_argument("--out", default=None)
ap.add_argument("--child", default=None, help=argparse.SUPPRESS)   # one reading: beauty, stats:MODE or halves:MODE
args = ap.parse_args()
out_file = open(args.out, "a") if args.out else None
KEY, REF_KEY = (0x9E3779B9, 0x85EBCA6B), (0x1234567, 0x7654321)
PARAMS = [(int(r), int(f), float(k)) for r, f, k in (p.split(":") for p in args.params.split(","))]
RNG = vp.RNG_PHILOX7
MODE = {"layers": 1, "groups": 2, "group_layers": 3}
SUN_GAIN, SKY_GAIN, OVER = (1.5, 1.2, 0.9), (0.5, 0.5, 0.5), (0.2, 0.4, 0.9)
VAR = (1, 3, 0.45)


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


def sha(arrays):
    h = hashlib.sha1()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:12]


def rel_l2(img, ref):
    a, b = img[..., :3].astype(np.float64), ref[..., :3].astype(np.float64)
    num, den = ((a - b) ** 2).sum(), (b ** 2).sum()
    if den == 0:                                     # (a plane that is identically zero in the reference: trans of a frame-filling cloud)
        return 0.0 if num == 0 else float("inf")
    return float(np.sqrt(num / den))


def stats_call(mode):
    return {1: vp.render_frames_layers_stats, 2: vp.render_frames_groups_stats, 3: vp.render_frames_group_layers_stats}[mode]


def reading(spec, what, tree=None):
    """one reading in a child process: {"t": (wall, kernel, launches), "hash": of what the call left}"""
    env = dict(os.environ)
    if tree:
        env["VOLPATH_TREE"] = os.path.abspath(tree)
        env.pop("VOLPATH_LIB", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), spec, "--frames", str(args.frames), "--child", what], env=env, capture_output=True, text=True)
    if r.returncode:
        raise RuntimeError("child %s failed: %s" % (what, r.stderr[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def child(spec, what):
    N = args.frames
    P, _ = scene.setup(spec, rng_mode=RNG, key=KEY, last_frame=N, sunsky=scene.default_sunsky())
    W, H = P.width, P.height
    vp.prepare(P)
    if what == "beauty":
        buf = vp.DeviceBuffer(W, H)
        vp.reserve_frames(P, N)
        vp.render_frames(buf.ptr, 0, 2, P); vp.synchronize()
        buf.reset()
        t = timed(lambda: vp.render_frames(buf.ptr, 0, N, P))
        print(json.dumps({"t": t, "hash": sha([buf.download()])}))
        return
    kind, mode = what.split(":")
    mode = MODE[mode]
    n = len(vp.PLANE_NAMES[mode])
    (vp.reserve_frames if mode == 1 else vp.reserve_frames_groups)(P, N)
    halves = 2 if kind == "halves" else 1
    acc = [[vp.DeviceBuffer(W, H) for _ in range(n)] for _ in range(halves)]
    rec = [[vp.StatsBuffer(W, H) for _ in range(n)] for _ in range(halves)]
    pairs = [[(a.ptr, r.ptr) for a, r in zip(acc[h], rec[h])] for h in range(halves)]
    if kind == "halves":
        call = lambda f, k: vp.render_frames_planes_halves_stats(mode, pairs[0], pairs[1], f, k, P)
    else:
        call = lambda f, k: stats_call(mode)(*[a.ptr for a in acc[0]], *[r.ptr for r in rec[0]], f, k, P)
    call(0, 2); vp.synchronize()                       # warm: the call's kernels are loaded
    for b in sum(acc + rec, []):
        b.reset()
    t = timed(lambda: call(0, N))
    counts = [int(r.download()["n"][0, 0]) for r in sum(rec, [])]
    assert counts == ([N] * n if halves == 1 else [(N + 1) // 2] * n + [N // 2] * n), counts
    print(json.dumps({"t": t, "hash": sha([b.download() for b in sum(acc, [])])}))


def cost(spec):
    say(f"== {spec}: {args.frames} frames per call, {args.repeat} readings of each call, one child process per reading, alternated (min / median / max)")
    for name in args.modes.split(","):
        a, b = [], []
        for _ in range(args.repeat):
            a.append(reading(spec, "stats:" + name)["t"])
            b.append(reading(spec, "halves:" + name)["t"])
        say(f"cost  {name:12s} _stats call          wall ms {mmm(x[0] for x in a)}   render kernel ms {mmm(x[1] for x in a)}   launches {a[0][2]}")
        say(f"cost  {name:12s} planes-halves call   wall ms {mmm(x[0] for x in b)}   render kernel ms {mmm(x[1] for x in b)}   launches {b[0][2]}")
        wa, wb = statistics.median(x[0] for x in a), statistics.median(x[0] for x in b)
        ka, kb = statistics.median(x[1] for x in a), statistics.median(x[1] for x in b)
        floor = max(spread(x[0] for x in a), spread(x[0] for x in b))
        diff = 100.0 * (wb / wa - 1)
        say(f"cost  {name:12s} halves against _stats, medians: wall {wb - wa:+.2f} ms ({diff:+.2f} %), render kernel {100.0 * (kb / ka - 1):+.2f} %;"
            f" wall minus render kernel (reduce, host): _stats {wa - ka:.2f} ms ({100.0 * (wa - ka) / wa:.2f} % of the call), halves {wb - kb:.2f} ms"
            f" ({100.0 * (wb - kb) / wb:.2f} %); spread of the alternation: _stats wall {spread(x[0] for x in a):.2f} %, halves wall {spread(x[0] for x in b):.2f} %"
            f" -- the difference is {'INSIDE' if abs(diff) <= floor else 'OUTSIDE'} the spread")


def parent(spec):
    own_tree = os.path.join(ROOT, "cuda-volpath_amd")
    t, o = [], []
    for _ in range(args.repeat):
        t.append(reading(spec, "beauty", args.parent_tree))
        o.append(reading(spec, "beauty", own_tree))
    same = len({x["hash"] for x in t + o}) == 1
    kp, ko = statistics.median(x["t"][1] for x in t), statistics.median(x["t"][1] for x in o)
    wp, wo = statistics.median(x["t"][0] for x in t), statistics.median(x["t"][0] for x in o)
    say(f"parent  vp_render_frames  wall ms {mmm(x['t'][0] for x in t)}   kernel ms {mmm(x['t'][1] for x in t)}   image {t[0]['hash']}")
    say(f"own     vp_render_frames  wall ms {mmm(x['t'][0] for x in o)}   kernel ms {mmm(x['t'][1] for x in o)}   image {o[0]['hash']}" + ("" if same else "   IMAGES DIFFER"))
    say(f"this build's beauty render against the parent's, child against child, medians: kernel {100.0 * (ko / kp - 1):+.2f} %, wall {100.0 * (wo / wp - 1):+.2f} % "
        f"(the parent's own spread: kernel {spread(x['t'][1] for x in t):.2f} %, wall {spread(x['t'][0] for x in t):.2f} %; this build's: kernel {spread(x['t'][1] for x in o):.2f} %)")


def returns(spec):
    Q, NR, mode = args.quality_frames, args.ref_frames, 3
    names = vp.PLANE_NAMES[mode]
    P, _ = scene.setup(spec, rng_mode=RNG, key=REF_KEY, last_frame=max(Q, NR), sunsky=scene.default_sunsky())
    W, H = P.width, P.height
    npix = W * H
    img = lambda: vp.DeviceBuffer(W, H)
    recs = lambda: vp.StatsBuffer(W, H)
    comp = img()

    def composite(planes, s):
        vp.relight_composite(comp.ptr, planes[0].ptr, planes[1].ptr, planes[2].ptr, npix, s, SUN_GAIN, SKY_GAIN, plate_rgb=OVER)
        return comp.download()

    ref = [img() for _ in names]
    vp.render_frames_group_layers(*[b.ptr for b in ref], 0, NR, P)
    ref_comp = composite(ref, 1.0 / NR)
    ref_img = [b.download() / np.float32(NR) for b in ref]
    vp.set_rng(RNG, KEY)
    whole, wrec = [img() for _ in names], [recs() for _ in names]
    vp.render_frames_group_layers_stats(*[b.ptr for b in whole], *[b.ptr for b in wrec], 0, Q, P)
    half = [[(img(), recs()) for _ in names] for _ in (0, 1)]
    pairs = [[(a.ptr, r.ptr) for a, r in h] for h in half]
    vp.render_frames_planes_halves_stats(mode, pairs[0], pairs[1], 0, Q, P)
    dst, ta, tb = [img() for _ in names], img(), img()
    var = [vp.lib().vp_malloc(npix * 4) for _ in range(3)]

    def row(label):
        planes = "  ".join("%s %.4f" % (n, rel_l2(d.download(), r)) for n, d, r in zip(names, dst, ref_img))
        return f"{label:34s} {planes}  composite {rel_l2(composite(dst, 1.0), ref_comp):.4f}"

    say(f"returns  {spec}: {W}x{H}, {Q} frames ({(Q + 1) // 2} + {Q // 2} in the halves), reference {NR} frames under other keys; relative L2 per plane and of"
        f" the composite at sun gain {SUN_GAIN}, sky gain {SKY_GAIN}, over {OVER}")
    for k in range(3):
        vp.scale_by_count(dst[k].ptr, whole[k].ptr, wrec[k].ptr, npix, 1.0)
    say("returns  " + spec + "  " + row("plain mean"))
    for R, F, k in PARAMS:
        for j in range(3):
            vp.denoise(dst[j].ptr, whole[j].ptr, wrec[j].ptr, W, H, R, F, k)
        say("returns  " + spec + "  " + row(f"({R}, {F}) --planes-denoise"))
        vp.denoise_cross_planes(mode, [d.ptr for d in dst], None, pairs[0], pairs[1], ta.ptr, tb.ptr, W, H, R, F, k)
        say("returns  " + spec + "  " + row(f"({R}, {F}) --planes-denoise-cross"))
        vp.denoise_cross_planes(mode, [d.ptr for d in dst], None, pairs[0], pairs[1], ta.ptr, tb.ptr, W, H, R, F, k, variance=VAR, var_ptrs=var)
        say("returns  " + spec + "  " + row(f"({R}, {F}) ... --plane-denoise-var"))
    vp.synchronize()
    for p in var:
        vp.lib().vp_free(p)
    for b in [comp, ta, tb] + ref + whole + wrec + dst + [x for h in half for pr in h for x in pr]:
        b.free()


vp.set_device(0)
for spec in args.workloads.split(","):
    if args.child:
        child(spec, args.child)
        continue
    cost(spec)
    if args.parent_tree:
        parent(spec)
    if args.quality_frames > 0:
        returns(spec)
