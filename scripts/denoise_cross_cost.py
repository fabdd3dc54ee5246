"""What the half-buffer render costs against vp_render_frames_stats, and what the cross-filter returns beside the self-guided vp_denoise
(development tool; the bench is bench.py):

    python scripts/denoise_cross_cost.py c2,c4f [--frames 1024] [--repeat 5] [--quality-frames 16] [--ref-frames 1024]
                                         [--params 5:1:0.45,10:3:0.45] [--parent-tree DIR] [--out FILE]

A workload is a bench workload of volpath/scene.py at its own image size (c2: 800 x 600, c4f: 1280 x 720).  Per workload:

  cost     vp_render_frames_stats and vp_render_frames_halves_stats on the same --frames frames, alternated --repeat times inside one
           process.  Every time is min / median / max over the repeats: the WHOLE CALL (a host clock from before the call to after
           vp_synchronize, which includes the reduce) and the render launches' kernel time (vp_render_time_ms).  The spread of the
           alternation -- (max - min) over the median -- is the noise floor, and the line says on which side of it the difference lies.
           The sum of the two halves' counts is checked against the frames.
  returns  --quality-frames frames: relative L2 of the RGB mean image against the mean of --ref-frames frames under OTHER keys, for the
           plain mean, vp_denoise self-guided on all the frames, and the cross-filter of the two halves (two vp_denoise calls with the
           roles swapped, vp_merge_halves), at the same (R, F, k); and the residual map's mean beside the true relative error it estimates.

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
ap.add_argument("--repeat", type=int, default=5)
ap.add_argument("--quality-frames", type=int, default=16)
ap.add_argument("--ref-frames", type=int, default=1024)
ap.add_argument("--params", default="5:1:0.45,10:3:0.45")
ap.add_argument("--parent-tree", default=None)
ap.add_argument("--out", default=None)
ap.add_argument("--plain-child", action="store_true", help=argparse.SUPPRESS)   # the child process of --parent-tree
args = ap.parse_args()
out_file = open(args.out, "a") if args.out else None
KEY, REF_KEY = (0x9E3779B9, 0x85EBCA6B), (0x1234567, 0x7654321)
PARAMS = [(int(r), int(f), float(k)) for r, f, k in (p.split(":") for p in args.params.split(","))]
RNG = int(os.environ.get("VP_PERF_RNG", vp.RNG_PHILOX7))


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


def rel_l2(img, ref):
    a, b = img[..., :3].astype(np.float64), ref[..., :3].astype(np.float64)
    return float(np.sqrt(((a - b) ** 2).sum() / (b ** 2).sum()))


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
    N, Q = args.frames, args.quality_frames
    P, info = scene.setup(spec, rng_mode=RNG, key=KEY, last_frame=max(N, Q, args.ref_frames), sunsky=sky)
    W, H = P.width, P.height
    npix = W * H
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
    half1, rec = vp.DeviceBuffer(W, H), (vp.StatsBuffer(W, H), vp.StatsBuffer(W, H))
    own_tree = os.path.join(ROOT, "cuda-volpath_amd")
    before = beauty_child(spec, args.parent_tree) if args.parent_tree else None
    own_before = beauty_child(spec, own_tree) if args.parent_tree else None

    # ---- cost: the uniform call with records against the halves call, same frames, alternated
    def stats():
        buf.reset(); rec[0].reset()
        return timed(lambda: vp.render_frames_stats(buf.ptr, rec[0].ptr, 0, N, P))

    def halves():
        buf.reset(); half1.reset(); rec[0].reset(); rec[1].reset()
        return timed(lambda: vp.render_frames_halves_stats(buf.ptr, half1.ptr, rec[0].ptr, rec[1].ptr, 0, N, P))

    vp.render_frames_stats(buf.ptr, rec[0].ptr, 0, 2, P)                                    # warm both shapes of the call: its kernels are loaded
    vp.render_frames_halves_stats(buf.ptr, half1.ptr, rec[0].ptr, rec[1].ptr, 0, 2, P); vp.synchronize()
    say(f"== {spec}: {W}x{H}, {N} frames per call, {args.repeat} repeats (min / median / max)")
    a, b = [], []
    for _ in range(args.repeat):
        a.append(stats())
        b.append(halves())
    r0, r1 = rec[0].download(), rec[1].download()
    assert (r0["n"] + r1["n"] == N).all() and (r0["n"] == (N + 1) // 2).all(), "a half did not receive its frames"
    say(f"cost  vp_render_frames_stats         wall ms {mmm(x[0] for x in a)}   render kernel ms {mmm(x[1] for x in a)}   launches {a[0][2]}")
    say(f"cost  vp_render_frames_halves_stats  wall ms {mmm(x[0] for x in b)}   render kernel ms {mmm(x[1] for x in b)}   launches {b[0][2]}")
    wa, wb = statistics.median(x[0] for x in a), statistics.median(x[0] for x in b)
    ka, kb = statistics.median(x[1] for x in a), statistics.median(x[1] for x in b)
    floor = max(spread(x[0] for x in a), spread(x[0] for x in b))
    diff = 100.0 * (wb / wa - 1)
    say(f"cost  halves against _stats, medians: wall {wb - wa:+.2f} ms ({diff:+.2f} %), render kernel {100.0 * (kb / ka - 1):+.2f} %;"
        f" wall minus render kernel (reduce, memsets, host): _stats {wa - ka:.2f} ms, halves {wb - kb:.2f} ms;"
        f" spread of the alternation (max - min over median): _stats wall {spread(x[0] for x in a):.2f} %, halves wall {spread(x[0] for x in b):.2f} %"
        f" -- the difference is {'INSIDE' if abs(diff) <= floor else 'OUTSIDE'} the spread")

    # ---- returns: Q frames, the three images against a many-frame mean under other keys
    vp.set_rng(RNG, REF_KEY)
    ref = vp.DeviceBuffer(W, H)
    vp.render_frames(ref.ptr, 0, args.ref_frames, P)
    vp.scale(ref.ptr, ref.ptr, npix, 1.0 / args.ref_frames)
    ref_img = ref.download()
    vp.set_rng(RNG, KEY)
    whole, wrec, dst, ta, tb = vp.DeviceBuffer(W, H), vp.StatsBuffer(W, H), vp.DeviceBuffer(W, H), vp.DeviceBuffer(W, H), vp.DeviceBuffer(W, H)
    resid = vp.lib().vp_malloc(npix * 4)
    vp.render_frames_stats(whole.ptr, wrec.ptr, 0, Q, P)
    buf.reset(); half1.reset(); rec[0].reset(); rec[1].reset()
    vp.render_frames_halves_stats(buf.ptr, half1.ptr, rec[0].ptr, rec[1].ptr, 0, Q, P)
    vp.scale_by_count(dst.ptr, whole.ptr, wrec.ptr, npix, 1.0)
    noisy = rel_l2(dst.download(), ref_img)
    say(f"returns  {spec}: {Q} frames ({(Q + 1) // 2} + {Q // 2} in the halves), reference {args.ref_frames} frames under other keys")
    for R, F, k in PARAMS:
        vp.denoise(dst.ptr, whole.ptr, wrec.ptr, W, H, R, F, k)
        self_guided = rel_l2(dst.download(), ref_img)
        t_cross = timed(lambda: vp.denoise_cross(dst.ptr, resid, buf.ptr, rec[0].ptr, half1.ptr, rec[1].ptr, ta.ptr, tb.ptr, W, H, R, F, k))[0]
        img = dst.download()
        cross = rel_l2(img, ref_img)
        rmap = np.empty((H, W), np.float32)
        vp.lib().vp_download(rmap.ctypes.data, resid, npix * 4)
        lum = lambda v: 0.2126 * v[..., 0].astype(np.float64) + 0.7152 * v[..., 1] + 0.0722 * v[..., 2]
        true_rel = np.abs(lum(img) - lum(ref_img)) / np.maximum(lum(ref_img), 1e-3)
        say(f"returns  {spec} ({R}, {F}, {k}): rel L2 plain mean {noisy:.4f} -> vp_denoise self-guided {self_guided:.4f} ({self_guided / noisy:.2f} x)"
            f" -> cross-filtered {cross:.4f} ({cross / noisy:.2f} x): cross is {'BETTER' if cross < self_guided else 'NOT better'} than self-guided;"
            f" residual map mean {float(rmap.mean()):.4f}, root mean square {float(np.sqrt((rmap.astype(np.float64) ** 2).mean())):.4f}"
            f" against the true relative luminance error's root mean square {float(np.sqrt((true_rel ** 2).mean())):.4f};"
            f" the three calls of the cross-filter (wall, first call) {t_cross:.2f} ms")
    vp.lib().vp_free(resid)

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
    for x in (buf, half1, rec[0], rec[1], ref, whole, wrec, dst, ta, tb):
        x.free()
