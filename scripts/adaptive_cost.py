"""What per-pixel statistics and adaptive sampling cost and return (development tool; the bench is bench.py):

    python scripts/adaptive_cost.py c2,c4f,c2:aa4 [--frames 1024] [--repeat 3] [--parts stats,rounds,returns]
                                    [--rounds 16,32,64,128,256] [--tols 0.05,0.02] [--round 32] [--ref-frames 4096]
                                    [--parent-tree DIR] [--out FILE]

A workload is a bench workload of volpath/scene.py, optionally with a sub-pixel factor (c2:aa4).  Every time is given as
min / median / max over the repeats; the variants of a part alternate inside one process.  Wall time is taken around a
synchronise, kernel time is the library's HIP-event time of the render launches (vp_render_time_ms: without the reduces and the
compactions).

  stats    vp_render_frames_stats against vp_render_frames, alternated; with --parent-tree (a built cuda-volpath_amd directory of
           the parent commit: its library and its Python package) also that build's vp_render_frames, in child processes before and
           after (the accumulator hashes must agree)
  rounds   what a round costs beyond its samples: vp_render_adaptive with a min_frames no pixel reaches, so that every pixel
           receives every frame, against ONE vp_render_frames_stats call of the same frames -- the difference is the compaction,
           the count read-back and the launch tail every serial round pays; per round size, as ms per round and share of the call
  returns  at each tolerance: samples and time over the uniform render's, and the error at an equal budget -- against a uniform
           reference of --ref-frames frames under other keys, the adaptive image (vp_scale_by_count) and a uniform render of the
           same total sample count rounded up to whole frames: relative RMS error and 99th-percentile per-pixel relative error of
           the luminance, relative to max(reference, 1e-3)
"""
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
ap.add_argument("--parts", default="stats,rounds,returns")
ap.add_argument("--rounds", default="16,32,64,128,256")
ap.add_argument("--tols", default="0.05,0.02")
ap.add_argument("--round", type=int, default=32)
ap.add_argument("--min-spp", type=int, default=16)
ap.add_argument("--ref-frames", type=int, default=4096)
ap.add_argument("--parent-tree", default=None)
ap.add_argument("--out", default=None)
ap.add_argument("--plain-child", action="store_true", help=argparse.SUPPRESS)   # the child process of --parent-tree
args = ap.parse_args()
out_file = open(args.out, "a") if args.out else None
KEY, REF_KEY = (0x9E3779B9, 0x85EBCA6B), (0x1234567, 0x7654321)
FLOOR = 1e-3


def say(*a):
    line = " ".join(str(v) for v in a)
    print(line, flush=True)
    if out_file:
        out_file.write(line + "\n"); out_file.flush()


def mmm(v):
    return "%.2f / %.2f / %.2f" % (min(v), statistics.median(v), max(v))


def timed(fn):
    """(wall ms around a synchronise, kernel ms by HIP events, launches, what fn returned)"""
    vp.synchronize(); vp.render_time_ms()
    t = time.perf_counter()
    r = fn()
    vp.synchronize()
    wall = (time.perf_counter() - t) * 1e3
    ms, n = vp.render_time_ms()
    return wall, ms, n, r


def lum(img):
    return 0.2126 * img[..., 0].astype(np.float64) + 0.7152 * img[..., 1] + 0.0722 * img[..., 2]


def errors(img, ref):
    rel = np.abs(lum(img) - lum(ref)) / np.maximum(lum(ref), FLOOR)
    return float(np.sqrt(np.mean(rel * rel))), float(np.percentile(rel, 99))


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
    wl, _, aa = spec.partition(":aa")
    s = int(aa) if aa else 1
    P, info = scene.setup(wl, rng_mode=int(os.environ.get("VP_PERF_RNG", vp.RNG_PHILOX7)), key=KEY, last_frame=max(args.frames, args.ref_frames), sunsky=sky)
    vp.set_subpixel(s)
    W, H, N = P.width, P.height, args.frames
    npix = W * H
    buf = vp.DeviceBuffer(W, H)
    vp.prepare(P); vp.reserve_frames(P, N)
    vp.render_frames(buf.ptr, 0, 2, P); vp.synchronize()

    def plain():
        buf.reset()
        return timed(lambda: vp.render_frames(buf.ptr, 0, N, P))

    def with_stats():
        buf.reset(); stats.reset()
        return timed(lambda: vp.render_frames_stats(buf.ptr, stats.ptr, 0, N, P))

    if args.plain_child:
        t = [plain()[:2] for _ in range(args.repeat)]
        print(json.dumps({"times": t, "hash": sha(buf.download())}))
        continue
    stats = vp.StatsBuffer(W, H)
    vp.render_frames_stats(buf.ptr, stats.ptr, 0, 2, P); vp.synchronize()
    say(f"== {spec}: {W}x{H}, {N} frames, {args.repeat} repeats (min / median / max)")
    if "stats" in args.parts:
        before = parent_child(spec, args.parent_tree) if args.parent_tree else None
        a, b = [], []
        for _ in range(args.repeat):
            a.append(plain()); ha = sha(buf.download())
            b.append(with_stats()); hb = sha(buf.download())
        after = parent_child(spec, args.parent_tree) if args.parent_tree else None
        say(f"stats   vp_render_frames        wall ms {mmm([x[0] for x in a])}   kernel ms {mmm([x[1] for x in a])}   image {ha}")
        say(f"stats   vp_render_frames_stats  wall ms {mmm([x[0] for x in b])}   kernel ms {mmm([x[1] for x in b])}   image {hb}")
        say("stats   difference of the medians: wall %+.2f ms, kernel %+.2f ms" % (
            statistics.median(x[0] for x in b) - statistics.median(x[0] for x in a), statistics.median(x[1] for x in b) - statistics.median(x[1] for x in a)))
        if before:
            t = before["times"] + after["times"]
            say(f"stats   parent build, vp_render_frames (child processes before and after)  wall ms {mmm([x[0] for x in t])}   kernel ms {mmm([x[1] for x in t])}"
                f"   image {before['hash']}" + ("" if before["hash"] == after["hash"] == ha else "   IMAGES DIFFER"))
    uniform_wall = None
    if "rounds" in args.parts or "returns" in args.parts:
        u = [with_stats() for _ in range(args.repeat)]
        uniform_wall = statistics.median(x[0] for x in u)
        say(f"uniform vp_render_frames_stats, one call: wall ms {mmm([x[0] for x in u])}   kernel ms {mmm([x[1] for x in u])}")
    if "rounds" in args.parts:
        sizes = [int(v) for v in args.rounds.split(",")]
        t = {B: [] for B in sizes}
        for _ in range(args.repeat):
            for B in sizes:       # (the sizes alternate)
                buf.reset(); stats.reset()
                t[B].append(timed(lambda: vp.render_adaptive(buf.ptr, stats.ptr, 0, N, P, 0.0, FLOOR, 1 << 30, B)))
                assert t[B][-1][3]["samples"] == npix * N
        for B in sizes:
            k = (N + B - 1) // B
            w = statistics.median(x[0] for x in t[B])
            say(f"rounds  B = {B:4d}: {k:3d} rounds, every pixel every frame   wall ms {mmm([x[0] for x in t[B]])}   kernel ms {mmm([x[1] for x in t[B]])}"
                f"   beyond the uniform call: {(w - uniform_wall) / k:+.3f} ms per round, {100.0 * (w - uniform_wall) / w:+.1f} % of the call")
    if "returns" in args.parts:
        ref = vp.DeviceBuffer(W, H)
        vp.set_rng(int(os.environ.get("VP_PERF_RNG", vp.RNG_PHILOX7)), REF_KEY)
        vp.render_frames(ref.ptr, 0, args.ref_frames, P)
        vp.scale(ref.ptr, ref.ptr, npix, 1.0 / args.ref_frames)
        ref_img = ref.download()
        ref.free()
        vp.set_rng(int(os.environ.get("VP_PERF_RNG", vp.RNG_PHILOX7)), KEY)
        full = None
        for tol in [float(v) for v in args.tols.split(",")]:
            t = []
            for _ in range(args.repeat):
                buf.reset(); stats.reset()
                t.append(timed(lambda: vp.render_adaptive(buf.ptr, stats.ptr, 0, N, P, tol, FLOOR, args.min_spp, args.round)))
            res = t[-1][3]
            vp.scale_by_count(buf.ptr, buf.ptr, stats.ptr, npix, 1.0)
            img = buf.download()
            noise = vp.stats_rel_error(stats.ptr, W, H, FLOOR)
            n_eq = -(-res["samples"] // npix)          # the same total sample count, rounded up to whole frames
            buf.reset()
            te = timed(lambda: vp.render_frames(buf.ptr, 0, n_eq, P))
            vp.scale(buf.ptr, buf.ptr, npix, 1.0 / n_eq)
            eq_img = buf.download()
            if full is None:
                buf.reset()
                vp.render_frames(buf.ptr, 0, N, P)
                vp.scale(buf.ptr, buf.ptr, npix, 1.0 / N)
                full = errors(buf.download(), ref_img)
            w = statistics.median(x[0] for x in t)
            ea, eu = errors(img, ref_img), errors(eq_img, ref_img)
            say(f"returns tol {tol}: {res['samples']} of {npix * N} samples ({100.0 * res['samples'] / (npix * N):.1f} %), {res['rounds']} rounds of {args.round}, "
                f"{res['active_left']} pixels still active; wall ms {mmm([x[0] for x in t])} = {100.0 * w / uniform_wall:.1f} % of the uniform render's; "
                f"kernel ms {mmm([x[1] for x in t])}")
            say(f"returns tol {tol}: error against {args.ref_frames} uniform frames under other keys -- adaptive: rel RMS {ea[0]:.4f}, p99 {ea[1]:.4f}; "
                f"uniform {n_eq} frames (equal budget, {te[0]:.1f} ms): rel RMS {eu[0]:.4f}, p99 {eu[1]:.4f}; uniform {N} frames: rel RMS {full[0]:.4f}, p99 {full[1]:.4f}; "
                f"noise map: median {float(np.median(noise)):.4f}, p99 {float(np.percentile(noise, 99)):.4f}")
    vp.set_subpixel(1)
    buf.free(); stats.free()
