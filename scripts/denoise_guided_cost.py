"""What the feature-guided NL-means filter costs and returns beside vp_denoise (development tool; the bench is bench.py):

    python scripts/denoise_guided_cost.py c2,c4f [--frames 16] [--ref-frames 1024] [--params 5:1:0.45,10:3:0.45]
                                          [--sigma-alpha 0.2] [--sigma-depth 0.2] [--feature-step 0.001] [--repeat 21] [--out FILE]
    python scripts/denoise_guided_cost.py c2 --against OTHER/libvolpath_hip.so [--rounds 3]

A workload is a bench workload of volpath/scene.py at its own image size (c2: 800 x 600, c4f: 1280 x 720).  Per workload:
vp_render_frames_stats of the frames and vp_render_features of the view, then per parameter set (radius:patch:k) and per form (0
tiled through LDS, 1 one thread per pixel from global memory)

  time     vp_denoise and vp_denoise_guided with the CLI's three features (alpha.y and depth.w with --sigma-alpha, depth.y with
           --sigma-depth), alternated, after a warm call of each: HIP events around ONE call on the context's stream (a torch stream
           handed to vp_set_stream), min / median / max over --repeat calls; and whether the two forms wrote the same bytes
  returns  relative L2 of the RGB mean image against the mean of --ref-frames frames under OTHER keys: the plain mean
           (vp_scale_by_count), vp_denoise's and vp_denoise_guided's

--against: vp_denoise alone (form 0), this tree's library against another build's, child process against child process, alternated
--rounds times; each child renders the frames and times --repeat warm calls per parameter set.  The other library lies in its own
build tree (cuda-volpath_amd/ with the volpath package and libvolpath_host.so beside it); VOLPATH_LIB hands it to the child.
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (a child of --against imports the volpath package that lies beside its library: an older build has fewer symbols than this tree's package binds)
sys.path.insert(0, os.path.dirname(os.path.abspath(os.environ["VOLPATH_LIB"])) if "VOLPATH_LIB" in os.environ else os.path.join(ROOT, "cuda-volpath_amd"))

ap = argparse.ArgumentParser()
ap.add_argument("workloads")
ap.add_argument("--frames", type=int, default=16)
ap.add_argument("--ref-frames", type=int, default=1024)
ap.add_argument("--params", default="5:1:0.45,10:3:0.45")
ap.add_argument("--sigma-alpha", type=float, default=0.2)
ap.add_argument("--sigma-depth", type=float, default=0.2)
ap.add_argument("--feature-step", type=float, default=0.001)
ap.add_argument("--repeat", type=int, default=21)
ap.add_argument("--out", default=None)
ap.add_argument("--against", default=None)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--child", action="store_true")
args = ap.parse_args()
out_file = open(args.out, "a") if args.out else None
KEY, REF_KEY = (0x9E3779B9, 0x85EBCA6B), (0x1234567, 0x7654321)
PARAMS = [(int(r), int(f), float(k)) for r, f, k in (p.split(":") for p in args.params.split(","))]


def say(*a):
    line = " ".join(str(v) for v in a)
    print(line, flush=True)
    if out_file:
        out_file.write(line + "\n"); out_file.flush()


def mmm(v):
    return "%.3f / %.3f / %.3f" % (min(v), statistics.median(v), max(v))


if args.against:
    # child against child, alternated: each line a child prints is "<R> <F> <min> <median> <max>"
    libs = [("this tree", os.path.join(ROOT, "cuda-volpath_amd", "libvolpath_hip.so")), ("other build", os.path.abspath(args.against))]
    res = {}
    for rnd in range(args.rounds):
        for name, path in libs:
            env = dict(os.environ, VOLPATH_LIB=path)
            cmd = [sys.executable, os.path.abspath(__file__), args.workloads, "--child", "--frames", str(args.frames), "--params", args.params,
                   "--repeat", str(args.repeat)]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
            if r.returncode:
                raise SystemExit(f"child with {path} ended with {r.returncode}: {r.stderr[-2000:]}")
            for line in r.stdout.splitlines():
                if line.startswith("T "):
                    _, wl, R, F, lo, med, hi = line.split()
                    res.setdefault((wl, int(R), int(F)), {}).setdefault(name, []).append((float(lo), float(med), float(hi)))
    say(f"== vp_denoise, form 0, {args.frames} frames: this tree's library against {args.against}, {args.rounds} child processes each, alternated;"
        f" per child {args.repeat} warm calls, min / median / max in ms")
    for (wl, R, F), by in res.items():
        for name, _ in libs:
            say(f"{wl} ({R}, {F}) {name:11s}: " + "   ".join("%.3f / %.3f / %.3f" % t for t in by[name])
                + "   median of medians %.3f" % statistics.median(t[1] for t in by[name]))
    raise SystemExit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import volpath as vp  # noqa: E402
from volpath import scene  # noqa: E402

RNG = int(os.environ.get("VP_PERF_RNG", vp.RNG_PHILOX7))


def rel_l2(img, ref):
    a, b = img[..., :3].astype(np.float64), ref[..., :3].astype(np.float64)
    return float(np.sqrt(((a - b) ** 2).sum() / (b ** 2).sum()))


if not torch.cuda.is_available():
    raise SystemExit("denoise_guided_cost.py needs a GPU: there is nothing to time without one")
torch.cuda.set_device(0)
vp.set_device(0)
stream = torch.cuda.Stream()
vp.set_stream(stream.cuda_stream)
sky = scene.default_sunsky()


def timed(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    call()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


for wl in args.workloads.split(","):
    N = args.frames
    if args.child:
        P, info = scene.setup(wl, rng_mode=RNG, key=KEY, last_frame=N, sunsky=sky)
        W, H = P.width, P.height
        buf, stats, dst = vp.DeviceBuffer(W, H), vp.StatsBuffer(W, H), vp.DeviceBuffer(W, H)
        vp.render_frames_stats(buf.ptr, stats.ptr, 0, N, P)
        for R, F, k in PARAMS:
            vp.denoise(dst.ptr, buf.ptr, stats.ptr, W, H, R, F, k)
            vp.synchronize()
            ms = [timed(lambda: vp.denoise(dst.ptr, buf.ptr, stats.ptr, W, H, R, F, k)) for _ in range(args.repeat)]
            print("T %s %d %d %.4f %.4f %.4f" % (wl, R, F, min(ms), statistics.median(ms), max(ms)), flush=True)
        for b in (buf, stats, dst):
            b.free()
        continue
    P, info = scene.setup(wl, rng_mode=RNG, key=REF_KEY, last_frame=max(N, args.ref_frames), sunsky=sky)
    W, H = P.width, P.height
    npix = W * H
    ref = vp.DeviceBuffer(W, H)
    vp.render_frames(ref.ptr, 0, args.ref_frames, P)
    vp.scale(ref.ptr, ref.ptr, npix, 1.0 / args.ref_frames)
    ref_img = ref.download()
    vp.set_rng(RNG, KEY)
    buf, stats, alpha, depth = vp.DeviceBuffer(W, H), vp.StatsBuffer(W, H), vp.DeviceBuffer(W, H), vp.DeviceBuffer(W, H)
    dst = {(g, form): vp.DeviceBuffer(W, H) for g in (0, 1) for form in (0, 1)}
    vp.render_frames_stats(buf.ptr, stats.ptr, 0, N, P)
    t_feat = timed(lambda: vp.render_features(P, args.feature_step, alpha_ptr=alpha.ptr, depth_ptr=depth.ptr))
    feats = [(alpha.ptr, 1, args.sigma_alpha), (depth.ptr, 1, args.sigma_depth), (depth.ptr, 3, args.sigma_alpha)]
    vp.scale_by_count(dst[0, 0].ptr, buf.ptr, stats.ptr, npix, 1.0)
    noisy = rel_l2(dst[0, 0].download(), ref_img)
    d_img = depth.download()
    say(f"== {wl}: {W}x{H}, {N} frames, reference {args.ref_frames} frames under other keys, {args.repeat} timed calls each (min / median / max);"
        f" features: alpha.y sigma {args.sigma_alpha}, depth.y sigma {args.sigma_depth}, depth.w sigma {args.sigma_alpha}, step {args.feature_step}")
    say(f"{wl}: plain mean rel L2 {noisy:.4f}; cover {float(d_img[..., 3].mean()):.3f}, depth.y = +inf on {float(np.isinf(d_img[..., 1]).mean()):.3f} of the pixels;"
        f" the feature pass itself (first call) {t_feat:.3f} ms")

    def run(g, form, R, F, k):
        vp.set_denoise_form(form)
        if g:
            vp.denoise_guided(dst[g, form].ptr, buf.ptr, stats.ptr, W, H, feats, R, F, k)
        else:
            vp.denoise(dst[g, form].ptr, buf.ptr, stats.ptr, W, H, R, F, k)

    for R, F, k in PARAMS:
        ms = {key: [] for key in dst}
        for key in dst:                     # warm: code objects loaded, caches in their steady state
            run(*key, R, F, k)
        vp.synchronize()
        for _ in range(args.repeat):
            for key in dst:                 # (the four calls alternate)
                ms[key].append(timed(lambda: run(*key, R, F, k)))
        vp.set_denoise_form(0)
        img = {key: b.download() for key, b in dst.items()}
        med = {key: statistics.median(v) for key, v in ms.items()}
        for form, name in ((0, "tiled"), (1, "plain")):
            say(f"{wl} ({R}, {F}, {k}) {name}: time   vp_denoise ms {mmm(ms[0, form])}   vp_denoise_guided ms {mmm(ms[1, form])}"
                f"   guided / unguided {med[1, form] / med[0, form]:.2f}")
        for g in (0, 1):
            if img[g, 0].tobytes() != img[g, 1].tobytes():
                say(f"{wl} ({R}, {F}, {k}): THE FORMS DIFFER ({'guided' if g else 'unguided'})")
        a, b = rel_l2(img[0, 0], ref_img), rel_l2(img[1, 0], ref_img)
        say(f"{wl} ({R}, {F}, {k}): returns   rel L2 plain mean {noisy:.4f} -> vp_denoise {a:.4f} ({a / noisy:.2f} x) -> vp_denoise_guided {b:.4f} ({b / noisy:.2f} x)")
    for b in [ref, buf, stats, alpha, depth] + list(dst.values()):
        b.free()
