"""What the NL-means filter of the output stage costs and returns (development tool; the bench is bench.py):

    python scripts/denoise_cost.py c2,c4f [--frames 16,64] [--ref-frames 1024] [--params 5:1:0.45,10:3:0.45] [--repeat 21] [--out FILE]

A workload is a bench workload of volpath/scene.py at its own image size (c2: 800 x 600, c4f: 1280 x 720).  Per workload and frame
count: vp_render_frames_stats of the frames, then per parameter set (radius:patch:k; the CLI defaults and the paper's 10:3:0.45
unless told otherwise)

  time     vp_denoise in both forms (0 tiled through LDS, 1 one thread per pixel from global memory), alternated, after a warm call
           of each: HIP events around ONE call on the context's stream (a torch stream handed to vp_set_stream), min / median / max
           over --repeat calls; and whether the two forms wrote the same bytes
  returns  relative L2 of the RGB mean image against the mean of --ref-frames frames under OTHER keys: the plain mean
           (vp_scale_by_count) and the filtered one; and the same for the cross-filtered pair of half-buffers (even frames in one,
           odd frames in the other, each filtered with the other as its guide, then averaged)
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-volpath_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import volpath as vp  # noqa: E402
from volpath import scene  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("workloads")
ap.add_argument("--frames", default="16,64")
ap.add_argument("--ref-frames", type=int, default=1024)
ap.add_argument("--params", default="5:1:0.45,10:3:0.45")
ap.add_argument("--repeat", type=int, default=21)
ap.add_argument("--out", default=None)
args = ap.parse_args()
out_file = open(args.out, "a") if args.out else None
KEY, REF_KEY = (0x9E3779B9, 0x85EBCA6B), (0x1234567, 0x7654321)
RNG = int(os.environ.get("VP_PERF_RNG", vp.RNG_PHILOX7))
PARAMS = [(int(r), int(f), float(k)) for r, f, k in (p.split(":") for p in args.params.split(","))]


def say(*a):
    line = " ".join(str(v) for v in a)
    print(line, flush=True)
    if out_file:
        out_file.write(line + "\n"); out_file.flush()


def mmm(v):
    return "%.3f / %.3f / %.3f" % (min(v), statistics.median(v), max(v))


def rel_l2(img, ref):
    a, b = img[..., :3].astype(np.float64), ref[..., :3].astype(np.float64)
    return float(np.sqrt(((a - b) ** 2).sum() / (b ** 2).sum()))


if not torch.cuda.is_available():
    raise SystemExit("denoise_cost.py needs a GPU: there is nothing to time without one")
torch.cuda.set_device(0)
vp.set_device(0)
stream = torch.cuda.Stream()
vp.set_stream(stream.cuda_stream)
sky = scene.default_sunsky()
for wl in args.workloads.split(","):
    counts = [int(v) for v in args.frames.split(",")]
    P, info = scene.setup(wl, rng_mode=RNG, key=REF_KEY, last_frame=max(max(counts), args.ref_frames), sunsky=sky)
    W, H = P.width, P.height
    npix = W * H
    ref = vp.DeviceBuffer(W, H)
    vp.render_frames(ref.ptr, 0, args.ref_frames, P)
    vp.scale(ref.ptr, ref.ptr, npix, 1.0 / args.ref_frames)
    ref_img = ref.download()
    vp.set_rng(RNG, KEY)
    buf, stats, dst, dst1 = vp.DeviceBuffer(W, H), vp.StatsBuffer(W, H), vp.DeviceBuffer(W, H), vp.DeviceBuffer(W, H)
    half = [(vp.DeviceBuffer(W, H), vp.StatsBuffer(W, H)) for _ in range(2)]
    say(f"== {wl}: {W}x{H}, reference {args.ref_frames} frames under other keys, {args.repeat} timed calls per form (min / median / max)")
    for N in counts:
        buf.reset(); stats.reset()
        vp.render_frames_stats(buf.ptr, stats.ptr, 0, N, P)
        for h in half:
            h[0].reset(); h[1].reset()
        for f in range(N):
            vp.render_frames_stats(half[f & 1][0].ptr, half[f & 1][1].ptr, f, 1, P)
        vp.scale_by_count(dst.ptr, buf.ptr, stats.ptr, npix, 1.0)
        noisy = rel_l2(dst.download(), ref_img)
        rec = stats.download()
        nd = rec["n"].astype(np.float64)
        measured = int((nd * rec["sum_y2"] - rec["sum_y"] * rec["sum_y"] > 0).sum())
        say(f"{wl} {N:3d} frames: plain mean rel L2 {noisy:.4f}; {measured} of {npix} pixels have a variance > 0 (the rest is returned unfiltered)")
        for R, F, k in PARAMS:
            ms = {0: [], 1: []}
            imgs = {}
            for form in (0, 1):             # warm: code objects loaded, caches in their steady state
                vp.set_denoise_form(form)
                vp.denoise((dst, dst1)[form].ptr, buf.ptr, stats.ptr, W, H, R, F, k)
            vp.synchronize()
            for _ in range(args.repeat):
                for form in (0, 1):         # (the forms alternate)
                    vp.set_denoise_form(form)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    vp.denoise((dst, dst1)[form].ptr, buf.ptr, stats.ptr, W, H, R, F, k)
                    e1.record(stream)
                    e1.synchronize()
                    ms[form].append(e0.elapsed_time(e1))
            for form in (0, 1):
                imgs[form] = (dst, dst1)[form].download()
            vp.set_denoise_form(0)
            same = imgs[0].tobytes() == imgs[1].tobytes()
            m0, m1 = statistics.median(ms[0]), statistics.median(ms[1])
            say(f"{wl} {N:3d} frames ({R}, {F}, {k}): time   tiled ms {mmm(ms[0])}   plain ms {mmm(ms[1])}   plain / tiled {m1 / m0:.2f}"
                + ("" if same else "   THE FORMS DIFFER"))
            # the cross-filtered pair: each half with the other as its guide, then their average
            vp.denoise(dst.ptr, half[0][0].ptr, half[0][1].ptr, W, H, R, F, k, guide_ptr=half[1][0].ptr, guide_stats_ptr=half[1][1].ptr)
            vp.denoise(dst1.ptr, half[1][0].ptr, half[1][1].ptr, W, H, R, F, k, guide_ptr=half[0][0].ptr, guide_stats_ptr=half[0][1].ptr)
            vp.accumulate(dst.ptr, dst1.ptr, npix)
            vp.scale(dst.ptr, dst.ptr, npix, 0.5)
            cross = rel_l2(dst.download(), ref_img)
            den = rel_l2(imgs[0], ref_img)
            say(f"{wl} {N:3d} frames ({R}, {F}, {k}): returns   rel L2 plain mean {noisy:.4f} -> filtered {den:.4f} ({den / noisy:.2f} x)"
                f" -> cross-filtered halves {cross:.4f} ({cross / noisy:.2f} x)")
    for b in (ref, buf, stats, dst, dst1, half[0][0], half[0][1], half[1][0], half[1][1]):
        b.free()
