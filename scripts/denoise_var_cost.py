"""What the variance stage of the cross-filter costs and what it returns (development tool; the bench is bench.py):

    python scripts/denoise_var_cost.py c2,c4f [--frames 16] [--ref-frames 1024] [--params 5:1:0.45,10:3:0.45] [--var-params 1:3:0.45,10:3:0.45]
                                       [--repeat 21] [--plain-repeat 5] [--out FILE]

A workload is a bench workload of volpath/scene.py at its own image size (c2: 800 x 600, c4f: 1280 x 720).  Per workload, on the two
halves of --frames frames (vp_render_frames_halves_stats):

  cost     vp_halves_variance; vp_filter_variance at each of --var-params, the tiled form (0) against the plain one (1), alternated;
           vp_denoise_var against vp_denoise_guided at each of --params, form 0, alternated, one half with the other as guide.  HIP
           events on the context's stream round each warm call; min / median / max in ms, and the spread (max - min over the median).
  returns  relative L2 of the RGB mean image against the mean of --ref-frames frames under OTHER keys -- the reference and the keys of
           denoise_cross_cost.py's table --: plain mean, vp_denoise self-guided on all the frames, the cross-filter, the cross-filter
           with the pooled variance alone (the variance pass at radius 0) and with the stage at the first of --var-params."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-volpath_amd"))

ap = argparse.ArgumentParser()
ap.add_argument("workloads")
ap.add_argument("--frames", type=int, default=16)
ap.add_argument("--ref-frames", type=int, default=1024)
ap.add_argument("--params", default="5:1:0.45,10:3:0.45")
ap.add_argument("--var-params", default="1:3:0.45,10:3:0.45")
ap.add_argument("--repeat", type=int, default=21)
ap.add_argument("--plain-repeat", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
out_file = open(args.out, "a") if args.out else None
KEY, REF_KEY = (0x9E3779B9, 0x85EBCA6B), (0x1234567, 0x7654321)
parse = lambda s: [(int(r), int(f), float(k)) for r, f, k in (p.split(":") for p in s.split(","))]
PARAMS, VAR_PARAMS = parse(args.params), parse(args.var_params)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import volpath as vp  # noqa: E402
from volpath import scene  # noqa: E402

RNG = int(os.environ.get("VP_PERF_RNG", vp.RNG_PHILOX7))


def say(*a):
    line = " ".join(str(v) for v in a)
    print(line, flush=True)
    if out_file:
        out_file.write(line + "\n"); out_file.flush()


def mmm(v):
    return "%.3f / %.3f / %.3f (spread %.1f %%)" % (min(v), statistics.median(v), max(v), 100.0 * (max(v) - min(v)) / statistics.median(v))


def rel_l2(img, ref):
    a, b = img[..., :3].astype(np.float64), ref[..., :3].astype(np.float64)
    return float(np.sqrt(((a - b) ** 2).sum() / (b ** 2).sum()))


if not torch.cuda.is_available():
    raise SystemExit("denoise_var_cost.py needs a GPU: there is nothing to time without one")
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


def alternated(calls, repeat):
    """each call once to warm it, then `repeat` rounds of all of them in turn: {name: [ms]}"""
    for _, c in calls:
        c()
    vp.synchronize()
    ms = {n: [] for n, _ in calls}
    for _ in range(repeat):
        for n, c in calls:
            ms[n].append(timed(c))
    return ms


class Floats:
    def __init__(self, n):
        self.ptr = vp.lib().vp_malloc(n * 4)
        assert self.ptr

    def free(self):
        vp.lib().vp_free(self.ptr)


for wl in args.workloads.split(","):
    N = args.frames
    P, info = scene.setup(wl, rng_mode=RNG, key=REF_KEY, last_frame=max(N, args.ref_frames), sunsky=sky)
    W, H = P.width, P.height
    npix = W * H
    ref = vp.DeviceBuffer(W, H)
    vp.render_frames(ref.ptr, 0, args.ref_frames, P)
    vp.scale(ref.ptr, ref.ptr, npix, 1.0 / args.ref_frames)
    ref_img = ref.download()
    vp.set_rng(RNG, KEY)
    whole, wrec = vp.DeviceBuffer(W, H), vp.StatsBuffer(W, H)
    h = (vp.DeviceBuffer(W, H), vp.DeviceBuffer(W, H))
    rec = (vp.StatsBuffer(W, H), vp.StatsBuffer(W, H))
    dst, ta, tb = vp.DeviceBuffer(W, H), vp.DeviceBuffer(W, H), vp.DeviceBuffer(W, H)
    u, q, uf, uf1 = Floats(npix), Floats(npix), Floats(npix), Floats(npix)
    vp.render_frames_stats(whole.ptr, wrec.ptr, 0, N, P)
    vp.render_frames_halves_stats(h[0].ptr, h[1].ptr, rec[0].ptr, rec[1].ptr, 0, N, P)
    say(f"== {wl}: {W}x{H}, {N} frames ({(N + 1) // 2} + {N // 2} in the halves), reference {args.ref_frames} frames under other keys;"
        f" {args.repeat} warm calls each, the plain form {args.plain_repeat} (min / median / max in ms, HIP events)")

    # ---- cost
    ms = alternated([("pool", lambda: vp.halves_variance(u.ptr, q.ptr, rec[0].ptr, rec[1].ptr, npix))], args.repeat)
    say(f"cost  {wl}  vp_halves_variance  {mmm(ms['pool'])}")
    host_u = np.empty((H, W), np.float32)
    vp.lib().vp_download(host_u.ctypes.data, u.ptr, npix * 4)
    say(f"cost  {wl}  u != 0 on {float((host_u != 0).mean()):.3f} of the pixels")
    for R, F, k in VAR_PARAMS:
        def run(form, d, R=R, F=F, k=k):
            vp.set_denoise_form(form)
            vp.filter_variance(d.ptr, u.ptr, q.ptr, W, H, R, F, k)
        ms = alternated([("tiled", lambda: run(0, uf)), ("plain", lambda: run(1, uf1))], args.plain_repeat)
        a, b = np.empty((H, W), np.float32), np.empty((H, W), np.float32)
        vp.lib().vp_download(a.ctypes.data, uf.ptr, npix * 4)
        vp.lib().vp_download(b.ctypes.data, uf1.ptr, npix * 4)
        vp.set_denoise_form(0)
        t0 = alternated([("tiled", lambda: run(0, uf))], args.repeat)["tiled"]
        say(f"cost  {wl}  vp_filter_variance ({R}, {F}, {k})  tiled {mmm(t0)}   alternated with plain: tiled {mmm(ms['tiled'])}   plain {mmm(ms['plain'])}"
            f"   plain / tiled {statistics.median(ms['plain']) / statistics.median(ms['tiled']):.1f} x   same bytes: {a.tobytes() == b.tobytes()}")
    vp.set_denoise_form(0)
    vR, vF, vk = VAR_PARAMS[0]
    vp.filter_variance(uf.ptr, u.ptr, q.ptr, W, H, vR, vF, vk)
    for R, F, k in PARAMS:
        kw = dict(guide_ptr=h[1].ptr, guide_stats_ptr=rec[1].ptr)
        ms = alternated([("guided", lambda: vp.denoise_guided(ta.ptr, h[0].ptr, rec[0].ptr, W, H, (), R, F, k, **kw)),
                         ("var", lambda: vp.denoise_var(tb.ptr, h[0].ptr, rec[0].ptr, W, H, uf.ptr, (), R, F, k, **kw))], args.repeat)
        mg, mv = statistics.median(ms["guided"]), statistics.median(ms["var"])
        say(f"cost  {wl}  ({R}, {F}, {k}) one half, the other as guide: vp_denoise_guided {mmm(ms['guided'])}   vp_denoise_var {mmm(ms['var'])}"
            f"   var against guided, medians {100.0 * (mv / mg - 1):+.1f} %")

    # ---- returns
    vp.scale_by_count(dst.ptr, whole.ptr, wrec.ptr, npix, 1.0)
    noisy = rel_l2(dst.download(), ref_img)
    for R, F, k in PARAMS:
        vp.denoise(dst.ptr, whole.ptr, wrec.ptr, W, H, R, F, k)
        self_guided = rel_l2(dst.download(), ref_img)
        cross_args = (dst.ptr, None, h[0].ptr, rec[0].ptr, h[1].ptr, rec[1].ptr, ta.ptr, tb.ptr, W, H, R, F, k)
        vp.denoise_cross(*cross_args)
        cross = rel_l2(dst.download(), ref_img)
        vp.denoise_cross(*cross_args, variance=(0, vF, vk), var_ptrs=(u.ptr, q.ptr, uf.ptr))
        pooled = rel_l2(dst.download(), ref_img)
        vp.denoise_cross(*cross_args, variance=(vR, vF, vk), var_ptrs=(u.ptr, q.ptr, uf.ptr))
        stage = rel_l2(dst.download(), ref_img)
        best = min(self_guided, cross, pooled, stage)
        say(f"returns  {wl} ({R}, {F}, {k}): rel L2 plain mean {noisy:.4f} | self-guided {self_guided:.4f} | cross {cross:.4f} | cross, pooled variance {pooled:.4f}"
            f" | cross, pooled + filtered ({vR}, {vF}, {vk}) {stage:.4f} | the stage is {'BETTER' if stage < cross else 'NOT better'} than the cross-filter"
            f" and {'BETTER' if stage < self_guided else 'NOT better'} than self-guided; best: "
            + ("self-guided" if best == self_guided else "cross" if best == cross else "pooled" if best == pooled else "pooled + filtered"))
    for x in (ref, whole, wrec, h[0], h[1], rec[0], rec[1], dst, ta, tb, u, q, uf, uf1):
        x.free()
