"""Exact against fast arithmetic (include/volpath.h vp_set_arithmetic) on the bench workloads: accuracy and kernel-time throughput.
   python scripts/arith_fast_compare.py [tol|perf|both] [REPEAT]
tol:  per workload (c2, c3, c4s at 1024 frames, c4f at 256; Philox2x32-10, the same keys in both modes) the mean-radiance images' per-channel
      relative mean difference, ||I_f - I_e||_2 / ||I_e||_2 (the stated tolerance, include/volpath.h VP_ARITH_FAST_REL_L2) and the share of
      general-class pixels whose one-frame sample differs.
perf: Msamples/s by HIP-event kernel time at 1024 frames (c3ref on Philox2x32-7), the two modes alternated REPEAT times in this process:
      best of each and the spread of each mode's runs (the noise floor)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-volpath_amd"))
import volpath as vp
from volpath import scene

what = sys.argv[1] if len(sys.argv) > 1 else "both"
rep = int(sys.argv[2]) if len(sys.argv) > 2 else 3
vp.set_device(0)
sky = scene.default_sunsky()
MODES = (("exact", vp.ARITH_EXACT), ("fast", vp.ARITH_FAST))


def render(P, n, buf):
    buf.reset()
    vp.render_frames(buf.ptr, 0, n, P)
    vp.synchronize()
    return buf.download()


if what in ("tol", "both"):
    for wl, frames in (("c2", 1024), ("c3", 1024), ("c4s", 1024), ("c4f", 256)):
        P, _ = scene.setup(wl, rng_mode=vp.RNG_PHILOX, last_frame=frames, sunsky=sky)
        buf = vp.DeviceBuffer(P.width, P.height)
        img, one = {}, {}
        for name, m in MODES:
            vp.set_arithmetic(m)
            img[name] = render(P, frames, buf)[..., :3].astype(np.float64) / frames
            one[name] = render(P, 1, buf)
        vp.set_arithmetic(vp.ARITH_EXACT)
        buf.free()
        gen = vp.pixel_table(P)[..., 5].astype(int) == 0
        ie, im = img["exact"], img["fast"]
        dmean = (im.mean(axis=(0, 1)) - ie.mean(axis=(0, 1))) / ie.mean(axis=(0, 1))
        l2 = np.linalg.norm(im - ie) / np.linalg.norm(ie)
        changed = np.any(one["exact"][gen] != one["fast"][gen], axis=-1).mean()
        print(f"tol {wl:4s} N={frames:4d}: mean rel diff (r,g,b) = {dmean[0]:+.2e} {dmean[1]:+.2e} {dmean[2]:+.2e}; "
              f"rel L2 = {l2:.4e}; general pixels changed after one frame = {100 * changed:.1f} % of {int(gen.sum())}", flush=True)

if what in ("perf", "both"):
    frames = 1024
    for wl, rng in (("c2", vp.RNG_PHILOX), ("c3", vp.RNG_PHILOX), ("c3ref", vp.RNG_PHILOX7), ("c4s", vp.RNG_PHILOX), ("c4f", vp.RNG_PHILOX)):
        P, _ = scene.setup(wl, rng_mode=rng, last_frame=frames, sunsky=sky)
        buf = vp.DeviceBuffer(P.width, P.height)
        runs = {"exact": [], "fast": []}
        appr = {}
        for name, m in MODES:   # warm-up: tables, staging, code objects
            vp.set_arithmetic(m)
            render(P, 2, buf)
        vp.render_time_ms()
        for r in range(rep):
            for name, m in (MODES if r % 2 == 0 else MODES[::-1]):
                vp.set_arithmetic(m)
                render(P, frames, buf)
                ms, n = vp.render_time_ms()
                runs[name].append(P.width * P.height * frames / ms / 1e3)
                appr[name] = vp.last_approach_mode()
        vp.set_arithmetic(vp.ARITH_EXACT)
        buf.free()
        e, f = np.array(runs["exact"]), np.array(runs["fast"])
        print(f"perf {wl:5s} {frames} frames: exact {e.max():8.1f} Ms/s (spread {100 * (e.max() - e.min()) / e.max():.2f} %)  "
              f"fast {f.max():8.1f} Ms/s (spread {100 * (f.max() - f.min()) / f.max():.2f} %)  fast/exact {f.max() / e.max():.4f}  "
              f"runs exact {np.round(e, 1).tolist()} fast {np.round(f, 1).tolist()}  approach mode exact {appr['exact']} fast {appr['fast']}",
              flush=True)
