"""What anti-aliasing costs: kernel-time throughput of bench workloads with and without a sub-pixel factor (development tool; the
bench is bench.py):   python scripts/subpixel_cost.py c2,c4f [FRAMES] [FACTORS, e.g. 1,4] [REPEAT]
Per workload and factor: all-pixel Msamples/s by HIP-event kernel time, the pixels and the kernel time of each class (general,
light, box-missing), the general class's own rate, how the camera rays got to the medium, and a hash of the accumulator."""
import hashlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-volpath_amd"))
import volpath as vp
from volpath import scene
wls = sys.argv[1].split(",")
frames = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
factors = [int(v) for v in sys.argv[3].split(",")] if len(sys.argv) > 3 else [1, 4]
rep = int(sys.argv[4]) if len(sys.argv) > 4 else 2
vp.set_device(0)
sky = scene.default_sunsky()
for wl in wls:
    P, info = scene.setup(wl, rng_mode=int(os.environ.get("VP_PERF_RNG", vp.RNG_PHILOX7)), last_frame=frames, sunsky=sky)
    buf = vp.DeviceBuffer(P.width, P.height)
    for s in factors:
        vp.set_subpixel(s)
        vp.prepare(P)
        vp.reserve_frames(P, frames)
        vp.render_frames(buf.ptr, 0, 2, P); vp.synchronize(); vp.render_time_ms(); vp.render_class_time_ms()
        best = None
        for r in range(rep):
            buf.reset()
            vp.render_frames(buf.ptr, 0, frames, P); vp.synchronize()
            ms, n = vp.render_time_ms()
            cls, px = vp.render_class_time_ms()
            if best is None or ms < best[0]:
                best = (ms, n, cls, px)
        ms, n, cls, px = best
        h = hashlib.sha1(buf.download().tobytes()).hexdigest()[:12]
        gen = px["general"] * frames / cls["general"] / 1e3 if cls["general"] > 0 else 0.0
        print(f"{wl:6s} S={s} {frames} frames: {P.width * P.height * frames / ms / 1e3:8.1f} Msamples/s all pixels ({ms:.1f} ms, {n} launches); "
              f"pixels general/light/box-missing {px['general']}/{px['light']}/{px['misses_box']}; class ms {cls['general']:.1f}/{cls['light']:.2f}/{cls['misses_box']:.2f}; "
              f"general class {gen:8.1f} Msamples/s; approach {vp.last_approach_mode()} table {vp.last_approach_table()} light-const {int(vp.last_light_const())}; image {h}",
              flush=True)
    vp.set_subpixel(1)
    buf.free()
