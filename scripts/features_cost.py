"""What the feature pass (vp_render_features) costs beside a one-frame beauty render of the same scene
(development tool; the bench is bench.py):

    python scripts/features_cost.py [c2,c4f] [--step 0.001] [--repeat 5] [--out profiles/experiments/features_cost.txt]

A workload is a bench workload of volpath/scene.py at the bench's size (c2: 800x600 Julia set, global majorant; c4f: the frame-filling
cloud at 1280x720).  The call is timed with HIP events recorded on the context's stream around it (the per-view table and the pixel
lists exist: vp_prepare ran), `repeat` times, given as min / median / max.  The same runs once more in a child process whose context
reads VP_NO_FEATURE_SKIP=1 (no class fills, no skip of the certified-empty stretch); the two results must have the same bits.  Beside
them: the kernel time of a one-frame vp_render_frames call (vp_render_time_ms) on the same scene."""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-volpath_amd"))
import numpy as np  # noqa: E402
import volpath as vp  # noqa: E402
from volpath import scene  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("workloads", nargs="?", default="c2,c4f")
ap.add_argument("--step", type=float, default=0.001)
ap.add_argument("--repeat", type=int, default=5)
ap.add_argument("--out", default=None)
ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
args = ap.parse_args()
out_file = open(args.out, "a") if args.out and not args.child else None
KEY = (0x9E3779B9, 0x85EBCA6B)
hip = C.CDLL("libamdhip64.so")


def say(*a):
    line = " ".join(str(v) for v in a)
    print(line, flush=True)
    if out_file:
        out_file.write(line + "\n"); out_file.flush()


def mmm(v):
    v = list(v)
    return "%.3f / %.3f / %.3f" % (min(v), statistics.median(v), max(v))


def event():
    e = C.c_void_p()
    assert hip.hipEventCreate(C.byref(e)) == 0
    return e


def sha(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()[:12]


def measure(spec):
    P, info = scene.setup(spec, rng_mode=vp.RNG_PHILOX7, key=KEY, last_frame=1, sunsky=sky)
    W, H = P.width, P.height
    a, d, buf = vp.DeviceBuffer(W, H), vp.DeviceBuffer(W, H), vp.DeviceBuffer(W, H)
    vp.prepare(P)
    stream = C.c_void_p(vp.lib().vp_get_stream())
    e0, e1 = event(), event()
    vp.render_features(P, args.step, alpha_ptr=a.ptr, depth_ptr=d.ptr); vp.synchronize()      # warm-up: code object, tables
    t = []
    for _ in range(args.repeat):
        assert hip.hipEventRecord(e0, stream) == 0
        vp.render_features(P, args.step, alpha_ptr=a.ptr, depth_ptr=d.ptr)
        assert hip.hipEventRecord(e1, stream) == 0
        vp.synchronize()
        ms = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
        t.append(ms.value)
    ga, gd = a.download(), d.download()
    vp.render_frames(buf.ptr, 0, 1, P); vp.synchronize(); vp.render_time_ms()                  # warm-up
    k = []
    for f in range(args.repeat):
        buf.reset()
        vp.render_frames(buf.ptr, f, 1, P); vp.synchronize()
        k.append(vp.render_time_ms()[0])
    general, light, miss = vp.pixel_lists(P)
    res = dict(W=W, H=H, features_ms=t, frame_ms=k, alpha=sha(ga), depth=sha(gd), classes=[len(general), len(light), len(miss)],
               cover=float((gd[..., 3] == 1).mean()))
    for b in (a, d, buf):
        b.free()
    return res


vp.lib().vp_get_stream.restype = C.c_void_p
vp.set_device(0)
sky = scene.default_sunsky()
if args.child:
    print(json.dumps({spec: measure(spec) for spec in args.workloads.split(",")}))
    sys.exit(0)
say(f"# vp_render_features at step {args.step}: HIP events on the context's stream around the call, {args.repeat} repeats, ms as min / median / max")
say("# git diff of this change shows nothing in vp_integrator.h, vp_dispatch.h, vp_kernels_fast.hip or the existing kernels: the beauty render")
say("# is the parent's, so it is not measured against the parent here; its one-frame kernel time stands beside the pass as a yardstick only")
r = subprocess.run([sys.executable, os.path.abspath(__file__), args.workloads, "--step", str(args.step), "--repeat", str(args.repeat), "--child"],
                   env=dict(os.environ, VP_NO_FEATURE_SKIP="1"), capture_output=True, text=True)
if r.returncode:
    raise RuntimeError("child with VP_NO_FEATURE_SKIP=1 failed: " + r.stderr[-2000:])
noskip = json.loads(r.stdout.strip().splitlines()[-1])
for spec in args.workloads.split(","):
    m, n = measure(spec), noskip[spec]
    say(f"== {spec}: {m['W']}x{m['H']}, pixel classes general / light / box-missing {m['classes']}, pixels that meet matter {100 * m['cover']:.1f} %")
    say(f"features, class fills and skip on     ms {mmm(m['features_ms'])}")
    say(f"features, VP_NO_FEATURE_SKIP=1        ms {mmm(n['features_ms'])}   ({statistics.median(n['features_ms']) / statistics.median(m['features_ms']):.2f} x)")
    say(f"one frame of vp_render_frames, kernel ms {mmm(m['frame_ms'])}   (the pass = {statistics.median(m['features_ms']) / statistics.median(m['frame_ms']):.2f} frames)")
    say("same bits with and without the shortcuts: " + ("yes" if (m["alpha"], m["depth"]) == (n["alpha"], n["depth"]) else "NO -- alpha %s/%s depth %s/%s" % (m["alpha"], n["alpha"], m["depth"], n["depth"])))
