"""What the three volume forms cost and what the precision buys (development tool; the bench is bench.py):

    python scripts/half_volume_cost.py [c4f256,c4f] [--frames 1024] [--repeat 3] [--l2-frames 256] [--out profiles/experiments/half_volume_cost.txt]

A workload is the frame-filling cloud of volpath/scene.py (c4f: 512^3, c4f256: its 256^3 twin) at 1280 x 720, decomposition
estimator, Philox2x32-7.  Its float densities go to the device as u8 (the unit quantiser of loadBinaryFile: what --bin and the bench
use), as f32 and as f16 (float_to_half_rne), each in a context of its own, set up once.  Reported per form:

  time     kernel time of ONE launch of --frames frames (vp_render_time_ms), the forms alternated --repeat times in one process after a
           warm launch of each; Msamples/s of the median, and min / max: the spread is the noise floor of the comparison
  bytes    what the packed cells occupy on the device (vp_get_volume_info)
  L2       relative L2 of the --l2-frames mean image of u8 and of f16 against f32's under the same keys: what the precision buys
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-volpath_amd"))
import numpy as np  # noqa: E402
import volpath as vp  # noqa: E402
from volpath import host, scene  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("workloads", nargs="?", default="c4f256,c4f")
ap.add_argument("--frames", type=int, default=1024)
ap.add_argument("--repeat", type=int, default=3)
ap.add_argument("--l2-frames", type=int, default=256)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "experiments", "half_volume_cost.txt"))
args = ap.parse_args()
out_file = open(args.out, "a")
KEY = (0x9E3779B9, 0x85EBCA6B)
FORMS = ("u8", "f32", "f16")


def say(*a):
    line = " ".join(str(v) for v in a)
    print(line, flush=True)
    out_file.write(line + "\n"); out_file.flush()


def rel_l2(img, ref):
    a, b = img[..., :3].astype(np.float64), ref[..., :3].astype(np.float64)
    return float(np.sqrt(((a - b) ** 2).sum() / (b ** 2).sum()))


if vp.device_count() < 1:
    raise SystemExit("half_volume_cost.py needs a GPU: there is nothing to time without one")
vp.set_device(0)
sky = scene.default_sunsky()
for wl in args.workloads.split(","):
    cfg = scene.WORKLOADS[wl]
    vol = vp.cloud_volume(cfg["n"], cfg["seed"])
    grids = {"u8": host.quantize(vol), "f32": vol, "f16": host.float_to_half(vol)}
    ctx, info = {}, {}
    P = vp.make_param(cfg["width"], cfg["height"])
    vp.mat(P, *scene.PRESET1)
    first = 16                                             # beyond the decomposition estimator's frame-11 switch
    for f in FORMS:
        ctx[f] = vp.Context(0)
        with ctx[f]:
            vp.init_volume(grids[f], brick=cfg["brick"], linear=True)
            info[f] = vp.volume_info()
            vp.init_envmap(sky[0]); vp.set_sun(sky[1], sky[2]); vp.set_camera(scene.camera_of(cfg))
            vp.set_estimator(cfg["est"]); vp.set_rng(vp.RNG_PHILOX7, KEY)
            vp.precompute_opacity(sky[1])
    del grids, vol
    buf = vp.DeviceBuffer(P.width, P.height)
    ms, mean = {f: [] for f in FORMS}, {}
    for f in FORMS:                                        # the mean images, which also warm every context
        with ctx[f]:
            buf.reset()
            vp.render_frames(buf.ptr, first, args.l2_frames, P)
            mean[f] = buf.download() / np.float32(args.l2_frames)
            vp.render_time_ms(reset=True)
    for _ in range(args.repeat):
        for f in FORMS:                                    # (the forms alternate)
            with ctx[f]:
                buf.reset()
                vp.render_frames(buf.ptr, first, args.frames, P)
                vp.synchronize()
                ms[f].append(vp.render_time_ms(reset=True)[0])
    samples = P.width * P.height * args.frames
    say(f"== {wl}: {cfg['n']}^3 cloud, {P.width}x{P.height}, {args.frames} frames per launch, {args.repeat} alternated launches per form")
    for f in FORMS:
        med = statistics.median(ms[f])
        say(f"{wl} {f:3s}: cells {info[f]['cell_bytes']:2d} B, {info[f]['cells_bytes'] / 1e6:9.1f} MB   kernel ms min / median / max "
            f"{min(ms[f]):.1f} / {med:.1f} / {max(ms[f]):.1f}   {samples / med / 1e3:.1f} Msamples/s (spread {100 * (max(ms[f]) - min(ms[f])) / med:.1f} %)")
    say(f"{wl} relative L2 of the {args.l2_frames}-frame mean against f32's, same keys: u8 {rel_l2(mean['u8'], mean['f32']):.3e}   f16 {rel_l2(mean['f16'], mean['f32']):.3e}")
    buf.free()
    for f in FORMS:
        ctx[f].destroy()
