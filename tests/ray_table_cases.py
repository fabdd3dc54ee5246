"""What tests/test_ray_table_gpu.py shares with the child processes it starts: the scene, the cameras and the renders of the per-view
ray table of the global-majorant integrator (LaunchDev::ray).  A helper, not a test.

Run as a script -- `python ray_table_cases.py OUT.npz` -- it renders every case of RENDERS on GPU 0 in the configuration its
environment asks for (VP_NO_RAY_TABLE is read when the device is first used, hence a process of its own per setting) and saves the
accumulators, the six work counters and vp_last_ray_table() of each."""
import os
import sys

import numpy as np

F32 = np.float32
N = 32                                   # Julia 32^3
SIZES = ((24, 16), (37, 19))             # 37 x 19: partial edge tiles, list slots outside the image
FIRST, NFRAMES = 9, 4                    # frames 9..12, across the decomposition estimator's frame-11 switch
DENSITY, G = 4000.0, 0.877
KEY = (3, 4)
COUNTERS = ("samples", "density_lookups", "bound_lookups", "opacity_lookups", "env_lookups", "scatters")
LA_FRAMES = 20                           # render_kernel calls per camera of the look-ahead sequence


def look_at(eye, target, up=(0.0, 1.0, 0.0)):
    """row-major 3x4 camera-to-world (kernel.cu:626): columns right, up, back, eye; the view direction is -back"""
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    back = eye - target
    back /= np.linalg.norm(back)
    right = np.cross(up, back)
    right /= np.linalg.norm(right)
    up2 = np.cross(back, right)
    return tuple(float(F32(v)) for k in range(3) for v in (right[k], up2[k], back[k], eye[k]))


def cameras(vp):
    c = {"default": tuple(vp.DEFAULT_CAMERA)}
    for n, a in enumerate((0.3, 1.9, 3.5, 5.1)):
        c[f"orbit{n}"] = look_at((3.0 * np.cos(a), 0.9 - 0.5 * n, 3.0 * np.sin(a)), (0.0, 0.0, 0.0))
    c["inside"] = look_at((0.1, 0.05, -0.2), (1.0, 0.7, 3.0))                 # every t_near < 0
    c["axis"] = look_at((0.0, 0.0, 3.0), (0.0, 0.0, 0.0))                     # u = 0 / v = 0: components +-0, reciprocals infinite
    c["partial"] = look_at((0.0, 0.0, 3.0), (1.2, 0.3, 0.0))                  # part of the image misses the box
    return c


def grid_of(kind, g):
    """the Julia set g (uchar cells: volpath.julia_volume(N) or the oracle's julia(N), the same bytes) as it is, or as binary16 cells
    (values k / 255, rounded)"""
    return g if kind == "u8" else np.ascontiguousarray((g.astype(F32) / F32(255.0)).astype(np.float16))


# name -> what differs from (global majorant, Philox2x32-7, 24 x 16, uchar volume, achromatic, default camera)
RENDERS = {
    "p7": dict(counters=True),
    "p7_37x19": dict(size=SIZES[1], counters=True),
    "p10": dict(rng=1, counters=True),
    "samplerh": dict(rng=0, counters=True),
    "chromatic": dict(chromatic=True, counters=True),
    "half": dict(volume="f16"),
    "layers": dict(layers=True),
    "fast": dict(fast=True),
    "sub2": dict(subpixel=2),
    "lookahead": dict(lookahead=True),
    "c3": dict(est=1, brick=8),                      # the decomposition estimator: untouched
    "c3ref": dict(est=1, brick=1, rng=0),
}


def scene(vp, cam=None, est=0, rng=2, brick=1, volume="u8", fast=False, subpixel=1, shard=(0, 1)):
    import scenes
    vp.set_arithmetic(vp.ARITH_FAST if fast else vp.ARITH_EXACT)
    vp.set_subpixel(subpixel)
    vp.init_volume(grid_of(volume, vp.julia_volume(N)), brick=brick, linear=True)
    vp.init_envmap(scenes.synthetic_env())
    vp.set_sun(scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER)
    vp.set_camera(tuple(vp.DEFAULT_CAMERA) if cam is None else cam)
    vp.set_estimator(est)
    vp.set_rng(rng, KEY)
    vp.set_tracking(0)
    vp.set_envmap_sampling(vp.ENV_PASSIVE)
    vp.set_exit_flights(1)
    vp.set_shard(*shard)
    vp.set_lookahead(vp.LOOKAHEAD_DEFAULT)
    vp.enable_counters(False)
    if est == vp.EST_DECOMP:
        vp.precompute_opacity(scenes.DEFAULT_SUN_DIR)


def param(mod, size, chromatic=False, layers=False):
    """the Param of a case from the library (mod = volpath: make_param) or the oracle (default_param)"""
    import scenes
    kw = dict(density=DENSITY, g=G, **({"brightness": 1.7} if layers else {}))      # (layers: tests/layers_lib.py JULIA_KW's brightness)
    P = (mod.make_param if hasattr(mod, "make_param") else mod.default_param)(size[0], size[1], **kw)
    if chromatic:
        mod.mat(P, *scenes.PRESET1)
    return P


def render(vp, name):
    """{key: array} of case `name` in the current process"""
    c = RENDERS[name]
    size = c.get("size", SIZES[0])
    scene(vp, est=c.get("est", 0), rng=c.get("rng", 2), brick=c.get("brick", 1), volume=c.get("volume", "u8"), fast=c.get("fast", False),
          subpixel=c.get("subpixel", 1))
    P = param(vp, size, c.get("chromatic", False), c.get("layers", False))
    out = {}
    buf, buf2 = vp.DeviceBuffer(*size), vp.DeviceBuffer(*size)
    try:
        if c.get("layers"):
            vp.render_frames_layers(buf.ptr, buf2.ptr, FIRST, NFRAMES, P)
            out["fg"], out["trans"] = buf.download(), buf2.download()
        elif c.get("lookahead"):
            cams = cameras(vp)
            for n, cam in enumerate((cams["default"], cams["orbit1"])):          # a camera move in the middle of the run
                vp.set_camera(cam)
                for f in range(FIRST + n * LA_FRAMES, FIRST + (n + 1) * LA_FRAMES):
                    vp.render_kernel(buf.ptr, f, P)
            vp.synchronize()
            out["img"] = buf.download()
            out["la"] = np.array(vp.lookahead_stats(), np.int64)
        else:
            vp.render_frames(buf.ptr, FIRST, NFRAMES, P)
            out["img"] = buf.download()
        out["table"] = np.array([vp.last_ray_table()], np.int64)
        if c.get("counters"):
            vp.enable_counters(True)
            vp.read_counters(reset=True)
            buf.reset()
            vp.render_frames(buf.ptr, FIRST, NFRAMES, P)
            k = vp.read_counters()
            vp.enable_counters(False)
            out["img_counting"] = buf.download()
            out["counters"] = np.array([k[q] for q in COUNTERS], np.int64)
            out["table_counting"] = np.array([vp.last_ray_table()], np.int64)
    finally:
        buf.free()
        buf2.free()
        vp.set_subpixel(1)
        vp.set_arithmetic(vp.ARITH_EXACT)
    return out


def main(path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tests"))
    sys.path.insert(0, os.path.join(root, "cuda-volpath_amd"))
    import volpath as vp
    vp.set_device(0)
    out = {}
    for name in RENDERS:
        for k, v in render(vp, name).items():
            out[f"{name}/{k}"] = v
    np.savez(path, **out)
    print("ray_table_cases: saved", len(out), "arrays")


if __name__ == "__main__":
    main(sys.argv[1])
