"""What vp_render_frames_layers and vp_composite must produce (include/volpath.h), from the CPU oracle alone.
A helper, not a test.

The expectation is built sample by sample with vpo_render_sample and its vpo_counters:

    a sample is UNSCATTERED iff its `scatters` counter is 0;
    fg sample    = the oracle's sample on the real scene, RGB zeroed where unscattered;
    trans sample = where unscattered (rgb of the oracle's sample on the UNIT-BACKGROUND TWIN, 1), else (0, 0, 0, 0);

the twin being the same scene with every environment texel 1, sun_power_original = (1, 1, 1) set after vpo_set_sun (sun_dir and
sun_power untouched) and brightness 1: with the passive environment none of the three influences a draw, so the twin's sample follows
the same path and, unscattered, is max(thr, 0).  Sums run in frame order in float32, like the accumulators.

The limit of `scatters == 0`: the definition says "reaches the environment with no scatter event".  A path that the reference's loop
cap (800 segments) ends before it leaves the box, without a scatter, is NOT unscattered by the definition (fg is its beauty sample,
trans is 0), but has `scatters == 0` here.  No scene of these tests comes near that cap (a ray of 40 box lengths under the restart
estimators); a scene that did would need the classification refined."""
import ctypes as C
import math

import numpy as np

import scenes

F32 = np.float32

# ---- the scenes of tests/test_layers_cpu.py and tests/test_layers_gpu.py (the smallest that reach every branch)
W, H = 16, 12
FRAMES = (10, 11)                 # they straddle the decomposition estimator's switch to the optical-depth table
LONG = tuple(range(10, 80))       # one launch of 70 frames: the approach walks and the constant rows run
ENV = scenes.synthetic_env()
KEY = (11, 22)
JULIA_KW = dict(density=60.0, g=0.877, brightness=1.7)       # thin enough that some pixels scatter in one frame and not in the other
SOFT_KW = dict(density=3.0, g=0.6, brightness=1.7, sigma_t=(1.0, 0.8, 0.55), albedo=(0.9, 0.8, 0.95))   # chromatic: thr is not 1


def soft_grid():
    """13 x 9 x 7 floats: random soft densities, nowhere empty"""
    rng = np.random.default_rng(26)
    return np.ascontiguousarray((rng.random((7, 9, 13), dtype=np.float32) ** 2).astype(np.float32))


def grid_of(name, oracle):
    """julia: 32^3 uchar; soft: the float volume; soft16: the same rounded to binary16"""
    if name == "julia":
        return oracle.julia(32)
    g = soft_grid()
    return g if name == "soft" else np.ascontiguousarray(g.astype(np.float16))


def param_kw(name):
    return JULIA_KW if name == "julia" else SOFT_KW


def scenes_for(oracle, grid, env, sun_dir, sun_power, **kw):
    """(real, twin): two OracleScenes that differ in what an unscattered path sees, and in nothing a draw depends on"""
    real = oracle.OracleScene(grid, env, sun_dir, sun_power, **kw)
    twin = oracle.OracleScene(grid, np.ones_like(np.asarray(env, F32)), sun_dir, sun_power, **kw)
    twin.S.sun_power_original[:] = (1.0, 1.0, 1.0)
    assert list(twin.S.sun_dir) == list(real.S.sun_dir) and list(twin.S.sun_power) == list(real.S.sun_power)
    return real, twin


def twin_param(oracle, P):
    Q = oracle.Param()
    C.memmove(C.byref(Q), C.byref(P), C.sizeof(Q))
    Q.brightness = 1.0
    return Q


def sample(oracle, real, twin, P, x, y, frame, Q=None):
    """(fg sample, trans sample, the real scene's sample, its counters) of one (x, y, frame)"""
    v, cnt = real.render_sample(P, x, y, frame)
    fg, tr = v.copy(), np.zeros(4, F32)
    if cnt.scatters == 0:
        t, tc = twin.render_sample(Q if Q is not None else twin_param(oracle, P), x, y, frame)
        assert tc.scatters == 0 and tc.rng_draws == cnt.rng_draws and tc.density_lookups == cnt.density_lookups, "the twin left the path"
        fg[:3] = 0.0
        tr[:3] = t[:3]
        tr[3] = 1.0
    return fg, tr, v, cnt


class Expectation:
    """fg, trans: (H, W, 4) float32 sums over `frames`; unscattered, no_lookup: (len(frames), H, W) bool per sample (no_lookup: the
    path fetched no density); miss: (H, W) bool, the camera ray misses the box; beauty: the oracle's plain accumulator of the same samples"""

    def __init__(self, oracle, real, twin, P, frames):
        W, H = P.width, P.height
        Q = twin_param(oracle, P)
        self.frames = list(frames)
        self.fg, self.trans, self.beauty = (np.zeros((H, W, 4), F32) for _ in range(3))
        self.unscattered = np.zeros((len(self.frames), H, W), bool)
        self.no_lookup = np.zeros((len(self.frames), H, W), bool)
        for n, f in enumerate(self.frames):            # frame order, float32: one addition per sample and accumulator
            for y in range(H):
                for x in range(W):
                    fg, tr, v, cnt = sample(oracle, real, twin, P, x, y, f, Q)
                    self.fg[y, x] = self.fg[y, x] + fg
                    self.trans[y, x] = self.trans[y, x] + tr
                    self.beauty[y, x] = self.beauty[y, x] + v
                    self.unscattered[n, y, x] = cnt.scatters == 0
                    self.no_lookup[n, y, x] = cnt.density_lookups == 0
        # the pixels whose camera ray misses the box (the restated camera ray through the oracle's own box test)
        self.miss = np.zeros((H, W), bool)
        m = list(real.S.inv_view)
        org = (C.c_float * 3)(m[3], m[7], m[11])
        tn, tf = C.c_float(), C.c_float()
        for y in range(H):
            for x in range(W):
                d = (C.c_float * 3)(*[float(c) for c in camera_dir(m, W, H, x, y)])
                self.miss[y, x] = not oracle.lib().vpo_intersect_box(org, d, real.S.box_min, real.S.box_max, C.byref(tn), C.byref(tf))
        for a in (self.fg, self.trans, self.beauty, self.unscattered, self.no_lookup, self.miss):
            a.setflags(write=False)

    def groups(self):
        """pixels per group: box-missing; unscattered in every frame (but tracked); scattered in every frame; mixed over the frames"""
        u_all, u_any = self.unscattered.all(0), self.unscattered.any(0)
        miss = self.miss
        assert (u_all | ~miss).all() and (self.no_lookup.all(0) | ~miss).all(), "a ray that misses the box fetches nothing and cannot scatter"
        return dict(miss=int(miss.sum()), unscattered=int((u_all & ~miss).sum()), scattered=int((~u_any).sum()), mixed=int((u_any & ~u_all).sum()))


_CACHE = {}


def expectation(oracle, key, make):
    """the Expectation of `key`, computed once per session (make() -> (real, twin, P, frames)) and read-only"""
    if key not in _CACHE:
        _CACHE[key] = Expectation(oracle, *make())
    return _CACHE[key]


def expected(oracle, name, est, rng_mode, frames=FRAMES, size=(W, H), density=None):
    """the Expectation of scene `name` (julia, soft, soft16) under (estimator, stream) on `frames`: once per session; density: another
    Param.density than the scene's own"""
    def make():
        g = grid_of(name, oracle)
        g = np.ascontiguousarray(g.astype(np.float32)) if g.dtype == np.float16 else g      # a binary16 volume renders as the widened floats
        real, twin = scenes_for(oracle, g, ENV, scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER, estimator=est, rng_mode=rng_mode, seed=KEY)
        if est == 1 and max(frames) > 10:
            real.precompute_opacity()
            twin.precompute_opacity()
        kw = dict(param_kw(name), **({} if density is None else {"density": density}))
        return real, twin, oracle.default_param(size[0], size[1], **kw), frames
    return expectation(oracle, (name, est, rng_mode, tuple(frames), tuple(size), density), make)


def composite(fg, trans, scale, plate=None, rgb=None):
    """vp_composite in float32 numpy: one multiply and one add per term, in the header's order"""
    fg, trans, s = np.asarray(fg, F32), np.asarray(trans, F32), F32(scale)
    B = np.asarray(plate, F32)[..., :3] if plate is not None else np.asarray(rgb, F32)
    out = np.empty_like(fg)
    out[..., :3] = fg[..., :3] * s + (trans[..., :3] * s) * B
    out[..., 3] = F32(1.0) - trans[..., 3] * s
    return out


def camera_dir(inv_view, W, H, x, y):
    """the oracle's camera direction of pixel (x, y) (vp_oracle.c camera_ray), restated in float32"""
    m = [F32(v) for v in inv_view]
    u = (F32(x) * F32(2.0) - F32(W)) / F32(W)
    v = (F32(y) * F32(2.0) - F32(H)) / F32(W)
    cz = F32(-1.0 / math.tan(float(F32(54.43)) * 0.00872664626))
    r = [u * m[4 * k] + v * m[4 * k + 1] + cz * m[4 * k + 2] for k in range(3)]
    inv = F32(1.0) / np.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2], dtype=F32)
    return np.array([r[0] * inv, r[1] * inv, r[2] * inv], F32)


def background(oracle, scene, d):
    """background() of an unscattered path along d on `scene`: the sun disc's value, or the environment"""
    sun = np.array(list(scene.S.sun_dir), F32)
    cos_sun = F32(94.0) / np.sqrt(F32(94.0) * F32(94.0) + F32(0.45) * F32(0.45), dtype=F32)
    if d[0] * sun[0] + d[1] * sun[1] + d[2] * sun[2] > cos_sun:
        return np.array(list(scene.S.sun_power_original), F32)
    out = (C.c_float * 3)()
    oracle.lib().vpo_eval_envmap(C.byref(scene.S), (C.c_float * 3)(*[float(c) for c in d]), out)
    return np.array(out[:], F32)
