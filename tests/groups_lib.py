"""What vp_render_frames_groups and vp_relight must produce (include/volpath.h), from the CPU oracle alone.
A helper, not a test.

The expectation is the header's equivalent form, built sample by sample with vpo_render_sample on two twins of the real scene:

    sun twin: every environment texel (0, 0, 0), everything else the real scene's  -> the sun accumulator
    sky twin: vpo_set_sun(dir, (0, 0, 0)), everything else the real scene's        -> the sky accumulator

With the passive environment neither the environment nor the sun's power influences a draw: each twin's sample must report the real
sample's rng_draws, scatters and density_lookups (asserted per sample), and all three carry the same w.  Sums run per pixel in frame
order in float32, like the accumulators.  The scenes are those of tests/layers_lib.py, whose throughputs are finite everywhere (the
equivalent form is the definition only there)."""
import numpy as np

import layers_lib as LL
import scenes

F32 = np.float32
W, H, FRAMES, LONG, ENV, KEY = LL.W, LL.H, LL.FRAMES, LL.LONG, LL.ENV, LL.KEY
ZERO = (0.0, 0.0, 0.0)
# the per-sample additivity bound of tests/test_groups_cpu.py, relative to the larger of |real| and sun + sky
ADDITIVITY = 3.0 * 2.0 ** -24


def scenes_for(oracle, grid, env, sun_dir, sun_power, **kw):
    """(real, sun twin, sky twin): three OracleScenes that differ in the lights and in nothing a draw depends on"""
    real = oracle.OracleScene(grid, env, sun_dir, sun_power, **kw)
    sun = oracle.OracleScene(grid, np.zeros_like(np.asarray(env, F32)), sun_dir, sun_power, **kw)
    sky = oracle.OracleScene(grid, env, sun_dir, ZERO, **kw)
    assert list(sun.S.sun_dir) == list(real.S.sun_dir) == list(sky.S.sun_dir) and list(sun.S.sun_power) == list(real.S.sun_power)
    assert not any(sky.S.sun_power) and not any(sky.S.sun_power_original) and not sun.env.any()
    return real, sun, sky


def sample(real, sun, sky, P, x, y, frame, base=None):
    """(sun sample, sky sample, the real scene's sample, its counters) of one (x, y, frame); base: the real scene's (sample, counters)
    where the caller has them already"""
    v, cnt = real.render_sample(P, x, y, frame) if base is None else base
    out = []
    for twin in (sun, sky):
        t, tc = twin.render_sample(P, x, y, frame)
        assert (tc.rng_draws, tc.scatters, tc.density_lookups) == (cnt.rng_draws, cnt.scatters, cnt.density_lookups), "a twin left the path"
        assert t[3] == v[3], "the twins carry the real sample's w"
        out.append(t)
    return out[0], out[1], v, cnt


class Expectation:
    """sun, sky, beauty: (H, W, 4) float32 sums over `frames`; lit_sun, lit_sky: (len(frames), H, W) bool, the sample's group RGB is
    not all zero; scattered: likewise, the path scattered; miss: (H, W) bool, the camera ray misses the box; worst: the largest
    per-sample |sun + sky - real| over max(|real|, sun + sky), per channel"""

    def __init__(self, oracle, real, sun, sky, P, frames):
        W, H = P.width, P.height
        self.frames = list(frames)
        self.sun, self.sky, self.beauty = (np.zeros((H, W, 4), F32) for _ in range(3))
        self.lit_sun, self.lit_sky, self.scattered = (np.zeros((len(self.frames), H, W), bool) for _ in range(3))
        self.worst = 0.0
        for n, f in enumerate(self.frames):            # frame order, float32: one addition per sample and accumulator
            for y in range(H):
                for x in range(W):
                    a, k, v, cnt = sample(real, sun, sky, P, x, y, f)
                    self.sun[y, x] = self.sun[y, x] + a
                    self.sky[y, x] = self.sky[y, x] + k
                    self.beauty[y, x] = self.beauty[y, x] + v
                    self.lit_sun[n, y, x] = a[:3].any()
                    self.lit_sky[n, y, x] = k[:3].any()
                    self.scattered[n, y, x] = cnt.scatters > 0
                    s64, v64 = a[:3].astype(np.float64) + k[:3].astype(np.float64), v[:3].astype(np.float64)
                    den = np.maximum(np.abs(v64), np.abs(s64))
                    if (den > 0).any():
                        self.worst = max(self.worst, float((np.abs(s64 - v64)[den > 0] / den[den > 0]).max()))
        self.miss = _miss(oracle, real, W, H)
        for a in (self.sun, self.sky, self.beauty, self.lit_sun, self.lit_sky, self.scattered, self.miss):
            a.setflags(write=False)


def _miss(oracle, real, W, H):
    """the pixels whose camera ray misses the box (layers_lib's restated camera ray through the oracle's own box test)"""
    import ctypes as C
    miss = np.zeros((H, W), bool)
    m = list(real.S.inv_view)
    org = (C.c_float * 3)(m[3], m[7], m[11])
    tn, tf = C.c_float(), C.c_float()
    for y in range(H):
        for x in range(W):
            d = (C.c_float * 3)(*[float(c) for c in LL.camera_dir(m, W, H, x, y)])
            miss[y, x] = not oracle.lib().vpo_intersect_box(org, d, real.S.box_min, real.S.box_max, C.byref(tn), C.byref(tf))
    return miss


_CACHE = {}


def expectation(oracle, key, make):
    """the Expectation of `key`, computed once per session (make() -> (real, sun, sky, P, frames)) and read-only"""
    if key not in _CACHE:
        _CACHE[key] = Expectation(oracle, *make())
    return _CACHE[key]


def expected(oracle, name, est, rng_mode, frames=FRAMES, size=(W, H), density=None, inv_view=None):
    """the Expectation of layers_lib's scene `name` (julia, soft, soft16) under (estimator, stream) on `frames`: once per session"""
    def make():
        g = LL.grid_of(name, oracle)
        g = np.ascontiguousarray(g.astype(np.float32)) if g.dtype == np.float16 else g      # a binary16 volume renders as the widened floats
        kw = dict(estimator=est, rng_mode=rng_mode, seed=KEY)
        if inv_view is not None:
            kw["inv_view"] = inv_view
        trio = scenes_for(oracle, g, ENV, scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER, **kw)
        if est == 1 and max(frames) > 10:
            for s in trio:
                s.precompute_opacity()
        pk = dict(LL.param_kw(name), **({} if density is None else {"density": density}))
        return trio + (oracle.default_param(size[0], size[1], **pk), frames)
    key = (name, est, rng_mode, tuple(frames), tuple(size), density, None if inv_view is None else tuple(np.asarray(inv_view, F32).ravel().tolist()))
    return expectation(oracle, key, make)


def relight(sun, sky, scale, sun_gain=(1.0, 1.0, 1.0), sky_gain=(1.0, 1.0, 1.0)):
    """vp_relight in float32 numpy: (sun * s) * gain + (sky * s) * gain per channel, one rounding per operation; w = sun.w * s"""
    sun, sky, s = np.asarray(sun, F32), np.asarray(sky, F32), F32(scale)
    gs, gk = np.asarray(sun_gain, F32), np.asarray(sky_gain, F32)
    out = np.empty_like(sun)
    out[..., :3] = (sun[..., :3] * s) * gs + (sky[..., :3] * s) * gk
    out[..., 3] = sun[..., 3] * s
    return out


def sun_axis_view(sun_dir=scenes.DEFAULT_SUN_DIR, distance=4.0):
    """a 3 x 4 inverse view matrix (rows: x y z of the camera's right, up, back axes and its origin) whose viewing axis -- the
    camera's -z -- is the sun direction, from a point `distance` behind the origin: the centre pixel of an even-sized image then
    looks (u, v) = (0, 0) along sun_dir, inside the sun's disc"""
    d = np.asarray(sun_dir, np.float64)
    d = d / np.linalg.norm(d)
    back = -d
    up0 = np.array([1.0, 0.0, 0.0])
    right = np.cross(up0, back)
    right /= np.linalg.norm(right)
    up = np.cross(back, right)
    org = -d * distance
    m = np.zeros((3, 4), np.float32)
    m[:, 0], m[:, 1], m[:, 2], m[:, 3] = right, up, back, org
    return m
