"""What vp_render_frames_group_layers, its _stats form and vp_relight_composite must produce (include/volpath.h, DESIGN.md section
2.10), from the CPU oracle alone.  A helper, not a test.

No new oracle code: layers_lib.sample and groups_lib.sample (or vpo_render_samples on the same four scenes, the loop that
tests/test_fuzz_planes_cpu.py pins to them) yield, per sample, fg, trans, sun, sky, beauty and the `unscattered` flag.  The definition's
table folds them:

    unscattered:  sun sample (0, 0, 0, w)    sky sample (0, 0, 0, w)    trans sample = the layers trans sample
    otherwise:    sun sample = groups' sun   sky sample = groups' sky   trans sample (0, 0, 0, 0)

w being the real sample's fourth channel.  Accumulators are float32 sums in frame order, records go through plane_stats_lib.fold, one
Stats per plane.  The scenes are those of tests/layers_lib.py."""
import numpy as np

import adaptive_lib as AL
import groups_lib as GL
import layers_lib as LL
import planes_fuzz_lib as PF
import scenes

F32 = np.float32
W, H, FRAMES, LONG, ENV, KEY = LL.W, LL.H, LL.FRAMES, LL.LONG, LL.ENV, LL.KEY
PLANES = ("sun", "sky", "trans")


def fold_samples(sun, sky, trans, beauty, unscattered):
    """the three samples of the definition's table from the per-sample values of the two plane calls: arrays (..., 4) and a bool (...)"""
    u = np.asarray(unscattered, bool)
    a, k, t = np.array(sun, F32), np.array(sky, F32), np.array(trans, F32)
    a[u, :3] = 0.0
    k[u, :3] = 0.0
    a[u, 3] = np.asarray(beauty, F32)[u, 3]
    k[u, 3] = np.asarray(beauty, F32)[u, 3]
    t[~u] = 0.0
    return a, k, t


class Samples:
    """Every sample of a render.  sun, sky, trans (this call's), fg, beauty and the groups call's own sun (gsun) and sky (gsky):
    (n, H, W, 4) float32, frame k of them is frame first + k; unscattered: (n, H, W) bool; miss: (H, W) bool.  All read-only."""

    def __init__(self, first, fg, trans, sun, sky, beauty, unscattered, miss):
        self.first, self.n = int(first), len(beauty)
        self.H, self.W = beauty.shape[1:3]
        self.fg, self.beauty, self.gsun, self.gsky = fg, beauty, sun, sky
        self.unscattered, self.miss = np.asarray(unscattered, bool), np.asarray(miss, bool)
        self.sun, self.sky, self.trans = fold_samples(sun, sky, trans, beauty, unscattered)
        for k in PLANES + ("fg", "beauty", "gsun", "gsky", "unscattered", "miss"):
            getattr(self, k).setflags(write=False)

    def acc(self, plane, lo=0, hi=None):
        """the accumulator of `plane` after frames lo .. hi - 1 of the render, from zero: float32, frame order"""
        a = np.zeros((self.H, self.W, 4), F32)
        for img in getattr(self, plane)[lo:self.n if hi is None else hi]:
            a = a + img
        return a

    def accs(self, lo=0, hi=None):
        return tuple(self.acc(p, lo, hi) for p in PLANES)

    def stats(self, lo=0, hi=None, owned=None, into=None):
        """the three Stats (accumulator and records) after frames lo .. hi - 1, continued from `into` where given: the fold of
        plane_stats_lib.fold over three planes"""
        import plane_stats_lib as PS
        hi = self.n if hi is None else hi
        st = into if into is not None else tuple(AL.Stats(self.W, self.H) for _ in PLANES)
        return PS.fold(lambda f: tuple(getattr(self, p)[f - self.first] for p in PLANES), self.W, self.H, self.first + lo, hi - lo, owned=owned, into=st)

    def groups(self):
        """pixels per group: box-missing; unscattered in every frame (but tracked); scattered in every frame; mixed over the frames"""
        u_all, u_any = self.unscattered.all(0), self.unscattered.any(0)
        assert (u_all | ~self.miss).all(), "a ray that misses the box cannot scatter"
        return dict(miss=int(self.miss.sum()), unscattered=int((u_all & ~self.miss).sum()), scattered=int((~u_any).sum()), mixed=int((u_any & ~u_all).sum()))


def of_frames(E):
    """the Samples of a planes_fuzz_lib.Frames"""
    return Samples(E.first, E.fg, E.trans, E.sun, E.sky, E.beauty, E.unscattered, E.miss)


_CACHE = {}


def expectation(oracle, key, make):
    """the Samples of `key`, computed once per session; make() -> (real, layers twin, sun twin, sky twin, Param, frames), the frames a
    run of consecutive ones"""
    if key not in _CACHE:
        real, twin, sun, sky, P, frames = make()
        frames = tuple(frames)
        assert frames == tuple(range(frames[0], frames[0] + len(frames)))
        Q = LL.twin_param(oracle, P)
        out = {k: np.zeros((len(frames), P.height, P.width, 4), F32) for k in PF.VALUES}
        uns = np.zeros((len(frames), P.height, P.width), bool)
        for i, f in enumerate(frames):
            one, scatters, _ = PF._frame_c(oracle, real, twin, sun, sky, P, Q, f)
            for k in PF.VALUES:
                out[k][i] = one[k]
            uns[i] = scatters == 0
        _CACHE[key] = Samples(frames[0], out["fg"], out["trans"], out["sun"], out["sky"], out["beauty"], uns, GL._miss(oracle, real, P.width, P.height))
    return _CACHE[key]


def scenes_for(oracle, grid, env, sun_dir, sun_power, opacity=False, **kw):
    """(real, layers twin, sun twin, sky twin): four OracleScenes that differ in the lights and in nothing a draw depends on"""
    real, sun, sky = GL.scenes_for(oracle, grid, env, sun_dir, sun_power, **kw)
    twin = LL.scenes_for(oracle, grid, env, sun_dir, sun_power, **kw)[1]
    if opacity:
        for s in (real, twin, sun, sky):
            s.precompute_opacity()
    return real, twin, sun, sky


def expected(oracle, name, est, rng_mode, frames=FRAMES, size=(W, H), density=None, inv_view=None):
    """the Samples of layers_lib's scene `name` (julia, soft, soft16) under (estimator, stream) on `frames`: once per session"""
    def make():
        g = LL.grid_of(name, oracle)
        g = np.ascontiguousarray(g.astype(np.float32)) if g.dtype == np.float16 else g      # a binary16 volume renders as the widened floats
        kw = dict(estimator=est, rng_mode=rng_mode, seed=KEY)
        if inv_view is not None:
            kw["inv_view"] = inv_view
        four = scenes_for(oracle, g, ENV, scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER, opacity=est == 1 and max(frames) > 10, **kw)
        pk = dict(LL.param_kw(name), **({} if density is None else {"density": density}))
        return four + (oracle.default_param(size[0], size[1], **pk), frames)
    key = (name, est, rng_mode, tuple(frames), tuple(size), density, None if inv_view is None else tuple(np.asarray(inv_view, F32).ravel().tolist()))
    return expectation(oracle, key, make)


def relight_composite(sun, sky, trans, scale, sun_gain=(1.0, 1.0, 1.0), sky_gain=(1.0, 1.0, 1.0), plate=None, rgb=None):
    """vp_relight_composite in float32 numpy, one rounding per operation in the header's order:
    f = (sun * s) * gain + (sky * s) * gain; dst = f + (trans * s) * B; w = 1 - trans.w * s"""
    sun, sky, trans, s = np.asarray(sun, F32), np.asarray(sky, F32), np.asarray(trans, F32), F32(scale)
    gs, gk = np.asarray(sun_gain, F32), np.asarray(sky_gain, F32)
    B = np.asarray(plate, F32)[..., :3] if plate is not None else np.asarray(rgb, F32)
    out = np.empty_like(sun)
    f = (sun[..., :3] * s) * gs + (sky[..., :3] * s) * gk
    out[..., :3] = f + (trans[..., :3] * s) * B
    out[..., 3] = F32(1.0) - trans[..., 3] * s
    return out


def three_steps(sun, sky, trans, scale, sun_gain=(1.0, 1.0, 1.0), sky_gain=(1.0, 1.0, 1.0), plate=None, rgb=None):
    """the sequence vp_relight_composite is defined by, from the restatements of its steps: groups_lib.relight, `scale` of the
    transmittance, layers_lib.composite with a scale of 1"""
    tmp = GL.relight(sun, sky, scale, sun_gain, sky_gain)
    t = np.asarray(trans, F32) * F32(scale)
    return LL.composite(tmp, t, F32(1.0), plate=plate, rgb=rgb)
