"""The random scenes of tests/scenes.py as cases for the plane calls -- vp_render_frames_layers, vp_render_frames_groups and their _stats
forms (include/volpath.h, DESIGN.md sections 2.6 to 2.8) --, and what those calls must produce on them, from the CPU oracle alone.
A helper, not a test.

Cases.  case(seed) is scenes.random_case(12000 + seed); long_case(seed) is scenes.random_case(15000 + seed) under the long-launch
recipe of tests/test_fuzz_gpu.py (grid cropped to 20^3, the decomposition or the global-majorant estimator, 64..100 frames, the
optical-depth table for the decomposition estimator) with the image at most 16 x 12.  Both are forced to the build the plane calls
accept (passive environment, spectral tracking), and a float32 grid of a seed that is a multiple of three is rounded to binary16 and
handed to the library as such; its expectation comes from the widened floats.

Expectation.  frames(oracle, case) keeps EVERY SAMPLE of every frame: the layers pair of layers_lib.sample, the groups pair of
groups_lib.sample, the beauty sample and the flags.  Accumulators are float32 sums of them in frame order (Frames.acc), records their
fold by plane_stats_lib.fold (Frames.stats).  The samples come from one of two loops with the same rules and the same assertions
("the twin left the path", "the twins carry the real sample's w"): the per-sample Python loop over layers_lib.sample and
groups_lib.sample, or vpo_render_samples -- the oracle's per-sample function for a whole frame in C -- on the same four scenes;
tests/test_fuzz_planes_cpu.py pins the second to the first byte for byte.  The optical-depth table is a function of grid, box and sun
direction, which the twins share with the real scene: it is computed once and handed to them (pinned there too).

Admission.  The header's equivalent forms, which the twins restate, are the definition only where every value is finite, and
`scatters == 0` means "unscattered" only where the path did reach the environment (tests/layers_lib.py on the 800-segment cap): a
sample with no scatter, density lookups and an all-zero twin RGB may have been ended by the cap.  admissible() is false for a case
with such a sample or with a non-finite value; such a case is left out, never compared more loosely.
  Finite VALUES do not show a non-finite THROUGHPUT: an amplifying channel (a negative null-collision factor of the spectral tracker)
can run a throughput to inf and on to NaN, after which no comparison of the tracker holds, the path flies out of the box, and fmaxf
turns the NaN of thr o background into 0 in the beauty sample and in both twins -- while the call's own definition keeps the sun's
light the path had summed until then, max(b R, 0), in the sun group.  Short seeds 7 and 25 each have one such sample (sun.x of
1.7e-9 and 1.4e-2 in the library, 0 in all three oracle renders): the library is right and the twins are not.  The oracle therefore
counts the samples whose throughput is not finite when the path ends (vpo_debug_nonfinite_throughput); a case with one is not admitted."""
import numpy as np

import groups_lib as GL
import layers_lib as LL
import plane_stats_lib as PS
import scenes

F32 = np.float32
SHORT_BASE, LONG_BASE = 12000, 15000
SHORT_SEEDS, LONG_SEEDS = 32, 8                   # the default lists
MAX_W, MAX_H = 16, 12                             # of a long case
PLANES = {"layers": ("fg", "trans"), "groups": ("sun", "sky")}
VALUES = ("fg", "trans", "sun", "sky", "beauty")
FLAGS = ("unscattered", "no_lookup", "lit_sun", "lit_sky", "ambiguous")


def _force(c, seed):
    """the build the plane calls accept; every third seed's float32 grid as binary16"""
    c["seed"] = seed
    c["env_mis"], c["track"] = False, 0
    if c["grid"].dtype == np.float32 and seed % 3 == 0:
        c["grid"] = np.ascontiguousarray(c["grid"].astype(np.float16))
    return c


def case(seed, host):
    c = scenes.random_case(SHORT_BASE + seed, host)
    c["long"] = False
    return _force(c, seed)


def long_case(seed, host):
    c = scenes.random_case(LONG_BASE + seed, host)
    rng = np.random.default_rng(77 + LONG_BASE + seed)
    c["grid"] = np.ascontiguousarray(c["grid"][:20, :20, :20])
    if c["grid"].dtype != np.uint8 and rng.random() < 0.7:
        c["grid"] = np.ascontiguousarray((np.clip(c["grid"], 0.0, 1.0) * 255.0).astype(np.uint8))
    c["est"] = int(rng.choice([1, 1, 1, 0]))
    c["brick"] = int(rng.choice([1, 2, 4, 8])) if c["est"] else 1
    c["W"], c["H"] = min(int(rng.integers(3, 20)), MAX_W), min(int(rng.integers(3, 14)), MAX_H)
    c["first"], c["nframes"] = int(rng.choice([0, 5, 11, 40])), int(rng.integers(64, 101))
    c["late"] = c["est"] == 1
    c["long"] = True
    return _force(c, seed)


def volume_format(c):
    return {np.dtype(np.uint8): "u8", np.dtype(np.float32): "f32", np.dtype(np.float16): "f16"}[c["grid"].dtype]


def across_switch(c):
    """the decomposition estimator's frames straddle its switch to the optical-depth table at frame 11"""
    return c["est"] == 1 and c["first"] <= 10 < c["first"] + c["nframes"] - 1


def what(c):
    """the case in a failure message"""
    return dict(seed=c["seed"], long=c["long"], grid=c["grid"].shape, dtype=str(c["grid"].dtype), box=c["box"], est=c["est"], rng=c["rng_mode"],
                linear=c["linear"], brick=c["brick"], size=(c["W"], c["H"]), first=c["first"], nframes=c["nframes"], world=c["world"], **c["kw"])


def oracle_scenes(oracle, c, share_opacity=True):
    """(real, layers twin, sun twin, sky twin, Param) of a case"""
    g = c["grid"]
    g = np.ascontiguousarray(g.astype(np.float32)) if g.dtype == np.float16 else g          # a binary16 volume renders as the widened floats
    kw = dict(box=c["box"], brick=c["brick"], linear=c["linear"], estimator=c["est"], rng_mode=c["rng_mode"], seed=c["key"], inv_view=c["cam"])
    real, sun, sky = GL.scenes_for(oracle, g, c["env"], c["sun_dir"], c["sun_power"], **kw)
    twin = LL.scenes_for(oracle, g, c["env"], c["sun_dir"], c["sun_power"], **kw)[1]
    if c["late"]:
        real.precompute_opacity()
        for s in (twin, sun, sky):
            if share_opacity:
                s.opacity, s.S.opacity = real.opacity, real.S.opacity
            else:
                s.precompute_opacity()
    return real, twin, sun, sky, oracle.default_param(c["W"], c["H"], **c["kw"])


def _frame_python(oracle, real, twin, sun, sky, P, Q, f):
    """one frame through layers_lib.sample and groups_lib.sample, sample by sample"""
    H, W = P.height, P.width
    out = {k: np.zeros((H, W, 4), F32) for k in VALUES}
    scatters, lookups = np.zeros((H, W), np.uint64), np.zeros((H, W), np.uint64)
    for y in range(H):
        for x in range(W):
            fg, tr, v, cnt = LL.sample(oracle, real, twin, P, x, y, f, Q)
            a, k = GL.sample(real, sun, sky, P, x, y, f, base=(v, cnt))[:2]
            for name, val in (("fg", fg), ("trans", tr), ("sun", a), ("sky", k), ("beauty", v)):
                out[name][y, x] = val
            scatters[y, x], lookups[y, x] = cnt.scatters, cnt.density_lookups
    return out, scatters, lookups


def _frame_c(oracle, real, twin, sun, sky, P, Q, f):
    """the same frame through vpo_render_samples: the rules and assertions of layers_lib.sample and groups_lib.sample on whole images"""
    v, cnt = real.render_samples(P, f)
    t, tc = twin.render_samples(Q, f)
    uns = cnt["scatters"] == 0
    same = (tc["scatters"] == 0) & (tc["rng_draws"] == cnt["rng_draws"]) & (tc["density_lookups"] == cnt["density_lookups"])
    assert same[uns].all(), "the twin left the path"
    fg, tr = v.copy(), np.zeros_like(v)
    fg[uns, :3] = 0.0
    tr[uns, :3] = t[uns, :3]
    tr[uns, 3] = 1.0
    out = {"fg": fg, "trans": tr, "beauty": v}
    for name, s in (("sun", sun), ("sky", sky)):
        g, gc = s.render_samples(P, f)
        assert all(np.array_equal(gc[q], cnt[q]) for q in ("rng_draws", "scatters", "density_lookups")), "a twin left the path"
        assert (g[..., 3] == v[..., 3]).all(), "the twins carry the real sample's w"
        out[name] = g
    return out, cnt["scatters"], cnt["density_lookups"]


class Frames:
    """Every sample of a case.  fg, trans, sun, sky, beauty: (n, H, W, 4) float32, frame k of them is frame first + k; unscattered,
    no_lookup (the path fetched no density), lit_sun, lit_sky (the group's RGB is not all zero), ambiguous (see the module's docstring):
    (n, H, W) bool; miss: (H, W) bool, the camera ray misses the box.  All read-only."""

    def __init__(self, oracle, c, loop="c", share_opacity=True):
        real, twin, sun, sky, P = oracle_scenes(oracle, c, share_opacity)
        Q = LL.twin_param(oracle, P)
        self.first, self.n, self.W, self.H = c["first"], c["nframes"], c["W"], c["H"]
        for k in VALUES:
            setattr(self, k, np.zeros((self.n, self.H, self.W, 4), F32))
        for k in FLAGS:
            setattr(self, k, np.zeros((self.n, self.H, self.W), bool))
        one = {"c": _frame_c, "python": _frame_python}[loop]
        nonfinite = oracle.lib().vpo_debug_nonfinite_throughput()
        for i in range(self.n):
            out, scatters, lookups = one(oracle, real, twin, sun, sky, P, Q, self.first + i)
            for k in VALUES:
                getattr(self, k)[i] = out[k]
            self.unscattered[i] = scatters == 0
            self.no_lookup[i] = lookups == 0
            self.lit_sun[i] = out["sun"][..., :3].any(-1)
            self.lit_sky[i] = out["sky"][..., :3].any(-1)
            # an unscattered sample's trans RGB is its twin's RGB
            self.ambiguous[i] = self.unscattered[i] & ~self.no_lookup[i] & ~out["trans"][..., :3].any(-1)
        self.nonfinite = oracle.lib().vpo_debug_nonfinite_throughput() > nonfinite      # some sample's throughput ended non-finite
        self.miss = GL._miss(oracle, real, self.W, self.H)
        self.inv_view, self.sun_dir = list(real.S.inv_view), np.array(list(real.S.sun_dir), F32)
        for k in VALUES + FLAGS + ("miss",):
            getattr(self, k).setflags(write=False)

    def acc(self, plane, lo=0, hi=None):
        """the accumulator of `plane` (fg, trans, sun, sky, beauty) after frames lo .. hi - 1 of the case, from zero: float32, frame order"""
        a = np.zeros((self.H, self.W, 4), F32)
        for img in getattr(self, plane)[lo:self.n if hi is None else hi]:
            a = a + img
        return a

    def pair(self, kind):
        """frame_pair(f) of plane_stats_lib.fold: the two one-frame images of `kind` (layers, groups) of absolute frame f"""
        p0, p1 = (getattr(self, k) for k in PLANES[kind])
        return lambda f: (p0[f - self.first], p1[f - self.first])

    def stats(self, kind, lo=0, hi=None, owned=None, into=None):
        """the two Stats (accumulator and records) of `kind` after frames lo .. hi - 1 of the case, continued from `into` where given"""
        hi = self.n if hi is None else hi
        return PS.fold(self.pair(kind), self.W, self.H, self.first + lo, hi - lo, owned=owned, into=into)

    def groups(self):
        """pixels per group: box-missing; unscattered in every frame (but tracked); scattered in every frame; mixed over the frames"""
        u_all, u_any = self.unscattered.all(0), self.unscattered.any(0)
        assert (u_all | ~self.miss).all() and (self.no_lookup.all(0) | ~self.miss).all(), "a ray that misses the box fetches nothing and cannot scatter"
        return dict(miss=int(self.miss.sum()), unscattered=int((u_all & ~self.miss).sum()), scattered=int((~u_any).sum()), mixed=int((u_any & ~u_all).sum()))


def frames(oracle, c, loop="c"):
    return Frames(oracle, c, loop)


def admissible(E):
    """None if the header's equivalent forms define every sample of the case, else why not"""
    if E.ambiguous.any():
        return "%d samples without a scatter, with density lookups and a black twin: the segment cap may have ended them" % int(E.ambiguous.sum())
    for k in VALUES:
        if not np.isfinite(getattr(E, k)).all():
            return "non-finite values in " + k
    if E.nonfinite:
        return "a path ended with a non-finite throughput"
    return None


_CACHE = {}


def expectation(oracle, long, seed):
    """(case, Frames) of a seed of the short or the long list: once per session, read-only"""
    from volpath import host
    if (long, seed) not in _CACHE:
        c = (long_case if long else case)(seed, host)
        _CACHE[(long, seed)] = (c, Frames(oracle, c))
    return _CACHE[(long, seed)]


def coverage(pairs):
    """how many of the (case, Frames) pairs have each property"""
    n = dict.fromkeys(("cases", "user_box", "point_filter", "brick_gt1", "float_grid", "first_ge_977", "across_switch", "world_gt1", "mixed", "miss",
                       "unscattered", "scattered", "no_miss", "est0", "est1", "est2", "rng0", "rng1", "rng2", "u8", "f32", "f16"), 0)
    for c, E in pairs:
        g = E.groups()
        for k, hit in (("cases", True), ("user_box", c["box"] is not None), ("point_filter", not c["linear"]), ("brick_gt1", c["brick"] > 1),
                       ("float_grid", c["grid"].dtype != np.uint8), ("first_ge_977", c["first"] >= 977), ("across_switch", across_switch(c)),
                       ("world_gt1", c["world"] > 1), ("mixed", g["mixed"] > 0), ("miss", g["miss"] > 0), ("unscattered", g["unscattered"] > 0),
                       ("scattered", g["scattered"] > 0), ("no_miss", g["miss"] == 0), ("est%d" % c["est"], True), ("rng%d" % c["rng_mode"], True),
                       (volume_format(c), True)):
            n[k] += bool(hit)
    return n
