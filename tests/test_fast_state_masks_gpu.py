"""render_k keeps its fast path states (TRACK, SHADOW, SETUP) in wave masks inside the tracking loop: the transitions the masks carry.

tests/test_instance_census_gpu.py runs every built instance against the oracle on full waves.  Here the launches are chosen for the
lanes' states: a launch with fewer samples than a wave has lanes (5 x 3 pixels, one frame: exhausted lanes, parked lanes, TRACK
and SHADOW lanes side by side in the only waves), a few waves (16 x 8 pixels, 8 frames), the loop's knobs at their bounds, and one
case per instance family whose lanes leave and enter the states by another way: real collisions and shadow rays handed back to
their path (global majorant, achromatic and chromatic), restarts and ST_SETUP (the two local-majorant estimators), collisions of
scalar tracking, the sequential sampler.h stream and MIS (no hand-back: the light estimate ends in the event pass), a medium whose
light class is integrated (density 209: its null collision is not neutral), a binary16 volume, a layers, a groups and a
group-layers launch, and the fast arithmetic unit.

Scene: the 32^3 Julia set, tests/scenes.py's environment, sun and default camera.  Bars: tolerance 0 on the image against the
oracle for every launch, and on the six work counters for the counting launch of the same samples (the counting instances are
kernels of their own; scalar tracking has none); the knob contexts against the same oracle image; layers, groups and group-layers against the expectations
of their libraries (tolerance 0; the libraries' own sizes, shared with their tests); the fast unit as its existing tests hold it:
a staged launch against the sum of its one-frame launches at tolerance 0, and those against the exact mode by check 3 of
tests/test_fuzz_fast_gpu.py, box-missing and light pixels bit for bit.

VP_STEPS_PER_PASS is a constant of the build, not a knob of a context: its run-time side is the lower bound of VP_WAIT_ITERS, which
is tried at that bound, below it (refused: the default) and far above."""
import numpy as np
import pytest

import group_layers_lib as GLL
import groups_lib as GL
import layers_lib as LL
import scenes
from test_fuzz_fast_gpu import PAIRED_FRAMES, assert_paired_agreement

pytestmark = pytest.mark.gpu

N = 32
KEY = (11, 22)
ENV = scenes.synthetic_env()
COUNTERS = ("samples", "density_lookups", "bound_lookups", "opacity_lookups", "env_lookups", "scatters")
UNDER, FEW = ((5, 3), 1), ((16, 8), 8)          # (size, frames): 15 samples in one wave; 128 samples x 8 frames
SHAPES = {"underfilled": UNDER, "few_waves": FEW}
CHROMATIC = dict(sigma_t=(1.0, 0.8, 0.55), albedo=(0.9, 0.8, 0.95))

# family -> volume form, estimator, brick, stream, MIS, tracking mode, medium
FAMILIES = {
    "global_ach":   dict(vol="u8",  est=0, brick=1, rng=2, mis=0, trk=0, kw={}),
    "global_chr":   dict(vol="u8",  est=0, brick=1, rng=2, mis=0, trk=0, kw=CHROMATIC),
    "decomp":       dict(vol="u8",  est=1, brick=4, rng=2, mis=0, trk=0, kw={}),
    "decomp_chr":   dict(vol="u8",  est=1, brick=4, rng=1, mis=0, trk=0, kw=CHROMATIC),
    "bounded":      dict(vol="u8",  est=2, brick=4, rng=2, mis=0, trk=0, kw={}),
    "scalar":       dict(vol="u8",  est=0, brick=1, rng=1, mis=0, trk=1, kw=CHROMATIC),
    "scalar_local": dict(vol="u8",  est=1, brick=4, rng=1, mis=0, trk=1, kw=CHROMATIC),
    "sampler_h":    dict(vol="u8",  est=0, brick=1, rng=0, mis=0, trk=0, kw={}),
    "sampler_h_local": dict(vol="u8", est=1, brick=4, rng=0, mis=0, trk=0, kw={}),
    "mis":          dict(vol="u8",  est=0, brick=1, rng=1, mis=1, trk=0, kw={}),
    "light_209":    dict(vol="u8",  est=0, brick=1, rng=2, mis=0, trk=0, kw=dict(density=209.0)),
    "half":         dict(vol="f16", est=0, brick=1, rng=2, mis=0, trk=0, kw={}),
}


@pytest.fixture
def ctx(vp):
    c = vp.Context(0)
    try:
        with c:
            yield c
    finally:
        c.destroy()


def _grid(oracle, vol):
    g = oracle.julia(N)
    return g if vol == "u8" else np.ascontiguousarray((g.astype(np.float32) / np.float32(255.0)).astype(np.float16))


_REF = {}


def _reference(oracle, family, shape):
    """(image, counters) of the oracle for one family's samples at one shape: once per session, read-only"""
    if (family, shape) not in _REF:
        F = FAMILIES[family]
        g = _grid(oracle, F["vol"])
        g = np.ascontiguousarray(g.astype(np.float32)) if g.dtype == np.float16 else g      # a binary16 volume renders as the widened floats
        osc = oracle.OracleScene(g, ENV, scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER, brick=F["brick"], estimator=F["est"], rng_mode=F["rng"],
                                 seed=KEY, env_mis=bool(F["mis"]), track_mode=F["trk"])
        (w, h), frames = SHAPES[shape]
        oP = oracle.default_param(w, h, **F["kw"])
        ref, cnt = None, None
        for f in range(frames):
            ref, c = osc.render_frame(oP, f, ref)
            d = c.as_dict()
            cnt = d if cnt is None else {q: cnt[q] + d[q] for q in d}
        ref.setflags(write=False)
        _REF[(family, shape)] = (ref, cnt)
    return _REF[(family, shape)]


def _scene(vp, oracle, family, size):
    F = FAMILIES[family]
    vp.init_volume(_grid(oracle, F["vol"]), brick=F["brick"], linear=True)
    vp.init_envmap(ENV)
    vp.set_sun(scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER)
    vp.set_camera()
    vp.set_estimator(F["est"])
    vp.set_rng(F["rng"], KEY)
    vp.set_tracking(F["trk"])
    vp.set_envmap_sampling(vp.ENV_MIS if F["mis"] else vp.ENV_PASSIVE)
    vp.set_shard(0, 1)
    return vp.make_param(size[0], size[1], **F["kw"])


def _render(vp, P, frames, count=False):
    buf = vp.DeviceBuffer(P.width, P.height)
    try:
        vp.enable_counters(count)
        vp.read_counters(reset=True)
        vp.render_frames(buf.ptr, 0, frames, P)
        got = buf.download()
        return got, (vp.read_counters() if count else None)
    finally:
        vp.enable_counters(False)
        buf.free()


def _differ(got, ref):
    return "%d of %d pixels differ" % (int((got != ref).any(-1).sum()), ref.shape[0] * ref.shape[1])


# ------------------------------------------------------------------------------------ every family, under-filled and a few waves
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("family", list(FAMILIES))
def test_family_equals_the_oracle(vp, oracle, ctx, family, shape):
    (w, h), frames = SHAPES[shape]
    ref, cnt = _reference(oracle, family, shape)
    assert cnt["samples"] == w * h * frames
    if shape == "few_waves":
        assert cnt["scatters"] > 0, "no path of this launch collides: it has no SHADOW lane"
    P = _scene(vp, oracle, family, (w, h))
    got, _ = _render(vp, P, frames)                      # the timed instance
    assert np.array_equal(got, ref, equal_nan=True), (family, shape, "timed", _differ(got, ref))
    if FAMILIES[family]["trk"]:                          # (work counters are not built for the scalar tracking kernels)
        return
    got, k = _render(vp, P, frames, count=True)          # the counting instance: the image again, and its work
    assert np.array_equal(got, ref, equal_nan=True), (family, shape, "counting", _differ(got, ref))
    for q in COUNTERS:
        assert k[q] == cnt[q], (family, shape, q, k[q], cnt[q])


# ------------------------------------------------------------------------------------------------------- the loop's knobs at their bounds
KNOBS = [
    dict(VP_WAIT_LANES="1"), dict(VP_WAIT_LANES="64"),
    dict(VP_WAIT_ITERS="1"), dict(VP_WAIT_ITERS="4"), dict(VP_WAIT_ITERS="1048576"),
    dict(VP_END_LANES="1"), dict(VP_END_LANES="64"),
    dict(VP_SETUP_LANES="1"), dict(VP_SETUP_LANES="64"),
    dict(VP_WAIT_LANES="1", VP_WAIT_ITERS="4", VP_END_LANES="1", VP_SETUP_LANES="1"),
    dict(VP_WAIT_LANES="64", VP_WAIT_ITERS="1048576", VP_END_LANES="64", VP_SETUP_LANES="64"),
]


@pytest.mark.parametrize("family", ["global_ach", "decomp", "sampler_h"])
def test_loop_knobs_at_their_bounds_keep_the_bits(vp, oracle, monkeypatch, family):
    (w, h), frames = FEW
    ref, _ = _reference(oracle, family, "few_waves")
    for knobs in KNOBS + [{}]:                           # ({}: the default context, last -- none of it has touched it)
        for k, v in knobs.items():
            monkeypatch.setenv(k, v)
        c = vp.Context(0)                                # (the knobs are read when a context is made)
        for k in knobs:
            monkeypatch.delenv(k)
        try:
            with c:
                P = _scene(vp, oracle, family, (w, h))
                got, _ = _render(vp, P, frames)
                under, _ = _render(vp, _scene(vp, oracle, family, UNDER[0]), UNDER[1])
        finally:
            c.destroy()
        assert np.array_equal(got, ref, equal_nan=True), (family, knobs, _differ(got, ref))
        small = _reference(oracle, family, "underfilled")[0]
        assert np.array_equal(under, small, equal_nan=True), (family, knobs, "under-filled", _differ(under, small))


# ---------------------------------------------------------------------------------------------- layers, groups, group layers: one launch each
def _planes_scene(vp, oracle, est, rng_mode, size):
    vp.init_volume(LL.grid_of("julia", oracle), brick=1, linear=True)
    vp.init_envmap(LL.ENV)
    vp.set_sun(scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER)
    vp.set_camera()
    vp.set_estimator(est)
    vp.set_rng(rng_mode, LL.KEY)
    vp.set_tracking(vp.TRACK_SPECTRAL)
    vp.set_envmap_sampling(vp.ENV_PASSIVE)
    vp.set_shard(0, 1)
    if est == 1:
        vp.precompute_opacity(scenes.DEFAULT_SUN_DIR)
    return vp.make_param(size[0], size[1], **LL.param_kw("julia"))


def _launch(vp, call, n_planes, first, n, P):
    bufs = [vp.DeviceBuffer(P.width, P.height) for _ in range(n_planes)]
    try:
        call(*[b.ptr for b in bufs], first, n, P)
        return [b.download() for b in bufs]
    finally:
        for b in bufs:
            b.free()


@pytest.mark.parametrize("est", [0, 1])
def test_layers_launch_equals_its_expectation(vp, oracle, ctx, est):
    E = LL.expected(oracle, "julia", est, 2)
    P = _planes_scene(vp, oracle, est, 2, (LL.W, LL.H))
    fg, tr = _launch(vp, vp.render_frames_layers, 2, LL.FRAMES[0], len(LL.FRAMES), P)
    assert np.array_equal(fg, E.fg, equal_nan=True), ("fg", _differ(fg, E.fg))
    assert np.array_equal(tr, E.trans, equal_nan=True), ("trans", _differ(tr, E.trans))


@pytest.mark.parametrize("est", [0, 1])
def test_groups_launch_equals_its_expectation(vp, oracle, ctx, est):
    E = GL.expected(oracle, "julia", est, 2)
    P = _planes_scene(vp, oracle, est, 2, (GL.W, GL.H))
    sun, sky = _launch(vp, vp.render_frames_groups, 2, GL.FRAMES[0], len(GL.FRAMES), P)
    assert np.array_equal(sun, E.sun, equal_nan=True), ("sun", _differ(sun, E.sun))
    assert np.array_equal(sky, E.sky, equal_nan=True), ("sky", _differ(sky, E.sky))


@pytest.mark.parametrize("est", [0, 1])
def test_group_layers_launch_equals_its_expectation(vp, oracle, ctx, est):
    E = GLL.expected(oracle, "julia", est, 2)
    P = _planes_scene(vp, oracle, est, 2, (GLL.W, GLL.H))
    got = _launch(vp, vp.render_frames_group_layers, 3, GLL.FRAMES[0], len(GLL.FRAMES), P)
    for k, (g, want) in enumerate(zip(got, E.accs())):
        assert np.array_equal(g, want, equal_nan=True), (GLL.PLANES[k], _differ(g, want))


# ------------------------------------------------------------------------------------------------------------ the fast arithmetic unit
def _fast_scene(vp, oracle, family, size):
    P = _scene(vp, oracle, family, size)
    if FAMILIES[family]["est"] == 1:
        vp.precompute_opacity(scenes.DEFAULT_SUN_DIR)
    return P


@pytest.mark.parametrize("family", ["global_ach", "global_chr", "decomp"])
def test_fast_unit_against_its_own_reference(vp, oracle, ctx, family):
    """the staged launch of 8 frames against the sum of its one-frame launches (the base instance), tolerance 0; PAIRED_FRAMES one-frame
    renders in both modes: box-missing and light pixels bit for bit, the general ones by check 3 of tests/test_fuzz_fast_gpu.py"""
    (w, h), frames = FEW
    P = _fast_scene(vp, oracle, family, (w, h))
    cls = vp.pixel_table(P)[..., 5].astype(int)
    buf = vp.DeviceBuffer(w, h)
    try:
        d = np.empty((PAIRED_FRAMES, h, w, 3), np.float64)
        e = np.empty_like(d)
        for i in range(PAIRED_FRAMES):
            for m, out in ((vp.ARITH_EXACT, e), (vp.ARITH_FAST, d)):
                vp.set_arithmetic(m)
                buf.reset()
                vp.render_frames(buf.ptr, i, 1, P)
                out[i] = buf.download()[..., :3]
            assert np.array_equal(d[i][cls != 0], e[i][cls != 0]), (family, i, "box-missing / light pixels")
        assert_paired_agreement(d, e, family)
        vp.set_arithmetic(vp.ARITH_FAST)
        buf.reset()
        for f in range(frames):
            vp.render_frames(buf.ptr, f, 1, P)
        one = buf.download()
        buf.reset()
        vp.render_frames(buf.ptr, 0, frames, P)
        got = buf.download()
        assert vp.last_arithmetic() == vp.ARITH_FAST
        assert np.array_equal(got, one), (family, _differ(got, one))
        (uw, uh), _ = UNDER
        Pu = _fast_scene(vp, oracle, family, (uw, uh))
        small = vp.DeviceBuffer(uw, uh)
        try:
            vp.render_frames(small.ptr, 0, 1, Pu)
            a = small.download()
            small.reset()
            vp.render_frames(small.ptr, 0, 1, Pu)
            assert vp.last_arithmetic() == vp.ARITH_FAST and np.isfinite(a).all() and np.array_equal(small.download(), a), (family, "under-filled")
        finally:
            small.free()
    finally:
        vp.set_arithmetic(vp.ARITH_EXACT)
        buf.free()
