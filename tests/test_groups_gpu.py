"""Light groups on the GPU (include/volpath.h vp_render_frames_groups / vp_relight).

Every comparison of accumulators is at tolerance 0: against the oracle-built expectation of tests/groups_lib.py (the zero-environment
and zero-sun twins of the CPU oracle), against the library's own vp_render_frames on those twins, or against the numpy restatement of
vp_relight.  The one bound is the relight-against-beauty test's, derived there.  Each test runs in a context of its own."""
import ctypes as C

import numpy as np
import pytest

import groups_lib as GL
import layers_lib as LL
import scenes
import subpixel_lib

pytestmark = pytest.mark.gpu

W, H, FRAMES, LONG = GL.W, GL.H, GL.FRAMES, GL.LONG
FIRST, N = FRAMES[0], len(FRAMES)
E_STATE = -2
F32 = np.float32
ZERO = (0.0, 0.0, 0.0)


@pytest.fixture
def ctx(vp):
    c = vp.Context(0)
    try:
        with c:
            yield c
    finally:
        c.destroy()


def _scene(vp, oracle, name, est, rng_mode, size=(W, H), camera=None, env=None, sun_power=scenes.DEFAULT_SUN_POWER):
    g = LL.grid_of(name, oracle)
    vp.init_volume(g, brick=1, linear=True)
    assert vp.volume_info()["format"] == {"julia": vp.VOL_U8, "soft": vp.VOL_F32, "soft16": vp.VOL_F16}[name]
    vp.init_envmap(GL.ENV if env is None else env)
    vp.set_sun(scenes.DEFAULT_SUN_DIR, sun_power)
    if camera is None:
        vp.set_camera()
    else:
        vp.set_camera([float(v) for v in np.asarray(camera, F32).ravel()])
    vp.set_estimator(est)
    vp.set_rng(rng_mode, GL.KEY)
    vp.set_tracking(vp.TRACK_SPECTRAL)
    vp.set_envmap_sampling(vp.ENV_PASSIVE)
    vp.set_shard(0, 1)
    if est == 1:
        vp.precompute_opacity(scenes.DEFAULT_SUN_DIR)
    return vp.make_param(size[0], size[1], **LL.param_kw(name))


class Pair:
    """the two accumulators of a groups call"""

    def __init__(self, vp, w=W, h=H):
        self.vp, self.sun, self.sky = vp, vp.DeviceBuffer(w, h), vp.DeviceBuffer(w, h)

    def render(self, first, n, P):
        self.vp.render_frames_groups(self.sun.ptr, self.sky.ptr, first, n, P)
        return self.sun.download(), self.sky.download()

    def reset(self):
        self.sun.reset()
        self.sky.reset()

    def free(self):
        self.sun.free()
        self.sky.free()


def _same(got, want, what):
    assert np.array_equal(got[0], want[0], equal_nan=True), (what, "sun", int((got[0] != want[0]).any(-1).sum()))
    assert np.array_equal(got[1], want[1], equal_nan=True), (what, "sky", int((got[1] != want[1]).any(-1).sum()))


# ------------------------------------------------------------------------------------------------------- against the oracle
CASES = [("soft", e, r) for e in (0, 1, 2) for r in (0, 2)] + [(n, e, r) for n in ("julia", "soft16") for e in (0, 1) for r in (0, 2)]


@pytest.mark.parametrize("name,est,rng_mode", CASES, ids=["%s-est%d-rng%d" % c for c in CASES])
def test_groups_equal_the_oracle_twins(vp, oracle, ctx, name, est, rng_mode):
    E = GL.expected(oracle, name, est, rng_mode)
    P = _scene(vp, oracle, name, est, rng_mode)
    general, light, miss = vp.pixel_lists(P)
    p = Pair(vp)
    try:
        got = p.render(FIRST, N, P)                     # batched: one staged launch
        _same(got, (E.sun, E.sky), (name, est, rng_mode, "batched"))
        p.reset()
        for f in FRAMES:                                # frame by frame: staged too (the direct path has no second target)
            single = p.render(f, 1, P)
        _same(single, (E.sun, E.sky), (name, est, rng_mode, "frame by frame"))
    finally:
        p.free()
    # pixel classes, from the expectation: box-missing pixels, pixels that scatter (general), and -- the Julia set has empty margins
    # inside its box -- pixels that cross the box without ever scattering (where the light class lives)
    assert E.miss.any() and E.scattered.any() and len(miss) == int(E.miss.sum()) and len(general) > 0
    if name == "julia":
        assert len(light) > 0 and (~E.scattered.any(0) & ~E.miss).any()
    both = (E.sun[..., :3].max(-1) > 0) & (E.sky[..., :3].max(-1) > 0)
    assert both.any() and np.isfinite(E.sun).all() and np.isfinite(E.sky).all()


@pytest.mark.parametrize("est,density,const", ((0, 61.0, False), (0, 64.0, True), (1, 61.0, False), (2, 61.0, False)))
def test_light_class_as_a_kernel_and_as_constants(vp, oracle, ctx, est, density, const):
    """The light pixel class of the Julia set (tests/test_layers_gpu.py has the reasons for the two densities): at a majorant of 61 a
    null collision in empty space moves the throughput and the light kernel runs, whose groups instance routes each sample to one
    plane; at 64 it is neutral and the class is written as constants, staged once in the first row of either plane."""
    E = GL.expected(oracle, "julia", est, 1, density=density)
    P = _scene(vp, oracle, "julia", est, 1)
    P.density = density
    general, light, miss = vp.pixel_lists(P)
    assert len(light) > 0 and len(miss) > 0 and len(general) > 0
    p = Pair(vp)
    try:
        for first, n in ((FIRST, N), (FIRST, 1)):
            p.reset()
            p.render(first, n, P)
            assert vp.last_light_const() == const
        _same(p.render(FIRST + 1, 1, P), (E.sun, E.sky), (density, "one frame, then the next"))
        p.reset()
        _same(p.render(FIRST, N, P), (E.sun, E.sky), (density, "batched"))
    finally:
        p.free()
    ly, lx = light >> 16, light & 0xffff
    assert not E.sun[ly, lx][:, :3].any() and (E.sky[ly, lx][:, :3].max(-1) > 0).all()     # the class sees the sky, never the sun (this camera)


@pytest.mark.parametrize("name,est", (("julia", 0), ("julia", 1), ("soft", 1)))
def test_a_launch_of_70_frames_equals_the_oracle_twins(vp, oracle, monkeypatch, name, est):
    """one launch of 64 frames or more: the approach walks hand their samples over (in a context that never takes the volume for too
    dense to walk: VP_DENSE_PERCENT=101), the constants of the launch are staged once, in both planes"""
    E = GL.expected(oracle, name, est, 1, frames=LONG)
    monkeypatch.setenv("VP_DENSE_PERCENT", "101")
    c = vp.Context(0)
    monkeypatch.delenv("VP_DENSE_PERCENT")
    try:
        with c:
            P = _scene(vp, oracle, name, est, 1)
            p = Pair(vp)
            try:
                got = p.render(LONG[0], len(LONG), P)
                if name == "julia":
                    assert vp.last_approach_mode() != 0, "the approach walk did not run"
                _same(got, (E.sun, E.sky), (name, est))
            finally:
                p.free()
    finally:
        c.destroy()
    assert E.miss.any() and E.scattered.any()


def test_sun_disc_pixel_goes_to_the_sun_group(vp, oracle, ctx):
    """a camera whose axis is the sun direction: pixel (W/2, H/2) looks into the disc (asserted on the oracle in
    tests/test_groups_cpu.py: unscattered, its sun sample is b thr o sun_power_original and its sky sample 0)"""
    view = GL.sun_axis_view()
    frames = tuple(range(10, 16))
    E = GL.expected(oracle, "soft", 0, 1, frames=frames, inv_view=view)
    x, y = W // 2, H // 2
    unscattered = ~E.scattered[:, y, x]
    assert unscattered.any() and E.lit_sun[unscattered, y, x].all() and not E.lit_sky[unscattered, y, x].any()
    P = _scene(vp, oracle, "soft", 0, 1, camera=view)
    p = Pair(vp)
    try:
        _same(p.render(frames[0], len(frames), P), (E.sun, E.sky), "sun-axis camera")
    finally:
        p.free()
    power = np.asarray(scenes.DEFAULT_SUN_POWER, F32)
    assert E.sun[y, x, 0] > 0.01 * power[0]              # the disc's value is in the sun group: orders of magnitude above any sky


def test_subpixel_factor_2_against_the_oracle_on_the_fine_image(vp, oracle, ctx):
    """vp_set_subpixel(2) at 8 x 6 against the oracle's twins at 16 x 12, gathered by vp_subpixel_offset"""
    w, h = W // 2, H // 2
    for name, est in (("julia", 1), ("soft", 0)):
        fine = {f: GL.expected(oracle, name, est, 1, frames=(f,)) for f in FRAMES}
        P = _scene(vp, oracle, name, est, 1, size=(w, h))
        want = tuple(subpixel_lib.accumulate(vp, w, h, 2, FIRST, N, lambda f, k=k: (fine[f].sun, fine[f].sky)[k]) for k in (0, 1))
        p = Pair(vp, w, h)
        try:
            vp.set_subpixel(2)
            _same(p.render(FIRST, N, P), want, (name, est, "S = 2"))
        finally:
            vp.set_subpixel(1)
            p.free()
        assert want[0][..., :3].max() > 0 and want[1][..., :3].max() > 0


def test_three_shards_sum_to_the_whole(vp, oracle, ctx):
    E = GL.expected(oracle, "soft", 0, 1)
    P = _scene(vp, oracle, "soft", 0, 1)
    whole, part = Pair(vp), Pair(vp)
    try:
        for r in range(3):
            vp.set_shard(r, 3)
            part.reset()
            a, k = part.render(FIRST, N, P)
            owned = np.array([[vp.tile_owner(x // 8, y // 8, 3) == r for x in range(W)] for y in range(H)])
            assert not a[~owned].any() and not k[~owned].any()      # a shard touches its own pixels only
            vp.accumulate(whole.sun.ptr, part.sun.ptr, W * H)
            vp.accumulate(whole.sky.ptr, part.sky.ptr, W * H)
        vp.set_shard(0, 1)
        _same((whole.sun.download(), whole.sky.download()), (E.sun, E.sky), "three shards")
    finally:
        vp.set_shard(0, 1)
        whole.free()
        part.free()


# -------------------------------------------------------------------------------- against the library's own renders of the twins
@pytest.mark.parametrize("name,est", (("julia", 0), ("julia", 1), ("soft", 2)))
def test_groups_equal_two_gpu_renders_of_the_twins(vp, oracle, ctx, name, est):
    """no oracle: 64 x 48, one launch of 70 frames; the sun accumulator is vp_render_frames with init_envmap(zeros), the sky
    accumulator vp_render_frames after set_sun(dir, 0)"""
    size, first, n = (64, 48), LONG[0], len(LONG)
    P = _scene(vp, oracle, name, est, 1, size=size)
    p, b = Pair(vp, *size), vp.DeviceBuffer(*size)
    try:
        got = p.render(first, n, P)
        _scene(vp, oracle, name, est, 1, size=size, env=np.zeros_like(GL.ENV))
        vp.render_frames(b.ptr, first, n, P)
        sun = b.download()
        _scene(vp, oracle, name, est, 1, size=size, sun_power=ZERO)
        b.reset()
        vp.render_frames(b.ptr, first, n, P)
        sky = b.download()
        assert got[0].tobytes() == sun.tobytes(), int((got[0] != sun).any(-1).sum())
        assert got[1].tobytes() == sky.tobytes(), int((got[1] != sky).any(-1).sum())
        assert sun[..., :3].max() > 0 and sky[..., :3].max() > 0 and np.array_equal(sun[..., 3], sky[..., 3])
    finally:
        p.free()
        b.free()


@pytest.mark.parametrize("name,est", (("julia", 1), ("soft", 2)))
def test_the_call_leaves_nothing_behind(vp, oracle, ctx, name, est):
    P = _scene(vp, oracle, name, est, 1)
    p, b = Pair(vp), vp.DeviceBuffer(W, H)
    try:
        vp.render_frames(b.ptr, FIRST, N, P)
        before = b.download()
        a, k = p.render(FIRST, N, P)
        assert np.array_equal(a[..., 3], before[..., 3]) and np.array_equal(k[..., 3], before[..., 3])     # both groups carry the beauty w
        b.reset()
        vp.render_frames(b.ptr, FIRST, N, P)            # after a groups call: the bits it rendered before
        assert np.array_equal(b.download(), before)
        b.reset()
        for f in FRAMES:
            vp.render_kernel(b.ptr, f, P)               # ... and the direct path
        assert np.array_equal(b.download(), before)
        assert before[..., :3].max() > 0 and (before[..., 3] > 0).any()
    finally:
        p.free()
        b.free()


def test_refusals_return_state_errors_and_touch_no_buffer(vp, oracle, ctx):
    P = _scene(vp, oracle, "soft", 0, 1)
    p = Pair(vp)
    try:
        mark = np.full((H, W, 4), 7.25, F32)
        p.sun.upload(mark)
        p.sky.upload(mark)

        def refused():
            rc = vp.lib().vp_render_frames_groups(p.sun.ptr, p.sky.ptr, FIRST, N, C.byref(P))
            vp.synchronize()
            assert rc == E_STATE, (rc, vp.lib().vp_last_error())
            assert np.array_equal(p.sun.download(), mark) and np.array_equal(p.sky.download(), mark)

        vp.set_envmap_sampling(vp.ENV_MIS)
        refused()
        vp.set_envmap_sampling(vp.ENV_PASSIVE)
        for mode in (vp.TRACK_SCALAR, vp.TRACK_MULTI_CHANNEL):
            vp.set_tracking(mode)
            refused()
        vp.set_tracking(vp.TRACK_SPECTRAL)
        vp.enable_counters(True)
        refused()
        vp.enable_counters(False)
        vp.set_arithmetic(vp.ARITH_FAST)                # the groups instances are the exact unit's
        refused()
        vp.set_arithmetic(vp.ARITH_EXACT)
        p.reset()
        E = GL.expected(oracle, "soft", 0, 1)
        _same(p.render(FIRST, N, P), (E.sun, E.sky), "after the refusals")     # the context stays usable
    finally:
        vp.enable_counters(False)
        vp.set_arithmetic(vp.ARITH_EXACT)
        p.free()


# ---------------------------------------------------------------------------------------------------------------------- vp_relight
def test_relight_with_unit_gains_is_the_scaled_beauty_image_to_rounding(vp, oracle, ctx):
    """vp_relight with gains 1 against `scale` of vp_render_frames' accumulator.  Per sample, sun + sky differs from the beauty sample
    by at most 3 roundings (tests/test_groups_cpu.py); each of the three accumulators adds n samples with one rounding per addition,
    of which the two group accumulators together are compared with one: 2n; the output stage rounds sun * s, sky * s, their sum and
    beauty * s: 4 -- and 4 to spare.  All terms are non-negative, so every rounding is relative to a partial sum of at most the total:
    |relit - beauty * s| <= (2n + 8) * 2^-24 * (sun + sky) * s per channel."""
    P = _scene(vp, oracle, "soft", 1, 1)
    n, s = len(LONG), F32(1.0) / F32(len(LONG))
    p, b, dst = Pair(vp), vp.DeviceBuffer(W, H), vp.DeviceBuffer(W, H)
    try:
        sun, sky = p.render(LONG[0], n, P)
        vp.render_frames(b.ptr, LONG[0], n, P)
        vp.scale(b.ptr, b.ptr, W * H, float(s))
        beauty = b.download()
        vp.relight(dst.ptr, p.sun.ptr, p.sky.ptr, W * H, float(s))
        relit = dst.download()
    finally:
        p.free()
        b.free()
        dst.free()
    mean = (sun[..., :3].astype(np.float64) + sky[..., :3].astype(np.float64)) * float(s)
    err = np.abs(relit[..., :3].astype(np.float64) - beauty[..., :3].astype(np.float64))
    bound = (2 * n + 8) * 2.0 ** -24 * mean
    print("relight against beauty: worst error / bound %.4f" % float((err[mean > 0] / bound[mean > 0]).max()))
    assert (err <= bound).all(), float((err[mean > 0] / bound[mean > 0]).max())
    assert np.array_equal(relit[..., 3], beauty[..., 3]) and mean.max() > 0            # w = sun.w * s: the beauty heat, scaled


def test_relight_equals_the_numpy_restatement(vp, oracle, ctx):
    E = GL.expected(oracle, "soft", 1, 1)
    s = F32(1.0) / F32(N)
    gs, gk = (2.0, 0.5, 0.0), (0.0, 1.0, 3.0)
    sun, sky, dst = (vp.DeviceBuffer(W, H) for _ in range(3))
    try:
        sun.upload(E.sun)
        sky.upload(E.sky)
        vp.relight(dst.ptr, sun.ptr, sky.ptr, W * H, float(s), gs, gk)
        want = GL.relight(E.sun, E.sky, s, gs, gk)
        assert dst.download().tobytes() == want.tobytes()
        vp.relight(sun.ptr, sun.ptr, sky.ptr, W * H, float(s), gs, gk)         # in place: dst == sun
        assert sun.download().tobytes() == want.tobytes()
        assert want[..., 0].max() > 0 and want[..., 2].max() > 0 and (want[..., 1] > 0).all()
    finally:
        for b in (sun, sky, dst):
            b.free()
