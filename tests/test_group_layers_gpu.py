"""Group layers on the GPU (include/volpath.h vp_render_frames_group_layers, its _stats form and vp_relight_composite; DESIGN.md
section 2.10).

Every comparison is at tolerance 0: accumulators against the oracle-built expectation of tests/group_layers_lib.py (the definition's
table folded over the samples of layers_lib and groups_lib) with np.array_equal, records by their bits against plane_stats_lib's fold,
the library's own calls -- vp_render_frames_layers on the real scene and on the two twin scenes, the three-step output sequence -- by
their bytes.  Each test runs in a context of its own."""
import ctypes as C

import numpy as np
import pytest

import adaptive_lib as AL
import group_layers_lib as GLL
import groups_lib as GL
import layers_lib as LL
import plane_stats_lib as PS
import scenes
import subpixel_lib

pytestmark = pytest.mark.gpu

W, H, FRAMES, LONG = GLL.W, GLL.H, GLL.FRAMES, GLL.LONG
FIRST, N = FRAMES[0], len(FRAMES)
E_STATE = -2
F32 = np.float32
ZERO = (0.0, 0.0, 0.0)
NAMES = GLL.PLANES


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
    vp.init_envmap(GLL.ENV if env is None else env)
    vp.set_sun(scenes.DEFAULT_SUN_DIR, sun_power)
    if camera is None:
        vp.set_camera()
    else:
        vp.set_camera([float(v) for v in np.asarray(camera, F32).ravel()])
    vp.set_estimator(est)
    vp.set_rng(rng_mode, GLL.KEY)
    vp.set_tracking(vp.TRACK_SPECTRAL)
    vp.set_envmap_sampling(vp.ENV_PASSIVE)
    vp.set_shard(0, 1)
    if est == 1:
        vp.precompute_opacity(scenes.DEFAULT_SUN_DIR)
    return vp.make_param(size[0], size[1], **LL.param_kw(name))


class Planes:
    """the three accumulators and the three record buffers of a group-layers call"""

    def __init__(self, vp, w=W, h=H):
        self.vp = vp
        self.acc = tuple(vp.DeviceBuffer(w, h) for _ in NAMES)
        self.rec = tuple(vp.StatsBuffer(w, h) for _ in NAMES)

    def plain(self, first, n, P):
        self.vp.render_frames_group_layers(*[b.ptr for b in self.acc], first, n, P)
        return tuple(b.download() for b in self.acc)

    def stats(self, first, n, P):
        self.vp.render_frames_group_layers_stats(*[b.ptr for b in self.acc + self.rec], first, n, P)
        return tuple(b.download() for b in self.acc + self.rec)

    def reset(self):
        for b in self.acc + self.rec:
            b.reset()

    def free(self):
        for b in self.acc + self.rec:
            b.free()


def _same(got, want, what):
    for k, name in enumerate(NAMES):
        assert np.array_equal(got[k], want[k], equal_nan=True), (what, name, "%d pixels" % int((got[k] != want[k]).any(-1).sum()))


def _same_rec(got, want, what, flags=None):
    for k, name in enumerate(NAMES):
        bad = PS.same_records(want[k], got[k], flags)
        assert bad is None, (what, name, bad)


# ------------------------------------------------------------------------------------------------------- against the expectation
CASES = [("soft", e, r) for e in (0, 1, 2) for r in (0, 1, 2)] + [(n, e, r) for n in ("julia", "soft16") for e in (0, 1) for r in (0, 2)]


@pytest.mark.parametrize("name,est,rng_mode", CASES, ids=["%s-est%d-rng%d" % c for c in CASES])
def test_planes_and_records_equal_the_expectation(vp, oracle, ctx, name, est, rng_mode):
    E = GLL.expected(oracle, name, est, rng_mode)
    want, records = E.accs(), E.stats()
    P = _scene(vp, oracle, name, est, rng_mode)
    general, light, miss = vp.pixel_lists(P)
    p = Planes(vp)
    try:
        one = p.plain(FIRST, N, P)                      # batched: one staged launch
        _same(one, want, (name, est, rng_mode, "batched"))
        assert not any(r.download()["n"].any() for r in p.rec), "the plain call wrote records"
        p.reset()
        for f in FRAMES:                                # frame by frame: staged too; two calls give the bits of one
            single = p.plain(f, 1, P)
        _same(single, want, (name, est, rng_mode, "frame by frame"))
        p.reset()
        got = p.stats(FIRST, N, P)                      # the _stats form: the plain call's accumulators by their bytes, the fold's records
        assert [a.tobytes() for a in got[:3]] == [a.tobytes() for a in one], (name, est, rng_mode, "_stats accumulators")
        _same_rec(got[3:], records, (name, est, rng_mode, "_stats"))
        p.reset()
        p.stats(FIRST, 1, P)                            # no hidden state: a second call continues a first
        got = p.stats(FIRST + 1, N - 1, P)
        _same(got[:3], want, (name, est, rng_mode, "_stats, 1 + 1"))
        _same_rec(got[3:], records, (name, est, rng_mode, "_stats, 1 + 1"))
    finally:
        p.free()
    g = E.groups()
    assert g["miss"] >= 1 and g["scattered"] + g["mixed"] >= 1 and len(miss) == g["miss"] and len(general) > 0, g
    if name == "julia":
        assert len(light) > 0 and g["unscattered"] >= 1, g      # (all four groups at once: tests/test_group_layers_cpu.py, stream 1)
    assert want[0][..., :3].max() > 0 and want[1][..., :3].max() > 0 and want[2][..., :3].max() > 0
    assert (records[2].sum_y > 0).any() and (records[0].sum_y == 0).any()


@pytest.mark.parametrize("est,density,const", ((0, 61.0, False), (0, 64.0, True), (1, 61.0, False), (2, 61.0, False)))
def test_light_class_as_a_kernel_and_as_constants(vp, oracle, ctx, est, density, const):
    """The light pixel class of the Julia set (tests/test_layers_gpu.py has the reasons for the two densities): at a majorant of 61 a
    null collision in empty space moves the throughput and the light kernel runs, whose samples carry no mark and have no word in the
    second plane; at 64 it is neutral and the class is written as constants, marked, in the first plane only."""
    E = GLL.expected(oracle, "julia", est, 1, density=density)
    want, records = E.accs(), E.stats()
    P = _scene(vp, oracle, "julia", est, 1)
    P.density = density
    general, light, miss = vp.pixel_lists(P)
    assert len(light) > 0 and len(miss) > 0 and len(general) > 0
    p = Planes(vp)
    try:
        for first, n in ((FIRST, N), (FIRST, 1)):
            p.reset()
            p.plain(first, n, P)
            assert vp.last_light_const() == const
        _same(p.plain(FIRST + 1, 1, P), want, (density, "one frame, then the next"))
        p.reset()
        got = p.stats(FIRST, N, P)
        _same(got[:3], want, (density, "batched, _stats"))
        _same_rec(got[3:], records, (density, "batched, _stats"))
    finally:
        p.free()
    ly, lx = light >> 16, light & 0xffff
    assert not want[0][ly, lx][:, :3].any() and not want[1][ly, lx][:, :3].any() and (want[2][ly, lx][:, 3] == N).all()     # the class never scatters


@pytest.mark.parametrize("name,est", (("julia", 0), ("julia", 1), ("soft", 1)))
def test_a_launch_of_70_frames_and_its_split_into_two_calls(vp, oracle, monkeypatch, name, est):
    """one launch of 64 frames or more: the approach walks hand their samples over (VP_DENSE_PERCENT=101: never too dense to walk), the
    constants of the launch are staged once, in the first plane; a call of 2 frames followed by a call of 68 leaves the bits of one"""
    E = GLL.expected(oracle, name, est, 1, frames=LONG)
    want, records = E.accs(), E.stats()
    monkeypatch.setenv("VP_DENSE_PERCENT", "101")
    c = vp.Context(0)
    monkeypatch.delenv("VP_DENSE_PERCENT")
    try:
        with c:
            P = _scene(vp, oracle, name, est, 1)
            p = Planes(vp)
            try:
                got = p.stats(LONG[0], len(LONG), P)
                if name == "julia":
                    assert vp.last_approach_mode() != 0, "the approach walk did not run"
                _same(got[:3], want, (name, est, "70 frames"))
                _same_rec(got[3:], records, (name, est, "70 frames"))
                p.reset()
                _same(p.plain(LONG[0], len(LONG), P), want, (name, est, "70 frames, plain"))
                p.reset()
                p.stats(LONG[0], 2, P)
                got = p.stats(LONG[0] + 2, len(LONG) - 2, P)
                _same(got[:3], want, (name, est, "2 + 68 frames"))
                _same_rec(got[3:], records, (name, est, "2 + 68 frames"))
            finally:
                p.free()
    finally:
        c.destroy()
    assert E.miss.any() and E.unscattered.any() and not E.unscattered.all()


def test_a_staging_cap_that_splits_the_call_into_launches(vp, oracle, monkeypatch):
    """VP_STAGE_MB=1 in a context of its own: 160 x 120 pixels are 300 KiB of staging per frame and plane, so a call of 8 frames is
    eight launches of the two-plane staging, as for a groups call -- and leaves the bits of the one launch of an uncapped context"""
    size, n = (160, 120), 8
    out = []
    for cap in (None, "1"):
        if cap:
            monkeypatch.setenv("VP_STAGE_MB", cap)
        c = vp.Context(0)
        monkeypatch.delenv("VP_STAGE_MB", raising=False)
        try:
            with c:
                P = _scene(vp, oracle, "julia", 1, 1, size=size)
                p = Planes(vp, *size)
                try:
                    assert vp.groups_frames_per_launch(P, 2) >= (n if cap is None else 1)
                    vp.synchronize()
                    vp.render_time_ms(reset=True)
                    got = p.stats(FIRST, n, P)
                    out.append((vp.render_time_ms(reset=True)[1], [a.tobytes() for a in got]))
                    assert all((got[3 + k]["n"] == n).all() for k in range(3)) and (got[5]["sum_y"] > 0).any() and (got[4]["sum_y"] > 0).any()
                finally:
                    p.free()
        finally:
            c.destroy()
    assert out[0][0] == 1 and out[1][0] == 8, (out[0][0], out[1][0])
    assert out[0][1] == out[1][1]


# -------------------------------------------------------------------------------- against the library's own calls
@pytest.mark.parametrize("name,est", (("julia", 0), ("julia", 1), ("soft", 2)))
def test_planes_equal_the_layers_renders_of_the_scene_and_its_twins(vp, oracle, ctx, name, est):
    """no oracle: 64 x 48, one launch of 70 frames.  trans is vp_render_frames_layers' trans; sun its fg with init_envmap(zeros); sky its
    fg after set_sun(dir, 0); the three w are equal bits.  On the pixels that scattered in every frame (trans.w == 0) sun and sky are
    vp_render_frames_groups' accumulators."""
    size, first, n = (64, 48), LONG[0], len(LONG)
    P = _scene(vp, oracle, name, est, 1, size=size)
    p = Planes(vp, *size)
    fg, tr = vp.DeviceBuffer(*size), vp.DeviceBuffer(*size)

    def layers():
        fg.reset()
        tr.reset()
        vp.render_frames_layers(fg.ptr, tr.ptr, first, n, P)
        return fg.download(), tr.download()
    try:
        sun, sky, trans = p.plain(first, n, P)
        real = layers()
        fg.reset()
        tr.reset()
        vp.render_frames_groups(fg.ptr, tr.ptr, first, n, P)
        gsun, gsky = fg.download(), tr.download()
        _scene(vp, oracle, name, est, 1, size=size, env=np.zeros_like(GLL.ENV))
        no_env = layers()
        _scene(vp, oracle, name, est, 1, size=size, sun_power=ZERO)
        no_sun = layers()
    finally:
        p.free()
        fg.free()
        tr.free()
    assert trans.tobytes() == real[1].tobytes() == no_env[1].tobytes() == no_sun[1].tobytes()
    assert sun.tobytes() == no_env[0].tobytes(), int((sun != no_env[0]).any(-1).sum())
    assert sky.tobytes() == no_sun[0].tobytes(), int((sky != no_sun[0]).any(-1).sum())
    assert sun[..., 3].tobytes() == sky[..., 3].tobytes() == real[0][..., 3].tobytes()
    always = trans[..., 3] == 0
    assert np.array_equal(sun[always], gsun[always]) and np.array_equal(sky[always], gsky[always])
    assert always.any() or name != "julia"              # (the soft volume is thin: every pixel gets through unscattered in some of 70 frames)
    assert sun[..., :3].max() > 0 and sky[..., :3].max() > 0 and trans[..., :3].max() > 0 and (trans[..., 3] == n).any()


def test_sun_disc_pixel_is_a_transmittance_sample(vp, oracle, ctx):
    """a camera whose axis is the sun direction: pixel (W/2, H/2) looks into the disc.  Its unscattered samples, which a groups call
    gives to the sun group with the disc's value, are transmittance samples here: nothing in sun RGB, their throughput in trans"""
    view = GL.sun_axis_view()
    frames = tuple(range(10, 16))
    E = GLL.expected(oracle, "soft", 0, 1, frames=frames, inv_view=view)
    x, y = W // 2, H // 2
    u = E.unscattered[:, y, x]
    assert u.any() and E.gsun[u, y, x, :3].any(-1).all() and not E.sun[u, y, x, :3].any() and (E.trans[u, y, x, :3] > 0).all()
    P = _scene(vp, oracle, "soft", 0, 1, camera=view)
    p = Planes(vp)
    try:
        got = p.plain(frames[0], len(frames), P)
        _same(got, E.accs(), "sun-axis camera")
    finally:
        p.free()
    assert got[2][y, x, 3] == u.sum() and got[0][y, x, 0] < E.acc("gsun")[y, x, 0]       # the disc's value, a groups call's sun sample, is in no plane


def test_subpixel_factor_2_against_the_expectation_on_the_fine_image(vp, oracle, ctx):
    """vp_set_subpixel(2) at 8 x 6 against the expectation at 16 x 12, gathered by vp_subpixel_offset"""
    w, h = W // 2, H // 2
    for name, est in (("julia", 1), ("soft", 0)):
        E = GLL.expected(oracle, name, est, 1)
        P = _scene(vp, oracle, name, est, 1, size=(w, h))
        want = tuple(subpixel_lib.accumulate(vp, w, h, 2, FIRST, N, lambda f, k=k: getattr(E, k)[f - FIRST]) for k in NAMES)
        p = Planes(vp, w, h)
        try:
            vp.set_subpixel(2)
            _same(p.plain(FIRST, N, P), want, (name, est, "S = 2"))
        finally:
            vp.set_subpixel(1)
            p.free()
        assert all(a[..., :3].max() > 0 for a in want)


def test_three_shards_sum_to_the_whole_and_touch_their_own_records(vp, oracle, ctx):
    E = GLL.expected(oracle, "soft", 0, 1)
    want, records = E.accs(), E.stats()
    P = _scene(vp, oracle, "soft", 0, 1)
    sentinel = np.zeros((H, W), vp.PIXEL_STATS_DTYPE)
    sentinel["sum_y"], sentinel["sum_y2"], sentinel["n"], sentinel["flags"] = -7.25, 1e300, 0xabcd0123, 0xfffffff0
    whole_rec = [np.zeros((H, W), vp.PIXEL_STATS_DTYPE) for _ in NAMES]
    whole, part = Planes(vp), Planes(vp)
    seen = np.zeros((H, W), int)
    try:
        for r in range(3):
            vp.set_shard(r, 3)
            owned = AL.owned_pixels(vp, W, H, r, 3)
            part.reset()
            for b in part.rec:
                b.upload(sentinel)
            got = part.stats(FIRST, N, P)
            for k in range(3):
                assert got[3 + k][~owned].tobytes() == sentinel[~owned].tobytes(), (r, NAMES[k])     # unowned records: untouched
                assert not got[k][~owned].any()                                                      # a shard touches its own pixels only
            part.reset()
            got = part.stats(FIRST, N, P)
            for k in range(3):
                whole_rec[k][owned] = got[3 + k][owned]
                vp.accumulate(whole.acc[k].ptr, part.acc[k].ptr, W * H)
            seen += owned
        vp.set_shard(0, 1)
        assert (seen == 1).all()
        _same(tuple(b.download() for b in whole.acc), want, "three shards")
        _same_rec(whole_rec, records, "three shards")
    finally:
        vp.set_shard(0, 1)
        whole.free()
        part.free()


def test_flags_are_neither_read_nor_written(vp, oracle, ctx):
    E = GLL.expected(oracle, "julia", 1, 1)
    P = _scene(vp, oracle, "julia", 1, 1)
    board = np.zeros((H, W), vp.PIXEL_STATS_DTYPE)
    yy, xx = np.mgrid[0:H, 0:W]
    board["flags"] = (((xx + yy) % 2) * AL.FROZEN + (xx % 3 == 0) * 0x5a000000).astype(np.uint32)
    p = Planes(vp)
    try:
        for b in p.rec:
            b.upload(board)
        got = p.stats(FIRST, N, P)
        _same(got[:3], E.accs(), "a board of flags")
        _same_rec(got[3:], E.stats(), "a board of flags", flags=board["flags"])      # frozen pixels are sampled like the others
    finally:
        p.free()


# ------------------------------------------------------------------------------------------------------------- no side effects
@pytest.mark.parametrize("name,est", (("julia", 1), ("soft", 2)))
def test_the_call_leaves_nothing_behind(vp, oracle, ctx, name, est):
    """a beauty, a groups and a layers render after the call give the bits they gave before it; the launch counters of the existing
    tables do not move during it, and those tables hold the instances they held"""
    P = _scene(vp, oracle, name, est, 1)
    p, a, b = Planes(vp), vp.DeviceBuffer(W, H), vp.DeviceBuffer(W, H)

    def others():
        out = []
        a.reset()
        vp.render_frames(a.ptr, FIRST, N, P)
        out.append(a.download().tobytes())
        a.reset()
        for f in FRAMES:
            vp.render_kernel(a.ptr, f, P)               # ... and the direct path
        out.append(a.download().tobytes())
        for call in (vp.render_frames_groups, vp.render_frames_layers):
            a.reset()
            b.reset()
            call(a.ptr, b.ptr, FIRST, N, P)
            out += [a.download().tobytes(), b.download().tobytes()]
        return out
    try:
        before = others()
        assert before[0] == before[1]
        tables = lambda: (vp.launch_census(vp.CENSUS_EXACT, vp.CENSUS_RENDER), vp.launch_census(vp.CENSUS_EXACT, vp.CENSUS_LAYERS), vp.groups_census(),
                          vp.launch_census(vp.CENSUS_FAST, vp.CENSUS_RENDER))
        t0, own0 = tables(), sum(vp.group_layers_census().values())
        one = p.plain(FIRST, N, P)
        p.reset()
        p.stats(FIRST, N, P)
        assert tables() == t0 and sum(vp.group_layers_census().values()) > own0
        assert len(t0[1]) == len(t0[2]) == 79 and set(t0[1]) == set(t0[2]) == set(vp.group_layers_census())
        assert others() == before
        p.reset()
        assert [x.tobytes() for x in p.plain(FIRST, N, P)] == [x.tobytes() for x in one]
        beauty = np.frombuffer(before[0], F32).reshape(H, W, 4)
        assert beauty[..., :3].max() > 0 and np.array_equal(one[0][..., 3], beauty[..., 3]) and np.array_equal(one[1][..., 3], beauty[..., 3])
    finally:
        p.free()
        a.free()
        b.free()


@pytest.mark.parametrize("with_stats", (False, True), ids=("plain", "stats"))
def test_refusals_return_state_errors_and_touch_no_buffer(vp, oracle, ctx, with_stats):
    P = _scene(vp, oracle, "soft", 0, 1)
    E = GLL.expected(oracle, "soft", 0, 1)
    p = Planes(vp)
    try:
        mark = np.full((H, W, 4), 7.25, F32)
        sentinel = np.zeros((H, W), vp.PIXEL_STATS_DTYPE)
        sentinel["sum_y"], sentinel["sum_y2"], sentinel["n"], sentinel["flags"] = -7.25, 1e300, 0xabcd0123, 0xfffffff0
        for b in p.acc:
            b.upload(mark)
        for b in p.rec:
            b.upload(sentinel)
        ptrs = [b.ptr for b in (p.acc + p.rec if with_stats else p.acc)]
        f = vp.lib().vp_render_frames_group_layers_stats if with_stats else vp.lib().vp_render_frames_group_layers

        def refused():
            rc = f(*ptrs, FIRST, N, C.byref(P))
            vp.synchronize()
            assert rc == E_STATE, (rc, vp.lib().vp_last_error())
            assert all(np.array_equal(b.download(), mark) for b in p.acc)
            assert all(b.download().tobytes() == sentinel.tobytes() for b in p.rec)

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
        vp.set_arithmetic(vp.ARITH_FAST)                # the instances are the exact unit's
        refused()
        vp.set_arithmetic(vp.ARITH_EXACT)
        p.reset()
        got = p.stats(FIRST, N, P) if with_stats else p.plain(FIRST, N, P)
        _same(got[:3], E.accs(), "after the refusals")     # the context stays usable
    finally:
        vp.enable_counters(False)
        vp.set_arithmetic(vp.ARITH_EXACT)
        p.free()


# -------------------------------------------------------------------------------------------------------------- the output stage
@pytest.mark.parametrize("plate", (False, True), ids=("constant", "plate"))
def test_relight_composite_equals_the_three_steps_and_the_restatement(vp, oracle, ctx, plate):
    """vp_relight_composite against vp_relight, scale and vp_composite with a scale of 1 on the device, and against the numpy
    restatement; out of place and in place into each of its three inputs"""
    E = GLL.expected(oracle, "soft", 1, 1)
    planes = [a.copy() for a in E.accs()]
    rng = np.random.default_rng(9)
    planes[0][0, :4] = F32(-0.0)                        # negative zeros and denormals among the inputs
    planes[1][0, 4:8, :3] = F32(2.0 ** -140)
    planes[2][1, :4, :3] = F32(-3.0 * 2.0 ** -149)
    back = (rng.random((H, W, 4)) * 4.0).astype(F32)
    s = F32(1.0) / F32(N)
    gs, gk, rgb = (2.0, 0.5, 0.0), (0.0, 1.0, 3.0), (0.7, 0.1, 9.0)
    kw = dict(plate=back) if plate else dict(rgb=rgb)
    want = GLL.relight_composite(*planes, s, gs, gk, **kw)
    assert want.tobytes() == GLL.three_steps(*planes, s, gs, gk, **kw).tobytes()
    bufs = [vp.DeviceBuffer(W, H) for _ in range(7)]
    sun, sky, trans, dst, tmp, t, bg = bufs
    try:
        def load():
            for b, a in zip((sun, sky, trans, bg), planes + [back]):
                b.upload(a)
        load()
        pk = dict(plate_ptr=bg.ptr) if plate else dict(plate_rgb=rgb)
        vp.relight(tmp.ptr, sun.ptr, sky.ptr, W * H, float(s), gs, gk)
        vp.scale(t.ptr, trans.ptr, W * H, float(s))
        vp.composite(dst.ptr, tmp.ptr, t.ptr, W * H, 1.0, **pk)
        steps = dst.download()
        assert steps.tobytes() == want.tobytes()
        dst.reset()
        vp.relight_composite(dst.ptr, sun.ptr, sky.ptr, trans.ptr, W * H, float(s), gs, gk, **pk)
        assert dst.download().tobytes() == steps.tobytes()
        for target in (sun, sky, trans):                # in place
            load()
            vp.relight_composite(target.ptr, sun.ptr, sky.ptr, trans.ptr, W * H, float(s), gs, gk, **pk)
            assert target.download().tobytes() == steps.tobytes()
        assert want[..., :3].max() > 0 and (want[..., 3] < 1).any() and (want[..., 3] > 0).any()
    finally:
        for b in bufs:
            b.free()
