"""Compositing layers on the GPU (include/volpath.h vp_render_frames_layers / vp_composite).

Every comparison is at tolerance 0 (np.array_equal): against the oracle-built expectation of tests/layers_lib.py, against the library's
own other ways of rendering the same samples, or against the numpy restatement of vp_composite.  The one statistical test is the
oracle-free slab pin at the end, with the constants and bounds of the slab-transmittance pin of tests/test_pins_gpu.py.  Each test runs
in a context of its own."""
import ctypes as C

import numpy as np
import pytest

import layers_lib as LL
import scenes
import subpixel_lib
from long_ray_cases import camera_rays64, slab64

pytestmark = pytest.mark.gpu

W, H, FRAMES, LONG = LL.W, LL.H, LL.FRAMES, LL.LONG
FIRST, N = FRAMES[0], len(FRAMES)
E_STATE = -2
F32 = np.float32


@pytest.fixture
def ctx(vp):
    c = vp.Context(0)
    try:
        with c:
            yield c
    finally:
        c.destroy()


def _scene(vp, oracle, name, est, rng_mode, opacity=None, density=None):
    g = LL.grid_of(name, oracle)
    vp.init_volume(g, brick=1, linear=True)
    assert vp.volume_info()["format"] == {"julia": vp.VOL_U8, "soft": vp.VOL_F32, "soft16": vp.VOL_F16}[name]
    vp.init_envmap(LL.ENV)
    vp.set_sun(scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER)
    vp.set_camera()
    vp.set_estimator(est)
    vp.set_rng(rng_mode, LL.KEY)
    vp.set_tracking(vp.TRACK_SPECTRAL)
    vp.set_envmap_sampling(vp.ENV_PASSIVE)
    vp.set_shard(0, 1)
    if est == 1 if opacity is None else opacity:
        vp.precompute_opacity(scenes.DEFAULT_SUN_DIR)
    return vp.make_param(W, H, **dict(LL.param_kw(name), **({} if density is None else {"density": density})))


class Pair:
    """the two accumulators of a layers call"""

    def __init__(self, vp, w=W, h=H):
        self.vp, self.fg, self.tr = vp, vp.DeviceBuffer(w, h), vp.DeviceBuffer(w, h)

    def render(self, first, n, P):
        self.vp.render_frames_layers(self.fg.ptr, self.tr.ptr, first, n, P)
        return self.fg.download(), self.tr.download()

    def reset(self):
        self.fg.reset()
        self.tr.reset()

    def free(self):
        self.fg.free()
        self.tr.free()


def _same(got, want, what):
    assert np.array_equal(got[0], want[0], equal_nan=True), (what, "fg", int((got[0] != want[0]).any(-1).sum()))
    assert np.array_equal(got[1], want[1], equal_nan=True), (what, "trans", int((got[1] != want[1]).any(-1).sum()))


# ------------------------------------------------------------------------------------------------------- against the oracle
CASES = [("soft", e, r) for e in (0, 1, 2) for r in (0, 1, 2)] + [(n, e, 1) for n in ("julia", "soft16") for e in (0, 1)]


@pytest.mark.parametrize("name,est,rng_mode", CASES, ids=["%s-est%d-rng%d" % c for c in CASES])
def test_layers_equal_the_oracle_expectation(vp, oracle, ctx, name, est, rng_mode):
    E = LL.expected(oracle, name, est, rng_mode)
    P = _scene(vp, oracle, name, est, rng_mode)
    p = Pair(vp)
    try:
        got = p.render(FIRST, N, P)                     # batched: one staged launch
        _same(got, (E.fg, E.trans), (name, est, rng_mode, "batched"))
        p.reset()
        for f in FRAMES:                                # frame by frame: staged too (the direct path has no second target)
            single = p.render(f, 1, P)
        _same(single, (E.fg, E.trans), (name, est, rng_mode, "frame by frame"))
    finally:
        p.free()
    # the test means something: all three kinds of sample occur, and transmittance is not just 0 or 1 on the chromatic volume
    assert E.unscattered.any() and not E.unscattered.all() and E.miss.any()
    assert E.fg[..., :3].max() > 0 and np.isfinite(E.fg).all() and np.isfinite(E.trans).all()


@pytest.mark.parametrize("est,density,const", ((0, 61.0, False), (0, 64.0, True), (1, 61.0, False), (2, 61.0, False)))
def test_light_class_as_a_kernel_and_as_constants(vp, oracle, ctx, est, density, const):
    """The light pixel class (camera rays through certified-empty cells only) of the Julia set.  A majorant of 61 has a reciprocal
    that does not multiply back to 1: a null collision in empty space moves the throughput, so the light kernel runs -- the
    global-majorant one and the local-majorant ones of the decomposition and bounded estimators.  Its samples carry no mark:
    the reduce is told their slots, and a sample it took for a foreground sample would put the throughput into fg.  At 64 the
    collision is neutral and the class is written as constants (1, 1, 1, -0.0f), like the box-missing pixels."""
    E = LL.expected(oracle, "julia", est, 1, density=density)
    P = _scene(vp, oracle, "julia", est, 1, density=density)
    general, light, miss = vp.pixel_lists(P)
    assert len(light) > 0 and len(miss) > 0 and len(general) > 0
    p = Pair(vp)
    try:
        for first, n in ((FIRST, N), (FIRST, 1)):
            p.reset()
            got = p.render(first, n, P)
            assert vp.last_light_const() == const
        _same(p.render(FIRST + 1, 1, P), (E.fg, E.trans), (density, "one frame, then the next"))
        p.reset()
        _same(p.render(FIRST, N, P), (E.fg, E.trans), (density, "batched"))
    finally:
        p.free()
    ly, lx = light >> 16, light & 0xffff
    t = E.trans[ly, lx]
    assert (t[:, 3] == N).all() and not E.fg[ly, lx][:, :3].any()          # every sample of the class is unscattered
    if est == 0:
        assert (t[:, :3] == F32(N)).all() == const                         # ... with a throughput of exactly 1, or not


@pytest.mark.parametrize("name,est", (("julia", 0), ("julia", 1), ("soft", 1)))
def test_a_launch_of_70_frames_equals_the_oracle_expectation(vp, oracle, monkeypatch, name, est):
    """one launch of 64 frames or more: the approach walks hand their samples over (in a context that never takes the volume for too
    dense to walk: VP_DENSE_PERCENT=101), the constants of the launch are staged once"""
    E = LL.expected(oracle, name, est, 1, frames=LONG)
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
                _same(got, (E.fg, E.trans), (name, est))
            finally:
                p.free()
    finally:
        c.destroy()
    g = E.groups()
    assert min(g.values()) >= (1 if name == "julia" else 0) and g["mixed"] >= 1, g


# -------------------------------------------------------------------------------- against the library's other ways to the same samples
def test_two_shards_merged_with_accumulate(vp, oracle, ctx):
    E = LL.expected(oracle, "soft", 0, 1)
    P = _scene(vp, oracle, "soft", 0, 1)
    whole, part = Pair(vp), Pair(vp)
    try:
        for r in range(2):
            vp.set_shard(r, 2)
            part.reset()
            fg, tr = part.render(FIRST, N, P)
            owned = np.array([[vp.tile_owner(x // 8, y // 8, 2) == r for x in range(W)] for y in range(H)])
            assert not fg[~owned].any() and not tr[~owned].any()    # a shard touches its own pixels only
            vp.accumulate(whole.fg.ptr, part.fg.ptr, W * H)
            vp.accumulate(whole.tr.ptr, part.tr.ptr, W * H)
        vp.set_shard(0, 1)
        _same((whole.fg.download(), whole.tr.download()), (E.fg, E.trans), "two shards")
    finally:
        vp.set_shard(0, 1)
        whole.free()
        part.free()


@pytest.mark.parametrize("name,est", (("julia", 1), ("soft", 0)))
def test_subpixel_factor_2_is_the_gather_of_the_fine_layers(vp, oracle, ctx, name, est):
    """vp_set_subpixel(2) at 16 x 12 against the library's own S = 1 layers at 32 x 24, gathered by vp_subpixel_offset"""
    P = _scene(vp, oracle, name, est, 1)
    fineP = subpixel_lib.fine_of(P, 2)
    fine, p = Pair(vp, 2 * W, 2 * H), Pair(vp)
    try:
        frames = {}
        for f in FRAMES:
            fine.reset()
            frames[f] = fine.render(f, 1, fineP)
        want = tuple(subpixel_lib.accumulate(vp, W, H, 2, FIRST, N, lambda f, k=k: frames[f][k]) for k in (0, 1))
        vp.set_subpixel(2)
        got = p.render(FIRST, N, P)
        _same(got, want, (name, est, "S = 2"))
        assert want[1][..., 3].max() == N and 0 < (want[1][..., 3] == 0).sum() < W * H
    finally:
        vp.set_subpixel(1)
        fine.free()
        p.free()


@pytest.mark.parametrize("name,est", (("julia", 1), ("soft", 2)))
def test_fg_w_is_the_beauty_w_and_the_mode_leaves_nothing_behind(vp, oracle, ctx, name, est):
    P = _scene(vp, oracle, name, est, 1)
    p, b = Pair(vp), vp.DeviceBuffer(W, H)
    try:
        vp.render_frames(b.ptr, FIRST, N, P)
        before = b.download()
        fg, tr = p.render(FIRST, N, P)
        assert np.array_equal(fg[..., 3], before[..., 3])
        b.reset()
        vp.render_frames(b.ptr, FIRST, N, P)            # after a layers call: the bits it rendered before
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
        p.fg.upload(mark)
        p.tr.upload(mark)

        def refused():
            rc = vp.lib().vp_render_frames_layers(p.fg.ptr, p.tr.ptr, FIRST, N, C.byref(P))
            vp.synchronize()
            assert rc == E_STATE, (rc, vp.lib().vp_last_error())
            assert np.array_equal(p.fg.download(), mark) and np.array_equal(p.tr.download(), mark)

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
        vp.set_arithmetic(vp.ARITH_FAST)                # the layers instances are the exact unit's
        refused()
        vp.set_arithmetic(vp.ARITH_EXACT)
        p.reset()
        E = LL.expected(oracle, "soft", 0, 1)
        _same(p.render(FIRST, N, P), (E.fg, E.trans), "after the refusals")     # the context stays usable
    finally:
        vp.enable_counters(False)
        vp.set_arithmetic(vp.ARITH_EXACT)
        p.free()


def test_composite_equals_the_numpy_restatement(vp, oracle, ctx):
    E = LL.expected(oracle, "soft", 1, 1)
    rng = np.random.default_rng(5)
    plate = rng.random((H, W, 4), dtype=np.float32) * F32(3.0)
    rgb = (0.25, 0.5, 1.75)
    s = F32(1.0) / F32(N)
    fg, tr, pl, dst = (vp.DeviceBuffer(W, H) for _ in range(4))
    try:
        fg.upload(E.fg)
        tr.upload(E.trans)
        pl.upload(plate)
        vp.composite(dst.ptr, fg.ptr, tr.ptr, W * H, float(s), plate_ptr=pl.ptr)
        assert np.array_equal(dst.download(), LL.composite(E.fg, E.trans, s, plate=plate))
        vp.composite(dst.ptr, fg.ptr, tr.ptr, W * H, float(s), plate_rgb=rgb)
        want = LL.composite(E.fg, E.trans, s, rgb=rgb)
        assert np.array_equal(dst.download(), want)
        vp.composite(fg.ptr, fg.ptr, tr.ptr, W * H, float(s), plate_rgb=rgb)       # in place
        assert np.array_equal(fg.download(), want)
        cov = want[..., 3]
        assert cov.min() == 0.0 and cov.max() == 1.0 and ((cov > 0) & (cov < 1)).any()     # coverage: missed, covered, mixed
    finally:
        for b in (fg, tr, pl, dst):
            b.free()


# ------------------------------------------------------------------------------------------------------------ oracle-free pin
@pytest.mark.parametrize("est", [0, 2])
def test_transmittance_layer_of_a_homogeneous_slab(vp, ctx, est):
    """The slab-transmittance pin of tests/test_pins_gpu.py (_free_flight: a homogeneous achromatic pure absorber viewed head-on; its
    constants, its bounds) on the transmittance layer: mean trans.x / n is exp(-rho * chord) -- with no environment colour to divide
    out -- and the foreground is empty."""
    Wp, Hp, frames, rho, c = 40, 30, 400, 1.2, 0.8
    env = np.zeros((8, 16, 4), np.float32)
    env[..., :3] = c
    env[..., 3] = 1
    vp.set_tracking(0)
    vp.set_envmap_sampling(0)
    vp.init_volume(np.full((16, 16, 16), 255, np.uint8), brick=1, linear=True)
    vp.init_envmap(env)
    vp.set_sun((1.0, 0.0, 0.0), (0, 0, 0))
    vp.set_camera()
    vp.set_estimator(est)
    vp.set_rng(vp.RNG_PHILOX, (5, est))
    vp.set_shard(0, 1)
    P = vp.make_param(Wp, Hp, density=rho, g=0.0, albedo=(0.0,) * 3, sigma_t=(1, 1, 1))
    p = Pair(vp, Wp, Hp)
    try:
        fg, tr = p.render(0, frames, P)
    finally:
        p.free()
    T_img = tr[..., 0].astype(np.float64) / frames
    o, d = camera_rays64(Wp, Hp)
    hit, tmin, tmax = slab64(o, d)
    chord = np.where(hit, tmax - np.maximum(tmin, 0), 0.0)
    T = np.exp(-rho * chord)
    assert hit.mean() > 0.3 and (chord > 1.5).any()
    se = np.sqrt(np.maximum(T * (1 - T), 1e-6) / frames)
    z = np.abs(T_img - T) / se
    assert np.array_equal(tr[~hit][:, :3], np.full((int((~hit).sum()), 3), frames, F32))    # rays that miss the box: exactly 1 per frame
    assert (z[hit] > 4.5).mean() < 0.01, float((z[hit] > 4.5).mean())   # binomial, 4.5 sigma per pixel
    assert abs(T_img[hit].mean() / T[hit].mean() - 1) < 0.01            # 1 % on the mean over the box
    # a collision of this medium is an absorption: such a path counts as scattered, carries nothing, and leaves both layers' colours alone
    assert not fg[..., :3].any() and (tr[~hit][:, 3] == frames).all() and (tr[..., 3] <= frames).all() and (tr[hit][:, 3] < frames).any()
