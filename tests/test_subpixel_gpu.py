"""GPU suite: anti-aliasing by stratified sub-pixel camera rays (include/volpath.h vp_set_subpixel).

The definition: with factor S the sample of pixel (x, y) in frame f of a W x H image is, bit for bit, the S = 1 sample of pixel
(S x + i, S y + j) in frame f of the S W x S H image, (i, j) = vp_subpixel_offset(x, y, f, S).  Every comparison here is
np.array_equal / tobytes() equality against that gather (tests/subpixel_lib.py): tolerance 0, no pixel left out."""
import ctypes as C

import numpy as np
import pytest

import scenes
import subpixel_lib as sub

pytestmark = pytest.mark.gpu

CAM2 = (0.96, 0.0, 0.28, 0.3, 0.0, 1.0, 0.0, 0.05, -0.28, 0.0, 0.96, -3.9)   # off-centre: the volume sits to one side


@pytest.fixture(autouse=True)
def _restore(vp):
    yield
    vp.set_subpixel(1)
    vp.set_arithmetic(vp.ARITH_EXACT)
    vp.set_lookahead(vp.LOOKAHEAD_DEFAULT)
    vp.set_pipeline(True)
    vp.set_shard(0, 1)
    vp.enable_counters(False)
    vp.set_camera()


def _julia_scene(vp, est, rng_mode, key=(5, 9), n=64, brick=1, cam=None):
    vp.set_subpixel(1)
    vp.init_volume(vp.julia_volume(n), brick=brick, linear=True)
    vp.init_envmap(scenes.synthetic_env())
    vp.set_sun(scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER)
    vp.set_camera() if cam is None else vp.set_camera(cam)
    vp.set_estimator(est)
    vp.set_tracking(0)
    vp.set_envmap_sampling(vp.ENV_PASSIVE)
    vp.set_shard(0, 1)
    vp.set_rng(rng_mode, key)
    if est == vp.EST_DECOMP:
        vp.precompute_opacity(scenes.DEFAULT_SUN_DIR)


def _render(vp, P, calls):
    buf = vp.DeviceBuffer(P.width, P.height)
    try:
        for first, n in calls:
            vp.render_frames(buf.ptr, first, n, P)
        return buf.download()
    finally:
        buf.free()


# ---- 1. against the oracle
@pytest.mark.parametrize("rng_name", ["samplerh", "philox7"])
@pytest.mark.parametrize("est_name", ["global", "decomposition"])
@pytest.mark.parametrize("s", [2, 4])
def test_julia_equals_the_oracle_gather(vp, oracle, s, est_name, rng_name):
    """Julia-64, 48x32, frames 0-19: past the lattice period and, for the decomposition estimator, across the frame-11 switch"""
    W, H, N = 48, 32, 20
    est = vp.EST_GLOBAL if est_name == "global" else vp.EST_DECOMP
    rng_mode = vp.RNG_SAMPLERH if rng_name == "samplerh" else vp.RNG_PHILOX7
    key = (1, 2)
    grid = oracle.julia(64)
    env = scenes.synthetic_env()
    osc = oracle.OracleScene(grid, env, scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER, estimator=est, rng_mode=rng_mode, seed=key)
    if est == vp.EST_DECOMP:
        osc.precompute_opacity()
    want = sub.oracle_expectation(vp, osc, oracle.default_param(W, H), s, 0, N)
    plain = None
    for f in range(N):
        plain, _ = osc.render_frame(oracle.default_param(W, H), f, plain)
    differing = int((want != plain).any(axis=-1).sum())
    print(f"S={s} {est_name} {rng_name}: the gathered image differs from the S = 1 image in {differing} of {W * H} pixels")
    assert differing > W * H // 8   # (the expectation is not the un-jittered image: the test cannot pass by accident)
    _julia_scene(vp, est, rng_mode, key)
    vp.set_subpixel(s)
    P = vp.make_param(W, H)
    got = _render(vp, P, [(0, N)])                      # one staged launch
    assert np.array_equal(got, want), float(np.abs(got - want).max())
    got = _render(vp, P, [(f, 1) for f in range(N)])    # frame by frame: direct accumulation, no staging
    assert np.array_equal(got, want), float(np.abs(got - want).max())
    got = _render(vp, P, [(0, 7), (7, 13)])             # launches that do not start on the lattice period
    assert np.array_equal(got, want), float(np.abs(got - want).max())


def test_soft_chromatic_float_volume_equals_the_oracle_gather(vp, oracle):
    """a soft float volume (control component active), chromatic medium, camera off centre, decomposition estimator across frame 11"""
    W, H, N, s = 48, 32, 20, 4
    grid = oracle.cloud(32)
    env = scenes.synthetic_env()
    key = (77, 3)
    osc = oracle.OracleScene(grid, env, scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER, estimator=vp.EST_DECOMP, rng_mode=vp.RNG_PHILOX, seed=key,
                             inv_view=CAM2)
    osc.precompute_opacity()
    oP = oracle.mat(oracle.default_param(W, H, density=60.0), *scenes.PRESET1)
    want = sub.oracle_expectation(vp, osc, oP, s, 0, N)
    vp.set_subpixel(1)
    vp.init_volume(grid, brick=1, linear=True)
    vp.init_envmap(env)
    vp.set_sun(scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER)
    vp.set_camera(CAM2)
    vp.set_estimator(vp.EST_DECOMP)
    vp.set_tracking(0)
    vp.set_envmap_sampling(vp.ENV_PASSIVE)
    vp.set_rng(vp.RNG_PHILOX, key)
    vp.precompute_opacity(scenes.DEFAULT_SUN_DIR)
    vp.set_subpixel(s)
    P = vp.mat(vp.make_param(W, H, density=60.0), *scenes.PRESET1)
    got = _render(vp, P, [(0, N)])
    assert np.array_equal(got, want), float(np.abs(got - want).max())
    assert (want[..., :3] > 0).any()


# ---- 2. against the library's own S = 1 at a size the oracle is too slow for
@pytest.mark.parametrize("arith", ["exact", "fast"])
@pytest.mark.parametrize("est_name", ["global", "decomposition"])
def test_every_call_pattern_equals_the_gather_of_the_library_s1(vp, est_name, arith):
    """160x120, S = 4 (fine 640x480, one frame at a time with S = 1), frames 5 .. 41 -- not aligned to the period of 16 --: as one
    vp_render_frames call, as several with the pipeline on and off, as render_kernel calls with look-ahead 0 and 256, and as three
    shards summed with vp_accumulate.  All the same bits."""
    W, H, s, first, n = 160, 120, 4, 5, 37
    est = vp.EST_GLOBAL if est_name == "global" else vp.EST_DECOMP
    _julia_scene(vp, est, vp.RNG_PHILOX7, brick=4 if est == vp.EST_DECOMP else 1)
    vp.set_arithmetic(vp.ARITH_FAST if arith == "fast" else vp.ARITH_EXACT)
    vp.set_lookahead(0)
    P = vp.make_param(W, H)
    want = sub.library_expectation(vp, P, s, first, n)   # (leaves the factor at s)
    assert vp.get_subpixel() == s
    plain = None
    vp.set_subpixel(1)
    plain = _render(vp, P, [(first, n)])
    vp.set_subpixel(s)
    assert int((want != plain).any(axis=-1).sum()) > 100   # (not the un-jittered image)
    vp.prepare(P)
    vp.reserve_frames(P, n)
    got = _render(vp, P, [(first, n)])
    assert got.tobytes() == want.tobytes(), ("one call", float(np.abs(got - want).max()))
    assert vp.last_arithmetic() == (vp.ARITH_FAST if arith == "fast" else vp.ARITH_EXACT)
    calls = [(5, 3), (8, 16), (24, 1), (25, 11), (36, 6)]
    for pipeline in (True, False):
        vp.set_pipeline(pipeline)
        got = _render(vp, P, calls)
        assert got.tobytes() == want.tobytes(), ("several calls, pipeline", pipeline)
    vp.set_pipeline(True)
    for la in (0, vp.LOOKAHEAD_DEFAULT):
        vp.set_lookahead(la)
        buf = vp.DeviceBuffer(W, H)
        try:
            for f in range(first, first + n):
                vp.render_kernel(buf.ptr, f, P)
            got = buf.download()
        finally:
            buf.free()
        assert got.tobytes() == want.tobytes(), ("render_kernel, look-ahead", la)
    vp.set_lookahead(0)
    total, part = vp.DeviceBuffer(W, H), vp.DeviceBuffer(W, H)
    try:
        for r in range(3):
            vp.set_shard(r, 3)
            part.reset()
            vp.render_frames(part.ptr, first, n, P)
            vp.accumulate(total.ptr, part.ptr, W * H)
        got = total.download()
    finally:
        vp.set_shard(0, 1)
        total.free(); part.free()
    assert got.tobytes() == want.tobytes(), "three shards"


# ---- 3. the certificate, oracle-free
@pytest.mark.parametrize("est_name", ["global", "decomposition"])
def test_coarse_pixel_classes_are_certified_by_the_fine_table(vp, est_name):
    W, H, s = 160, 120, 4
    est = vp.EST_GLOBAL if est_name == "global" else vp.EST_DECOMP
    _julia_scene(vp, est, vp.RNG_PHILOX7, brick=4 if est == vp.EST_DECOMP else 1)
    vp.set_subpixel(s)
    P = vp.make_param(W, H)
    general, light, miss = vp.pixel_lists(P)
    cls = vp.pixel_table(sub.fine_of(P, s))[..., 5].astype(np.int64)   # the table of the image the Param names: the fine one
    assert cls.shape == (s * H, s * W) and set(np.unique(cls)) <= {0, 1, 2}
    block = cls.reshape(H, s, W, s).transpose(0, 2, 1, 3).reshape(H, W, s * s)
    listed = np.full((H, W), -1)
    for k, lst in enumerate((general, light, miss)):
        y, x = (lst >> 16).astype(np.int64), (lst & 0xffff).astype(np.int64)
        assert (listed[y, x] == -1).all()
        listed[y, x] = k
    assert (listed >= 0).all() and len(general) + len(light) + len(miss) == W * H
    assert len(general) and len(light) and len(miss)   # (this view has all three)
    not_general = listed != 0
    assert not (block[not_general] == 0).any()          # no general fine pixel under a pixel that is not listed as general
    assert (block[listed == 2] == 2).all()              # box-missing: all of its fine pixels miss the box
    assert (block[listed == 1] != 0).all()
    # and nothing is over-classified for no reason: a pixel listed as general has a general fine pixel or mixes the other two
    g = block[listed == 0]
    assert ((g == 0).any(axis=1) | ((g == 1).any(axis=1) & (g == 2).any(axis=1))).all()


# ---- 4. the state machine
def test_factor_changes_camera_moves_and_batches_in_flight(vp):
    from volpath import host, scene as vscene
    W, H, n = 200, 150, 8
    P0, info = vscene.setup("c1", rng_mode=vp.RNG_PHILOX7, key=(3, 4), last_frame=64)
    P = vp.make_param(W, H)
    vp.set_lookahead(0)
    # S = 4
    vp.set_subpixel(4)
    got4 = _render(vp, P, [(0, n)])
    assert got4.tobytes() == sub.library_expectation(vp, P, 4, 0, n).tobytes()
    # back to 1: what a context that never heard of the mode renders
    vp.set_subpixel(1)
    got1 = _render(vp, P, [(0, n)])
    ctx = vp.Context(0)
    with ctx:
        assert vp.get_subpixel() == 1
        vscene.setup("c1", rng_mode=vp.RNG_PHILOX7, key=(3, 4), last_frame=64)
        vp.set_lookahead(0)
        fresh = _render(vp, P, [(0, n)])
    ctx.destroy()
    assert got1.tobytes() == fresh.tobytes()
    assert got1.tobytes() != got4.tobytes()
    # a camera move, then S = 2
    cam = tuple(float(v) for v in host.camera_matrix((3.9 * np.cos(0.7), -0.78, 3.9 * np.sin(0.7)), (-np.cos(0.7), 0.2, -np.sin(0.7)), (0.0, 1.0, 0.0)))
    vp.set_camera(cam)
    vp.set_subpixel(2)
    got2 = _render(vp, P, [(0, n)])
    assert got2.tobytes() == sub.library_expectation(vp, P, 2, 0, n).tobytes()
    # vp_set_subpixel while look-ahead batches are in flight: the batch behind the one being served is told to stop, the frames that
    # were handed out are whole, and nothing staged under the old factor is served under the new one
    vp.set_lookahead(vp.LOOKAHEAD_DEFAULT)
    vp.synchronize()
    l0, c0 = vp.lookahead_stats()
    a, b = vp.DeviceBuffer(W, H), vp.DeviceBuffer(W, H)
    try:
        for f in range(3):
            vp.render_kernel(a.ptr, f, P)          # frame 0 alone, then a batch from frame 1 with its successor queued behind it
        vp.set_subpixel(4)
        for f in range(3, 6):
            vp.render_kernel(a.ptr, f, P)          # the run goes on under the new factor
        for f in range(4):
            vp.render_kernel(b.ptr, f, P)
        got_a, got_b = a.download(), b.download()
    finally:
        a.free(); b.free()
    l1, c1 = vp.lookahead_stats()
    assert l1 - l0 >= 2 and c1 - c0 >= 1, (l1 - l0, c1 - c0)
    vp.set_lookahead(0)
    # buffer a: three frames under S = 2, then frames 3..5 under S = 4, added one by one in that order
    want_a = sub.library_expectation(vp, P, 2, 0, 3)
    vp.set_subpixel(1)
    frame, fbuf = sub.library_fine_frames(vp, sub.fine_of(P, 4))
    try:
        for f in range(3, 6):
            want_a = want_a + sub.gather(vp, frame(f), W, H, f, 4)
    finally:
        fbuf.free()
    assert got_a.tobytes() == want_a.tobytes()
    assert got_b.tobytes() == sub.library_expectation(vp, P, 4, 0, 4).tobytes()


# ---- 5. limits and refusals
def test_limits_and_refusals_leave_the_context_usable(vp):
    _julia_scene(vp, vp.EST_GLOBAL, vp.RNG_PHILOX7, n=32)
    vp.set_subpixel(8)
    wide = vp.make_param(8200, 8)             # 8 x 8200 = 65600 > 65536: the fine x does not fit x << 16 | y
    buf = vp.DeviceBuffer(8200, 8)
    try:
        assert vp.lib().vp_render_frames(buf.ptr, 0, 2, C.byref(wide)) == -3   # VP_E_ARG
        assert "sub-pixel" in vp.lib().vp_last_error().decode()
        assert vp.lib().vp_prepare(C.byref(wide)) == -3
        assert not buf.download().any()
    finally:
        buf.free()
    # the context is usable afterwards, at the largest factor
    P = vp.make_param(40, 24)
    got = _render(vp, P, [(2, 5)])
    assert got.tobytes() == sub.library_expectation(vp, P, 8, 2, 5).tobytes()
    # the one unsupported combination: work counters (a separately compiled kernel variant without the mode)
    vp.enable_counters(True)
    buf = vp.DeviceBuffer(40, 24)
    try:
        assert vp.lib().vp_render_frames(buf.ptr, 0, 2, C.byref(P)) == -2     # VP_E_STATE
        assert "counters" in vp.lib().vp_last_error().decode()
        assert not buf.download().any()
        vp.enable_counters(False)
        vp.render_frames(buf.ptr, 2, 5, P)
        assert buf.download().tobytes() == got.tobytes()
        # with S = 1 the counters work as before
        vp.set_subpixel(1)
        vp.enable_counters(True)
        vp.read_counters(reset=True)
        vp.render_frames(buf.ptr, 0, 2, P)
        assert vp.read_counters()["samples"] == 2 * 40 * 24
    finally:
        vp.enable_counters(False)
        buf.free()


# ---- the combinations beyond the shipped configuration work too (include/volpath.h): bounded estimator, MIS, scalar / multi-channel tracking
@pytest.mark.parametrize("what", ["bounded", "mis", "scalar", "multichannel"])
def test_other_builds_equal_the_oracle_gather(vp, oracle, what):
    W, H, N, s = 24, 16, 6, 4
    est = vp.EST_BOUNDED if what == "bounded" else vp.EST_DECOMP
    track = {"scalar": vp.TRACK_SCALAR, "multichannel": vp.TRACK_MULTI_CHANNEL}.get(what, vp.TRACK_SPECTRAL)
    mis = what == "mis"
    key = (11, 12)
    grid = scenes.blob_volume_u8(20)
    env = scenes.synthetic_env()
    osc = oracle.OracleScene(grid, env, scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER, estimator=est, rng_mode=vp.RNG_PHILOX, seed=key, env_mis=mis,
                             track_mode=track)
    want = sub.oracle_expectation(vp, osc, oracle.default_param(W, H, density=120.0), s, 0, N)
    vp.set_subpixel(1)
    vp.init_volume(grid, brick=1, linear=True)
    vp.init_envmap(env)
    vp.set_sun(scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER)
    vp.set_camera()
    vp.set_estimator(est)
    vp.set_rng(vp.RNG_PHILOX, key)
    vp.set_tracking(track)
    vp.set_envmap_sampling(vp.ENV_MIS if mis else vp.ENV_PASSIVE)
    try:
        vp.set_subpixel(s)
        P = vp.make_param(W, H, density=120.0)
        got = _render(vp, P, [(0, N)])
        assert np.array_equal(got, want, equal_nan=True), float(np.nanmax(np.abs(got - want)))
        got = _render(vp, P, [(f, 1) for f in range(N)])
        assert np.array_equal(got, want, equal_nan=True)
    finally:
        vp.set_tracking(0)
        vp.set_envmap_sampling(vp.ENV_PASSIVE)
