"""GPU parity: the HIP path, called through the C ABI, against the CPU oracle on identical seeds.

Bar: BIT-EXACT float4 accumulators (both sides evaluate the same binary32 operation sequences;
see DESIGN.md "Arithmetic contract").  tolerance = 0.
"""
import numpy as np
import pytest

import scenes

pytestmark = pytest.mark.gpu

W, H = 64, 48


def _setup(vp, oracle, grid, est, rng_mode, brick, P_kw=None, preset=None, linear=True, key=(0, 0)):
    env = scenes.synthetic_env()
    osc = oracle.OracleScene(grid, env, scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER, brick=brick,
                             linear=linear, estimator=est, rng_mode=rng_mode, seed=key)
    oP = oracle.default_param(W, H, **(P_kw or {}))
    vP = vp.make_param(W, H, **(P_kw or {}))
    if preset:
        oracle.mat(oP, *preset)
        vp.mat(vP, *preset)
        assert list(oP.sigma_t) == [vP.sigma_t.x, vP.sigma_t.y, vP.sigma_t.z]
        assert list(oP.albedo) == [vP.albedo.x, vP.albedo.y, vP.albedo.z]
    vp.init_volume(grid, brick=brick, linear=linear)
    vp.init_envmap(env)
    vp.set_sun(scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER)
    vp.set_camera()
    vp.set_estimator(est)
    vp.set_rng(rng_mode, key)
    vp.set_shard(0, 1)
    return osc, oP, vP


def _oracle_frames(osc, oP, frames):
    acc = None
    tot = None
    for f in frames:
        acc, c = osc.render_frame(oP, f, acc)
        d = c.as_dict()
        tot = d if tot is None else {k: tot[k] + d[k] for k in d}
    return acc, tot


@pytest.mark.parametrize("est", [1, 0, 2])
@pytest.mark.parametrize("rng_mode", [0, 1, 2])
def test_julia32_frames_bit_exact(vp, oracle, est, rng_mode):
    grid = oracle.julia(32)
    osc, oP, vP = _setup(vp, oracle, grid, est, rng_mode, brick=1, key=(123, 456))
    osc.precompute_opacity()
    vp.precompute_opacity(scenes.DEFAULT_SUN_DIR)
    # opacity table itself must agree bit for bit
    assert np.array_equal(vp.opacity_table((32, 32, 32)), osc.opacity)
    frames = list(range(0, 14))
    ref, cnt = _oracle_frames(osc, oP, frames)
    buf = vp.DeviceBuffer(W, H)
    # (a) the reference's call pattern: one render_kernel per frame
    for f in frames:
        vp.render_kernel(buf.ptr, f, vP)
    got = buf.download()
    assert np.array_equal(got, ref), f"max abs diff {np.abs(got - ref).max()}"
    # (b) the batched extension gives the same bits
    buf.reset()
    vp.enable_counters(True)
    vp.read_counters(reset=True)
    vp.render_frames(buf.ptr, 0, len(frames), vP)
    got2 = buf.download()
    c = vp.read_counters()
    vp.enable_counters(False)
    assert np.array_equal(got2, ref)
    for k in ("samples", "density_lookups", "bound_lookups", "opacity_lookups", "env_lookups", "scatters"):
        assert c[k] == cnt[k], (k, c[k], cnt[k])
    buf.free()


@pytest.mark.parametrize("est,brick,density", [(0, 1, 800.0), (0, 1, 209.0), (1, 1, 800.0), (1, 8, 800.0), (1, 8, 209.0)])
@pytest.mark.parametrize("rng_mode", [0, 1, 2])
def test_approach_kernels_walk_the_estimators_steps(vp, oracle, est, brick, density, rng_mode, monkeypatch):
    """approach_k / approach_local_k walk the camera rays through their certified-empty stretch ahead of the integrator (staged
    launches; the hand-over carries the stream's state: a pair index, or sampler.h's two words).  A counting launch makes those steps in the integrator itself unless VP_COUNT_APPROACH is set; with
    it the walk's steps and segments are tallied by the approach kernels: image and work counters == oracle either way, and
    the integrator is left with fewer density lookups of its own than the estimator makes.  Density 209: a majorant whose null
    collision in empty space is one ulp off neutral -- the global-majorant integrator then looks the walked throughput up by the
    number of steps, the decomposition walk stops at the first segment whose majorant is not neutral."""
    grid = oracle.julia(64)
    osc, oP, vP = _setup(vp, oracle, grid, est, rng_mode, brick=brick, key=(31, 7), P_kw=dict(density=density))
    if est == 1:
        osc.precompute_opacity()
        vp.precompute_opacity(scenes.DEFAULT_SUN_DIR)
    frames = list(range(7, 13))
    ref, cnt = _oracle_frames(osc, oP, frames)
    buf = vp.DeviceBuffer(W, H)
    # a plain staged launch uses the walk: mode 2 where the global-majorant medium's null collision is not neutral (density 209)
    vp.render_frames(buf.ptr, frames[0], len(frames), vP)
    assert np.array_equal(buf.download(), ref)
    assert vp.last_approach_mode() == (2 if (est == 0 and density == 209.0) else 1)
    for walk in (False, True):
        if walk:
            monkeypatch.setenv("VP_COUNT_APPROACH", "1")
        buf.reset()
        vp.enable_counters(True)
        vp.read_counters(reset=True)
        vp.render_frames(buf.ptr, frames[0], len(frames), vP)
        got = buf.download()
        c = vp.read_counters()
        vp.enable_counters(False)
        assert np.array_equal(got, ref), (walk, float(np.abs(got - ref).max()))
        for k in ("samples", "density_lookups", "bound_lookups", "opacity_lookups", "env_lookups", "scatters"):
            assert c[k] == cnt[k], (walk, k, c[k], cnt[k])
        assert (vp.last_approach_mode() != 0) == walk
    buf.free()


@pytest.mark.parametrize("brick,density", [(1, 800.0), (8, 800.0), (8, 209.0)])
@pytest.mark.parametrize("rng_mode", [0, 2])
def test_approach_walk_reads_the_segment_table_from_64_frames_on(vp, oracle, brick, density, rng_mode, monkeypatch):
    """Round 5: in launches of 64 frames and more the decomposition estimator's walk (a wave = one pixel in 64 frames) reads the
    restart segments of its pixel's camera ray from a per-view table (approach_segments_k -> approach_local_tab_k) instead of
    setting each one up per sample.  70 frames (a full block of 64 and a ragged one), across the frame-11 switch: image == oracle,
    the work counters with the walk tallied == oracle, the same with the walk cut short (VP_APPROACH_STEPS: the table's records
    beyond the cut are not walked) and with the table switched off (a context of its own: knobs are read at creation)."""
    grid = oracle.julia(64)
    osc, oP, vP = _setup(vp, oracle, grid, 1, rng_mode, brick=brick, key=(5, 77), P_kw=dict(density=density))
    osc.precompute_opacity()
    vp.precompute_opacity(scenes.DEFAULT_SUN_DIR)
    frames = list(range(3, 73))
    ref, cnt = _oracle_frames(osc, oP, frames)
    buf = vp.DeviceBuffer(W, H)
    vp.render_frames(buf.ptr, frames[0], len(frames), vP)
    assert np.array_equal(buf.download(), ref)
    assert vp.last_approach_mode() == 1 and vp.last_approach_table() == 1
    vp.render_frames(buf.ptr, frames[0], 6, vP)          # a short launch walks without the table
    assert vp.last_approach_mode() == 1 and vp.last_approach_table() == 0
    monkeypatch.setenv("VP_COUNT_APPROACH", "1")
    buf.reset()
    vp.enable_counters(True)
    vp.read_counters(reset=True)
    vp.render_frames(buf.ptr, frames[0], len(frames), vP)
    got = buf.download()
    c = vp.read_counters()
    vp.enable_counters(False)
    assert np.array_equal(got, ref)
    assert vp.last_approach_table() == 1
    for k in ("samples", "density_lookups", "bound_lookups", "opacity_lookups", "env_lookups", "scatters"):
        assert c[k] == cnt[k], (k, c[k], cnt[k])
    buf.free()
    monkeypatch.delenv("VP_COUNT_APPROACH")
    for env_set, table in ((dict(VP_APPROACH_STEPS="3"), 1), (dict(VP_NO_APPROACH_TABLE="1"), 0), (dict(VP_APPROACH_FRAMES_LOG2="5"), 0)):
        for k, v in env_set.items():
            monkeypatch.setenv(k, v)
        ctx = vp.Context(0)
        for k in env_set:
            monkeypatch.delenv(k)
        try:
            with ctx:
                _setup(vp, oracle, grid, 1, rng_mode, brick=brick, key=(5, 77), P_kw=dict(density=density))
                vp.precompute_opacity(scenes.DEFAULT_SUN_DIR)
                b2 = vp.DeviceBuffer(W, H)
                vp.render_frames(b2.ptr, frames[0], len(frames), vP)
                assert np.array_equal(b2.download(), ref), env_set
                assert vp.last_approach_table() == table, env_set
                b2.free()
        finally:
            ctx.destroy()


@pytest.mark.parametrize("brick", [1, 8])
def test_julia64_chromatic_bricks(vp, oracle, brick):
    grid = oracle.julia(64)
    osc, oP, vP = _setup(vp, oracle, grid, 1, 0, brick=brick, preset=scenes.PRESET1)
    tab, b, r = vp.bound_table()
    assert b == brick and r == osc.radius
    assert np.array_equal(tab, osc.bounds)
    ref, _ = _oracle_frames(osc, oP, range(4))
    buf = vp.DeviceBuffer(W, H)
    vp.render_frames(buf.ptr, 0, 4, vP)
    assert np.array_equal(buf.download(), ref)
    buf.free()


@pytest.mark.parametrize("density", [800.0, 209.0])
@pytest.mark.parametrize("rng_mode", [0, 1, 2])
def test_global_majorant_chromatic_light_and_general_pixels(vp, oracle, rng_mode, density):
    """Global-majorant estimator on a chromatic medium (the null-collision weights are not exactly 1, so the throughput of a
    path depends on how many steps it took): pixels whose camera ray meets only empty cells run the light kernel, the others
    the general one, side by side.  Image and work counters == oracle for the sequential sampler.h stream (whose unused
    collision variate must still be consumed) and both counter-based ones; the pixel table holds all three classes.
    Density 209: a majorant for which the weight of a null collision in EMPTY space is one ulp below 1 (at 800 it is exactly 1),
    so the light kernel's throughput table (thr_table_k) is not a row of ones."""
    grid = oracle.julia(64)
    osc, oP, vP = _setup(vp, oracle, grid, 0, rng_mode, brick=1, preset=scenes.PRESET1, key=(5, 77), P_kw=dict(density=density))
    assert (vp.null_collision_table(vP, 64)[-1] != 1.0) == (density == 209.0)
    t = vp.pixel_table(vP)
    classes = np.bincount(t[..., 5].astype(int).ravel(), minlength=3)
    assert classes.min() > 50, classes                      # general, certified-empty and box-missing pixels all occur
    ref, cnt = _oracle_frames(osc, oP, range(5))
    buf = vp.DeviceBuffer(W, H)
    vp.enable_counters(True)
    vp.read_counters(reset=True)
    vp.render_frames(buf.ptr, 0, 5, vP)
    got = buf.download()
    c = vp.read_counters()
    vp.enable_counters(False)
    assert np.array_equal(got, ref), float(np.abs(got - ref).max())
    for k in ("samples", "density_lookups", "env_lookups", "scatters"):
        assert c[k] == cnt[k], (k, c[k], cnt[k])
    assert 0 < c["density_loads"] < 0.6 * c["density_lookups"]     # most fetches are certified away
    # frame by frame through the reference's entry point (direct accumulation, both kernels into one buffer)
    buf.reset()
    for f in range(5):
        vp.render_kernel(buf.ptr, f, vP)
    assert np.array_equal(buf.download(), ref)
    buf.free()


@pytest.mark.parametrize("quantized", [True, False])
@pytest.mark.parametrize("linear", [True, False])
def test_blob_volume_filter_modes(vp, oracle, quantized, linear):
    grid = scenes.blob_volume_u8() if quantized else scenes.blob_volume_f32()
    osc, oP, vP = _setup(vp, oracle, grid, 1, 0, brick=1, linear=linear, P_kw=dict(density=60.0, g=0.3))
    ref, _ = _oracle_frames(osc, oP, range(3))
    buf = vp.DeviceBuffer(W, H)
    vp.render_frames(buf.ptr, 0, 3, vP)
    assert np.array_equal(buf.download(), ref)
    buf.free()


def test_math_and_rng_bits(vp, oracle):
    rng = np.random.default_rng(5)
    u = rng.random(200000).astype(np.float32)
    cases = {0: u, 1: (-80 * u).astype(np.float32), 2: (u * 6.2831855).astype(np.float32),
             3: (u * 6.2831855).astype(np.float32), 4: (u * 2 - 1).astype(np.float32),
             5: np.tan((u - 0.5) * 3.1).astype(np.float32), 6: u}
    for which, x in cases.items():
        assert np.array_equal(vp.test_math(which, x), oracle.math_array(which, x)), which
    assert vp.test_math(0, np.zeros(1, np.float32))[0] == -np.inf
    # the edges of the helpers' domains (test_helpers_gpu.py) and the codes of rcp_, sqrt_, rsqrt_ and sincos_turns_: the exact
    # helpers equal the oracle there too
    import test_helpers_gpu as TH
    xa, xc, xt = TH._exact_only_inputs()
    guards = np.array([-87.0, np.nextafter(np.float32(-87), np.float32(-100)), 88.0, np.nextafter(np.float32(88), np.float32(100)),
                       0.0, -0.0, -np.inf, np.inf], np.float32)
    xr = TH.normal_inputs(-125.0, 125.0)
    xr[::2] = -xr[::2]
    den = np.array([3.0e-39, 5.0e-39, 1.0e-38, 1.1e-38, 0.0], np.float32)
    edge = {0: [TH.log_inputs(), np.array([0.0, -0.0], np.float32)], 1: [TH.exp_inputs(), guards], 2: [xa], 3: [xa],
            4: [xc, np.array([1.5, -1.5, 2.0, -2.0], np.float32)], 5: [xt, np.array([np.inf, -np.inf, np.nan, 1e-40, -1e-40], np.float32)],
            6: [TH.normal_inputs(-126.0, 84.0)], 7: [xr, den], 8: [TH.normal_inputs(seed=15), den], 9: [TH.normal_inputs(seed=15), den],
            10: [TH.turns_inputs()], 11: [TH.turns_inputs()]}
    for which, xs in edge.items():
        x = np.concatenate(xs)
        assert np.array_equal(vp.test_math(which, x), oracle.math_array(which, x), equal_nan=True), which
    for mode in (0, 1, 2):
        a = vp.test_rng(mode, 3, 5, 7, 64, key=(11, 22))
        b = oracle.rng_stream(mode, 3, 5, 7, 64, key=(11, 22))
        assert np.array_equal(a, b)


def test_shard_union_is_bit_identical(vp, oracle):
    """pixel-tile sharding: the per-rank accumulators add up (one non-zero + zeros) to the 1-GPU image."""
    grid = oracle.julia(32)
    osc, oP, vP = _setup(vp, oracle, grid, 1, 1, brick=1, key=(9, 9))
    ref, _ = _oracle_frames(osc, oP, range(3))
    total = np.zeros((H, W, 4), np.float32)
    buf = vp.DeviceBuffer(W, H)
    for rank in range(3):
        buf.reset()
        vp.set_shard(rank, 3)
        vp.render_frames(buf.ptr, 0, 3, vP)
        total += buf.download()
    vp.set_shard(0, 1)
    assert np.array_equal(total, ref)
    buf.free()


def test_against_committed_golden_vectors(vp, oracle):
    """The HIP path against tests/golden/oracle_renders.npz (no live oracle in the comparison)."""
    import os
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_renders.npz"))
    grid = vp.julia_volume(32)
    assert np.array_equal(grid, gold["julia32"])
    env = scenes.synthetic_env()
    for est, name in ((1, "decomp"), (0, "global"), (2, "bounded")):
        for rng, rname in ((0, "samplerh"), (1, "philox")):
            vp.init_volume(grid, brick=1, linear=True)
            vp.init_envmap(env)
            vp.set_sun(scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER)
            vp.set_camera()
            vp.set_estimator(est)
            vp.set_rng(rng, (123, 456))
            vp.precompute_opacity(scenes.DEFAULT_SUN_DIR)
            buf = vp.DeviceBuffer(W, H)
            vp.render_frames(buf.ptr, 0, 14, vp.make_param(W, H))
            assert np.array_equal(buf.download(), gold[f"{name}_{rname}_f0_13"]), (name, rname)
            buf.free()
    tab, _, _ = vp.bound_table()
    assert np.array_equal(tab, gold["bounds32_r1"])
    assert np.array_equal(vp.opacity_table((32, 32, 32)), gold["opacity32"])
    # the compiled-out builds
    kw = dict(density=150.0, g=0.6, albedo=(0.9, 0.8, 0.7), sigma_t=(1.0, 0.7, 0.45))
    try:
        for tag, track, envm in (("mis", 0, 1), ("scalar", 1, 0), ("multichannel", 2, 0)):
            vp.set_tracking(track)
            vp.set_envmap_sampling(envm)
            vp.init_envmap(env)
            vp.set_estimator(1)
            vp.set_rng(1, (123, 456))
            buf = vp.DeviceBuffer(W, H)
            vp.render_frames(buf.ptr, 8, 6, vp.make_param(W, H, **kw))
            assert np.array_equal(buf.download(), gold[f"decomp_philox_{tag}_f8_13"]), tag
            buf.free()
    finally:
        vp.set_tracking(0)
        vp.set_envmap_sampling(0)


def test_scale_and_gamma_kernels(vp, oracle):
    import ctypes as C
    rng = np.random.default_rng(0)
    src = rng.random((H, W, 4), dtype=np.float32) * 3
    a = vp.DeviceBuffer(W, H)
    b = vp.DeviceBuffer(W, H)
    a.upload(src)
    vp.scale(b.ptr, a.ptr, W * H, 0.125)
    assert np.array_equal(b.download(), src * np.float32(0.125))
    vp.gamma_correct(b.ptr, a.ptr, W * H, 0.5, 2.2)
    ref = np.empty_like(src)
    oracle.lib().vpo_gamma_correct(ref.ctypes.data_as(C.c_void_p), src.ctypes.data_as(C.c_void_p), W * H, 0.5, 2.2)
    assert np.array_equal(b.download(), ref)
    vp.scale(a.ptr, a.ptr, W * H, 2.0)  # in place, as host.cpp:503 does
    assert np.array_equal(a.download(), src * np.float32(2.0))
    a.free()
    b.free()


def test_full_size_properties(vp):
    """BASELINE size (Julia 256^3, 800x600): size-independent properties instead of an oracle run."""
    from volpath import scene as vscene
    P, info = vscene.setup("c3", rng_mode=vp.RNG_PHILOX, last_frame=0)
    assert abs(info["occupancy"] - 0.0265) < 2e-4
    a = vp.DeviceBuffer(800, 600)
    b = vp.DeviceBuffer(800, 600)
    vp.render_frames(a.ptr, 0, 6, P)                    # batched
    for f in range(6):
        vp.render_kernel(b.ptr, f, P)                   # frame by frame
    ia, ib = a.download(), b.download()
    assert np.array_equal(ia, ib)                       # batching never changes a bit
    assert np.isfinite(ia).all() and (ia >= 0).all()
    heat = ia[..., 3] / 6
    assert abs((heat == 0).mean() - 0.88) < 0.02        # SURVEY section 6 probe
    # sharded halves add up to the whole, bit for bit
    tot = np.zeros_like(ia)
    for r in range(2):
        a.reset()
        vp.set_shard(r, 2)
        vp.render_frames(a.ptr, 0, 6, P)
        tot += a.download()
    vp.set_shard(0, 1)
    assert np.array_equal(tot, ia)
    a.free()
    b.free()


def test_full_size_estimators_and_builds_converge_to_one_image(vp):
    """BASELINE size, beyond the oracle's reach: the three kernels, and the MIS / scalar / multi-channel builds of the live
    one, are estimators of the SAME image.  192 spp each on Julia 256^3 at 800x600; compared on 40x40-pixel block means
    (1 % of the image mean + 4 standard errors of the pair) and on the whole-image mean.  The live kernel and its builds
    agree to 0.2 %; so do the two kernels without the optical-depth table; between the groups stands the bias of that
    table (quirk Q5: deep scatters after frame 10 use a dt = 0.001 march instead of a tracked shadow ray), 0.3-0.7 %.
    The STREAMS as well: the counter-based streams changed the random process in oracle and kernel together (shadow rays
    on sub-streams, the phase function sampled before the shadow ray, sun rays ended where only empty cells are left), so bit-equality
    with the oracle no longer ties them to the reference's order of draws -- sampler.h mode does.  The Philox2x32-10 and -7 images of
    the global-majorant and the live kernel must be the sampler.h images within the same Monte-Carlo bounds."""
    from volpath import scene as vscene
    frames = 192
    images = {}
    try:
        for name, est, track, envm, rng in (("decomp", 1, 0, 0, vp.RNG_PHILOX), ("global", 0, 0, 0, vp.RNG_PHILOX), ("bounded", 2, 0, 0, vp.RNG_PHILOX),
                                            ("decomp_mis", 1, 0, 1, vp.RNG_PHILOX), ("decomp_scalar", 1, 1, 0, vp.RNG_PHILOX),
                                            ("decomp_multichannel", 1, 2, 0, vp.RNG_PHILOX),
                                            ("decomp_samplerh", 1, 0, 0, vp.RNG_SAMPLERH), ("global_samplerh", 0, 0, 0, vp.RNG_SAMPLERH),
                                            ("decomp_philox7", 1, 0, 0, vp.RNG_PHILOX7), ("global_philox7", 0, 0, 0, vp.RNG_PHILOX7)):
            vp.set_tracking(track)
            vp.set_envmap_sampling(envm)
            P, info = vscene.setup("c3ref", rng_mode=rng, key=(11, est * 7 + track * 3 + envm), last_frame=frames)
            vp.set_estimator(est)
            buf = vp.DeviceBuffer(800, 600)
            vp.render_frames(buf.ptr, 0, frames, P)
            images[name] = buf.download()[..., :3].astype(np.float64) / frames
            buf.free()
    finally:
        vp.set_tracking(0)
        vp.set_envmap_sampling(0)
    blocks = lambda im: im.reshape(15, 40, 20, 40, 3).mean(axis=(1, 3))
    spread = lambda im: im.reshape(15, 40, 20, 40, 3).std(axis=(1, 3)) / np.sqrt(1600.0)

    def same_image(a, b, rtol_mean, block_frac):
        ia, ib = images[a], images[b]
        assert np.isfinite(ia).all() and np.isfinite(ib).all()
        assert np.allclose(ia.mean(axis=(0, 1)), ib.mean(axis=(0, 1)), rtol=rtol_mean), (a, b, ia.mean(axis=(0, 1)), ib.mean(axis=(0, 1)))
        tol = block_frac * ib.mean() + 4.0 * np.sqrt(spread(ia) ** 2 + spread(ib) ** 2)
        bad = np.abs(blocks(ia) - blocks(ib)) > tol
        assert bad.mean() < 0.01, (a, b, bad.mean())

    for name in ("decomp_mis", "decomp_scalar", "decomp_multichannel"):
        same_image(name, "decomp", 2e-3, 0.01)
    same_image("bounded", "global", 2e-3, 0.01)
    same_image("global", "decomp", 1.2e-2, 0.03)   # across the Q5 approximation
    # the reference's own streams against the counter-based ones, estimator by estimator
    for est in ("decomp", "global"):
        same_image(est, est + "_samplerh", 2e-3, 0.01)
        same_image(est + "_philox7", est + "_samplerh", 2e-3, 0.01)


def test_cli_render_matches_oracle_ppm(vp, oracle, tmp_path):
    """volpath_render (C++ host: Hosek sky bake, camera, reference entry points, gamma, PPM writer) end to end."""
    import ctypes as C
    import os
    import subprocess
    from volpath import host
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "cuda-volpath_amd", "volpath_render")
    out = str(tmp_path / "cli.ppm")
    r = subprocess.run([exe, "--julia", "32", "--size", "64", "48", "--spp", "4", "--out", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    env, sun_dir, sun_power = host.bake_sunsky(0.5, 0.2)
    osc = oracle.OracleScene(oracle.julia(32), env, sun_dir, sun_power, inv_view=host.camera_matrix())
    acc, _ = _oracle_frames(osc, oracle.default_param(64, 48), range(4))
    disp = np.empty_like(acc)
    oracle.lib().vpo_gamma_correct(disp.ctypes.data_as(C.c_void_p), acc.ctypes.data_as(C.c_void_p), 64 * 48, 0.25, 2.2)
    expect = (np.minimum(disp[::-1, :, :3], 1.0) * np.float32(255)).astype(np.uint8)
    raw = open(out, "rb").read()
    head = b"P6\n64 48\n255\n"
    assert raw.startswith(head)
    got = np.frombuffer(raw[len(head):], np.uint8).reshape(48, 64, 3)
    assert np.array_equal(got, expect)


@pytest.mark.parametrize("quantized", [True, False])
@pytest.mark.parametrize("brick", [1, 4])
def test_gpu_bound_table_builder(vp, oracle, quantized, brick):
    """H1 on the GPU (separable max/min passes + brick merge) against the oracle's brute-force windows,
    on a ragged non-cubic volume."""
    rng = np.random.default_rng(11)
    nz, ny, nx = 9, 14, 120
    g = rng.random((nz, ny, nx), dtype=np.float32)
    g[rng.random(g.shape) < 0.6] = 0
    grid = (g * 255).astype(np.uint8) if quantized else g
    vp.init_volume(grid, brick=brick)
    tab, b, r = vp.bound_table(quantized)
    assert b == brick and r == oracle.bound_radius(nx) + (1 if brick > 1 else 0) and r >= 3
    assert np.array_equal(tab, oracle.bounds(grid, r, brick))


@pytest.mark.parametrize("case", ["ragged_image", "one_pixel", "tiny_volume", "isotropic_absorbing", "zero_density",
                                  "negative_g", "late_frames_philox", "off_centre_box", "global_chromatic",
                                  "global_chromatic_philox", "global_point_filter", "bounded_chromatic_philox",
                                  "bounded_segment_cap", "decomp_scatter_cap"])
def test_edge_cases_bit_exact(vp, oracle, case):
    global W, H
    W0, H0 = W, H
    try:
        grid, kw, frames, est, rng, box, env = oracle.julia(32), {}, range(3), 1, 0, None, scenes.synthetic_env()
        preset, linear = None, True
        if case == "ragged_image":
            W, H = 70, 45           # partial 8x8 tiles on both edges
        elif case == "one_pixel":
            W, H = 1, 1
        elif case == "tiny_volume":
            grid = np.array([[[0, 255], [128, 7], [3, 90]]], np.uint8)  # nz=1, ny=3, nx=2
            kw = dict(density=5.0)
        elif case == "isotropic_absorbing":
            kw = dict(g=0.0, albedo=(0.5, 0.7, 0.9), sigma_t=(1.0, 0.8, 0.6), density=300.0)
        elif case == "zero_density":
            kw = dict(density=0.0)
        elif case == "negative_g":
            kw = dict(g=-0.4)
        elif case == "late_frames_philox":
            frames, rng, est = range(100000, 100003), 1, 0
        elif case in ("global_chromatic", "global_chromatic_philox"):
            est, rng = 0, (1 if case.endswith("philox") else 0)
            kw = dict(g=0.5, albedo=(0.95, 0.8, 0.6), sigma_t=(1.0, 0.7, 0.45), density=120.0)
            frames = range(5)
        elif case == "global_point_filter":
            est, linear = 0, False
        elif case == "bounded_chromatic_philox":
            est, rng = 2, 1
            kw = dict(g=0.5, albedo=(0.95, 0.8, 0.6), sigma_t=(1.0, 0.7, 0.45), density=120.0)
            frames = range(11, 14)  # past frame 10: __d_render_bounded still never reads the opacity volume
        elif case in ("bounded_segment_cap", "decomp_scatter_cap"):
            # a solid, dense, non-absorbing block: paths run into max_depth = 800 (kernel.cu:34)
            est = 2 if case.startswith("bounded") else 1
            grid = np.full((16, 16, 16), 255, np.uint8)
            kw = dict(density=4000.0, g=0.0)
            W, H = 24, 16
            frames = range(1)
        elif case == "off_centre_box":
            box = ((-0.3, -1.1, 0.2), (1.2, 0.4, 1.9))
            env = np.full((1, 1, 4), 0.25, np.float32)   # 1x1 environment
        osc = oracle.OracleScene(grid, env, scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER, box=box, estimator=est,
                                 rng_mode=rng, seed=(7, 7), linear=linear)
        oP = oracle.default_param(W, H, **kw)
        vP = vp.make_param(W, H, **kw)
        vp.init_volume(grid, box=box, brick=1, linear=linear)
        vp.init_envmap(env)
        vp.set_sun(scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER)
        vp.set_camera()
        vp.set_estimator(est)
        vp.set_rng(rng, (7, 7))
        vp.set_shard(0, 1)
        ref, _ = _oracle_frames(osc, oP, frames)
        buf = vp.DeviceBuffer(W, H)
        vp.render_frames(buf.ptr, frames[0], len(frames), vP)
        got = buf.download()
        buf.free()
        assert np.array_equal(got, ref, equal_nan=True), f"{case}: max abs diff {np.nanmax(np.abs(got - ref))}"
        if case == "bounded_segment_cap":
            assert ref[..., 3].max() == np.float32(0.8)   # heat = 800 * 0.001 for a capped sample
        if case == "decomp_scatter_cap":
            assert ref[..., 3].max() == 800.0
    finally:
        W, H = W0, H0


@pytest.mark.parametrize("est", [1, 0, 2])
@pytest.mark.parametrize("rng_mode", [0, 1])
def test_active_envmap_mis_bit_exact(vp, oracle, est, rng_mode):
    """The reference's !PASSIVE_ENVMAP build: CDF tables (kernel.cu:1144-1210) and one-sample MIS (:2220-2297)."""
    grid = oracle.julia(32)
    env = scenes.synthetic_env()
    env[3, 5, :3] = 0.0   # a black texel inside a row: a zero-probability entry of the row CDF
    osc = oracle.OracleScene(grid, env, scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER, estimator=est, rng_mode=rng_mode,
                             seed=(9, 4), env_mis=True)
    kw = dict(density=150.0, g=0.6) if est != 1 else {}
    preset = scenes.PRESET1 if est == 2 else None
    oP, vP = oracle.default_param(W, H, **kw), vp.make_param(W, H, **kw)
    if preset:
        oracle.mat(oP, *preset)
        vp.mat(vP, *preset)
    try:
        vp.set_envmap_sampling(vp.ENV_MIS)
        vp.init_volume(grid, brick=1)
        vp.init_envmap(env)
        cdf_y, cdf_x, norm = vp.env_tables(env.shape[1], env.shape[0])
        assert np.array_equal(cdf_y, osc.cdf_y) and np.array_equal(cdf_x, osc.cdf_x)
        assert np.float32(norm) == np.float32(osc.pdfnorm_alt)
        vp.set_sun(scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER)
        vp.set_camera()
        vp.set_estimator(est)
        vp.set_rng(rng_mode, (9, 4))
        vp.set_shard(0, 1)
        osc.precompute_opacity()
        vp.precompute_opacity(scenes.DEFAULT_SUN_DIR)
        frames = range(8, 14)     # across the frame > 10 opacity switch of the live kernel
        ref, cnt = _oracle_frames(osc, oP, frames)
        buf = vp.DeviceBuffer(W, H)
        vp.enable_counters(True)
        vp.read_counters(reset=True)
        vp.render_frames(buf.ptr, frames[0], len(frames), vP)
        got = buf.download()
        c = vp.read_counters()
        vp.enable_counters(False)
        buf.free()
        assert np.array_equal(got, ref), f"max abs diff {np.abs(got - ref).max()}"
        for k in ("density_lookups", "env_lookups", "scatters", "opacity_lookups"):
            assert c[k] == cnt[k], (k, c[k], cnt[k])
        assert cnt["env_lookups"] > cnt["samples"]          # more than the one background lookup per path
    finally:
        vp.set_envmap_sampling(vp.ENV_PASSIVE)


@pytest.mark.parametrize("est,frame", [(0, 6636), (0, 9355), (1, 10110), (2, 10110)])
def test_mis_zero_pdf_continue_quirk(vp, oracle, est, frame):
    """kernel.cu:2266 / :1539 / :1900: an environment sample of zero pdf `continue`s the path loop, so the path goes on
    from the OLD origin in the OLD direction.  It takes a random number of exactly 0 on a black first column; the
    (estimator, frame) pairs were found by scanning frames with the oracle's hit counter (Philox key (9, 4))."""
    grid = oracle.julia(32)
    env = scenes.synthetic_env()
    env[:, 0, :3] = 0.0
    osc = oracle.OracleScene(grid, env, scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER, estimator=est, rng_mode=1,
                             seed=(9, 4), env_mis=True)
    kw = dict(density=150.0, g=0.6)
    oP, vP = oracle.default_param(W, H, **kw), vp.make_param(W, H, **kw)
    osc.precompute_opacity()
    before = oracle.lib().vpo_debug_mis_zero_pdf()
    ref, _ = osc.render_frame(oP, frame)
    assert oracle.lib().vpo_debug_mis_zero_pdf() > before, "this frame no longer takes the zero-pdf branch"
    try:
        vp.set_envmap_sampling(vp.ENV_MIS)
        vp.init_volume(grid, brick=1)
        vp.init_envmap(env)
        vp.set_sun(scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER)
        vp.set_camera()
        vp.set_estimator(est)
        vp.set_rng(1, (9, 4))
        vp.set_shard(0, 1)
        vp.precompute_opacity(scenes.DEFAULT_SUN_DIR)
        buf = vp.DeviceBuffer(W, H)
        vp.render_frames(buf.ptr, frame, 1, vP)
        got = buf.download()
        buf.free()
        assert np.array_equal(got, ref), f"max abs diff {np.abs(got - ref).max()}"
    finally:
        vp.set_envmap_sampling(vp.ENV_PASSIVE)


@pytest.mark.parametrize("est", [1, 0, 2])
@pytest.mark.parametrize("track,rng_mode", [(1, 0), (2, 1), (2, 0), (1, 1)])
def test_scalar_tracking_builds_bit_exact(vp, oracle, est, track, rng_mode):
    """The reference's compiled-out SPECTRAL_TRACKING 0 (track 1) and MULTI_CHANNEL 1 (track 2) builds of all three kernels."""
    grid = oracle.julia(32)
    env = scenes.synthetic_env()
    osc = oracle.OracleScene(grid, env, scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER, estimator=est, rng_mode=rng_mode,
                             seed=(2, 8), track_mode=track)
    kw = dict(density=200.0, g=0.5, albedo=(0.9, 0.8, 0.7), sigma_t=(1.0, 0.7, 0.45))
    oP, vP = oracle.default_param(W, H, **kw), vp.make_param(W, H, **kw)
    try:
        vp.set_tracking(track)
        vp.init_volume(grid, brick=1)
        vp.init_envmap(env)
        vp.set_sun(scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER)
        vp.set_camera()
        vp.set_estimator(est)
        vp.set_rng(rng_mode, (2, 8))
        vp.set_shard(0, 1)
        osc.precompute_opacity()
        vp.precompute_opacity(scenes.DEFAULT_SUN_DIR)
        frames = range(8, 14)     # across the frame > 10 opacity switch of the live kernel
        ref, _ = _oracle_frames(osc, oP, frames)
        buf = vp.DeviceBuffer(W, H)
        vp.render_frames(buf.ptr, frames[0], len(frames), vP)
        got = buf.download()
        buf.free()
        assert np.array_equal(got, ref), f"max abs diff {np.abs(got - ref).max()}"
        if track == 2:
            assert ((got[..., :3] > 0).sum(-1) <= len(frames)).all()   # one channel per sample
    finally:
        vp.set_tracking(vp.TRACK_SPECTRAL)


def test_render_kernel_lookahead_is_invisible(vp, oracle):
    """render_kernel stages frames ahead when called for consecutive frames; every observable state of the accumulator
    must equal the one-launch-per-frame result: after each call, across state changes, frame jumps and buffer swaps."""
    grid = oracle.julia(32)
    osc, oP, vP = _setup(vp, oracle, grid, 1, 1, brick=1, key=(5, 6))
    osc.precompute_opacity()
    vp.precompute_opacity(scenes.DEFAULT_SUN_DIR)
    vp.set_lookahead(8)
    try:
        buf, buf2 = vp.DeviceBuffer(W, H), vp.DeviceBuffer(W, H)
        ref = np.zeros((H, W, 4), np.float32)
        # (a) 21 consecutive frames (frame 0 alone, then batches of 8, the depth set above -- [1..8], [9..16], [17..24] --, each queued when the one before it is entered)
        for f in range(21):
            vp.render_kernel(buf.ptr, f, vP)
            ref, _ = osc.render_frame(oP, f, ref)
            if f in (0, 1, 2, 6, 7, 14, 15, 20):
                assert np.array_equal(buf.download(), ref), f"after frame {f}"
        # (b) the camera moves while frames 21.. are staged: they must be dropped
        cam = np.array([[0, .3, .95, 3.7], [0, .95, -.3, -.9], [-1, 0, 0, .1]], np.float32)
        vp.set_camera(cam.ravel().tolist())
        osc2 = oracle.OracleScene(grid, scenes.synthetic_env(), scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER, brick=1,
                                  estimator=1, rng_mode=1, seed=(5, 6), inv_view=cam)
        osc2.precompute_opacity()
        for f in (21, 22, 23):
            vp.render_kernel(buf.ptr, f, vP)
            ref, _ = osc2.render_frame(oP, f, ref)
        assert np.array_equal(buf.download(), ref)
        # (c) a frame jump, a repeated frame, and a Param change inside a staged run
        ref2 = np.zeros((H, W, 4), np.float32)
        vP2 = vp.make_param(W, H, density=300.0)
        oP2 = oracle.default_param(W, H, density=300.0)
        for f, (vq, oq) in [(40, (vP, oP)), (41, (vP, oP)), (42, (vP, oP)), (42, (vP, oP)), (43, (vP2, oP2)), (44, (vP2, oP2)),
                            (45, (vP2, oP2)), (3, (vP2, oP2))]:
            vp.render_kernel(buf2.ptr, f, vq)
            ref2, _ = osc2.render_frame(oq, f, ref2)
        assert np.array_equal(buf2.download(), ref2)
        # (d) staged frames may go to a different accumulator than the one of the miss
        buf.reset(); buf2.reset()
        a = np.zeros((H, W, 4), np.float32); b = np.zeros((H, W, 4), np.float32)
        for f in range(50, 58):
            tgt, acc = (buf, "a") if f % 2 == 0 else (buf2, "b")
            vp.render_kernel(tgt.ptr, f, vP2)
            if acc == "a": a, _ = osc2.render_frame(oP2, f, a)
            else: b, _ = osc2.render_frame(oP2, f, b)
        assert np.array_equal(buf.download(), a) and np.array_equal(buf2.download(), b)
        buf.free(); buf2.free()
    finally:
        vp.set_lookahead(vp.LOOKAHEAD_DEFAULT)
        vp.set_camera()


def test_bad_arguments_are_rejected(vp):
    grid = vp.julia_volume(8)
    vp.init_volume(grid)
    vp.init_envmap(scenes.synthetic_env())
    vp.set_sun(scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER)
    vp.set_camera()
    vp.set_estimator(1)
    P = vp.make_param(16, 16)
    buf = vp.DeviceBuffer(16, 16)
    with pytest.raises(vp.VolpathError):
        vp.render_frames(buf.ptr, 0, 0, P)          # no frames
    with pytest.raises(vp.VolpathError):
        vp.render_frames(None, 0, 1, P)             # null accumulator
    with pytest.raises(vp.VolpathError):
        vp.render_frames(buf.ptr, 20, 1, P)         # frame > 10 without precompute_opacity (kernel.cu:2183)
    with pytest.raises(vp.VolpathError):
        vp.render_frames(buf.ptr, 0, 1, vp.make_param(70000, 4))   # sampler.h packs x<<16|y
    vp.precompute_opacity(scenes.DEFAULT_SUN_DIR)
    vp.render_frames(buf.ptr, 20, 1, P)
    assert np.isfinite(buf.download()).all()
    buf.free()


def test_lds_brick_table_with_opacity_frames(vp, oracle):
    """BASELINE config 3 in miniature: 8^3 bricks (LDS-staged table), frames across the frame-11 estimator
    switch (quirk Q5), Philox streams."""
    grid = oracle.julia(64)
    osc, oP, vP = _setup(vp, oracle, grid, 1, 1, brick=8, key=(3, 1))
    osc.precompute_opacity()
    vp.precompute_opacity(scenes.DEFAULT_SUN_DIR)
    ref, cnt = _oracle_frames(osc, oP, range(8, 14))
    assert cnt["opacity_lookups"] > 0
    buf = vp.DeviceBuffer(W, H)
    vp.render_frames(buf.ptr, 8, 6, vP)
    assert np.array_equal(buf.download(), ref)
    buf.free()


def test_multi_launch_batches_in_subprocess(oracle, tmp_path):
    """vp_render_frames splits long renders into several launches when the staging buffer is capped;
    the split must not change a bit (run in a child process so that VP_STAGE_MB is read at device init)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r"""
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import volpath as vp, scenes
vp.set_device(0)
grid = vp.julia_volume(32)
vp.init_volume(grid); vp.init_envmap(scenes.synthetic_env()); vp.set_sun(scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER)
vp.set_camera(); vp.set_estimator(0); vp.set_rng(1, (5, 6))
P = vp.make_param(64, 48); buf = vp.DeviceBuffer(64, 48)
vp.render_frames(buf.ptr, 0, 40, P)
n = vp.render_time_ms()[1]
np.save(%r, buf.download()); print("launches", n)
""" % (os.path.join(root, "cuda-volpath_amd"), os.path.join(root, "tests"), str(tmp_path / "out.npy"))
    outs = []
    for mb in ("1", "512"):   # 1 MiB of staging = 21 frames of 64x48 per launch -> two launches
        env = dict(os.environ, VP_STAGE_MB=mb)
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        outs.append((np.load(str(tmp_path / "out.npy")), int(r.stdout.split()[-1])))
    assert outs[0][1] > outs[1][1] == 1
    assert np.array_equal(outs[0][0], outs[1][0])


def test_bench_two_ranks_rehearsal_matches_one_rank(tmp_path):
    """bench.py's N>1 path end to end on this one-GPU box (both ranks on GPU 0, reduce over gloo), started AS TYPED --
    `python bench.py --gpus 2`, no external torchrun: bench.py starts its ranks as a child process before anything touches the
    GPU.  The 2-rank image of frames [0,8) must equal the 1-rank image bit for bit, the JSON line must be well formed, and
    --scaling both adds the fixed-job (strong) measurement to the weak line.  --full: the roofline, the per-camera set-up time and the
    complete record; --dump-outputs: the last timed step's accumulator, here (one step, no warm-up) the summed image itself."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    bench = os.path.join(root, "bench.py")
    one, two = str(tmp_path / "one.npy"), str(tmp_path / "two.npy")
    common = ["--steps", "1", "--warmup", "0", "--no-cpu-baseline", "--workload", "c1", "--full"]
    full1, full2 = str(tmp_path / "full1.json"), str(tmp_path / "full2.json")
    out1 = tmp_path / "out1"
    r1 = subprocess.run([sys.executable, bench, "--gpus", "1", "--spp", "8", "--dump-image", one, "--full-out", full1, "--call-pattern",
                         "--dump-outputs", str(out1)] + common, capture_output=True, text=True, cwd=root)
    assert r1.returncode == 0, r1.stdout + r1.stderr
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env["VP_BENCH_REHEARSAL"] = "1"
    r2 = subprocess.run([sys.executable, bench, "--gpus", "2", "--spp", "4", "--scaling", "both", "--dump-image", two, "--full-out", full2] + common,
                        capture_output=True, text=True, cwd=root, env=env)
    assert r2.returncode == 0, r2.stdout + r2.stderr
    # the driver's contract: the LAST line of stdout is one JSON object of at most 3 KB (round 4's 20 KB line was cut by the driver's
    # 8 KB tail and never parsed); everything else is in the --full-out file
    for r in (r1, r2):
        last = r.stdout.rstrip("\n").splitlines()[-1]
        assert last.startswith("{") and len(last) <= 3072, len(last)
    line1 = json.loads(r1.stdout.rstrip("\n").splitlines()[-1])
    line2 = json.loads(r2.stdout.rstrip("\n").splitlines()[-1])
    rec1, rec2 = json.load(open(full1)), json.load(open(full2))
    for line, rec, n in ((line1, rec1, 1), (line2, rec2, 2)):
        assert line["n_gpus"] == n and line["scaling"] == "weak" and line["unit"] == "Msamples/s" and line["value"] > 0
        assert line["config"]["spp_per_step"] == 8 and set(line["roofline"]) >= {"bound", "achieved", "peak", "frac", "traffic", "kernel", "launch_ms"}
        assert abs(line["value"] - rec["value"]) <= 1e-4 * rec["value"] and line["roofline"]["kernel"] == "vp::render_k"
        assert set(rec["per_class"]) >= {"general", "light", "misses_box"} and rec["per_camera_setup_ms"] > 0
    # the driver's contract (one JSON line) and what this repo adds to it
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert k in line1, k
    assert line1["higher_is_better"] is True and line1["vs_baseline"] is None and line1["config"]["workload"].startswith("julia128") and line1["dtype"] == "f32"
    assert line1["roofline"]["bound"] == "hbm" and line1["roofline"]["unit"] == "GB/s" and 0 < line1["roofline"]["frac"] < 1
    cp = rec1["reference_call_pattern"]     # (--call-pattern) the reference host's own loop: one render_kernel per frame, a synchronisation after each
    assert cp["frames"] == 1200 and cp["msamples_per_s"] > 0 and cp["orbit"]["msamples_per_s"] > 0 and cp["orbit"]["first_frame_after_a_move_ms_median"] > 0
    assert line1["call_pattern"]["msamples_per_s"] > 0 and "reference_call_pattern" not in rec2 and "call_pattern" not in line2
    assert line2["strong"]["scaling"] == "strong" and line2["strong"]["spp_per_step"] == 4 and line2["strong"]["value"] > 0
    assert len(line2["ranks"]["kernel_ms"]) == 2 and line2["ranks"]["collective_ranks"] == 2 and line2["ranks"]["backend"] == "gloo"
    assert np.array_equal(np.load(one), np.load(two))
    acc1 = np.load(str(out1 / "hdr_accumulator.npy"))
    assert acc1.dtype == np.float32 and acc1.shape == (300, 400, 4) and np.array_equal(acc1, np.load(one))


def test_bench_four_rank_rehearsal_is_bit_identical_and_its_line_short(tmp_path):
    """`bench.py --gpus N --scaling both` AS TYPED with as many ranks as this pool lets one card carry beside the
    test runner -- the process guard allows six processes on the GPU, this pytest process is one of them, and a run with six ranks was
    killed by it ("8 processes had the GPU open"): FOUR ranks.  (Eight shards of ONE process are
    test_cli_bin_ingest_matches_oracle_and_two_contexts_match_one's --gpus 8 and test_pixel_lists_are_the_stable_partition_of_the_tile_
    order's world = 8.)  All ranks on GPU 0, the reduce over gloo.  The tile split's image equals the one-rank image bit for bit, the
    final stdout line is one JSON object of at most 3 KB with the per-rank times, the balance, both ways of sharing the fixed job and
    the collective's rank count.  Plain runs (no --full); --dump-outputs writes the last timed step's accumulator of rank 0, here
    (one step, no warm-up) the summed image itself, on one rank and on four."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    bench = os.path.join(root, "bench.py")
    one, four = str(tmp_path / "one.npy"), str(tmp_path / "four.npy")
    common = ["--steps", "1", "--warmup", "0", "--no-cpu-baseline", "--workload", "c1"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r1 = subprocess.run([sys.executable, bench, "--gpus", "1", "--spp", "16", "--dump-image", one, "--full-out", str(tmp_path / "f1.json"),
                         "--dump-outputs", str(tmp_path / "o1")] + common, capture_output=True, text=True, cwd=root, env=env)
    assert r1.returncode == 0, r1.stdout + r1.stderr
    env["VP_BENCH_REHEARSAL"] = "1"
    r4 = subprocess.run([sys.executable, bench, "--gpus", "4", "--spp", "4", "--scaling", "both", "--dump-image", four,
                         "--full-out", str(tmp_path / "f4.json"), "--dump-outputs", str(tmp_path / "o4")] + common,
                        capture_output=True, text=True, cwd=root, env=env, timeout=900)
    assert r4.returncode == 0, r4.stdout + r4.stderr
    last = r4.stdout.rstrip("\n").splitlines()[-1]
    assert last.startswith("{") and len(last) <= 3072, len(last)
    line = json.loads(last)
    assert line["n_gpus"] == 4 and line["scaling"] == "weak" and line["config"]["spp_per_step"] == 16 and line["value"] > 0
    assert len(line["ranks"]["kernel_ms"]) == 4 and len(line["ranks"]["wall_s"]) == 4 and line["ranks"]["collective_ranks"] == 4
    assert line["ranks"]["balance_max_over_mean"] >= 1.0 and line["strong"]["spp_per_step"] == 4
    assert set(line["strong"]["by_split"]) == {"tiles", "frames"} and line["strong"]["split"] in ("tiles", "frames")
    assert np.array_equal(np.load(one), np.load(four))
    for d in ("o1", "o4"):
        assert np.array_equal(np.load(str(tmp_path / d / "hdr_accumulator.npy")), np.load(one))


def test_bench_frame_split_adds_partial_images_in_rank_order(vp, tmp_path):
    """bench.py --scaling strong --split frames (SURVEY section 8e's sample split: every rank renders ALL pixels in its contiguous
    share of the frames; the partial images are gathered and added in rank order on rank 0).  binary32 addition does not associate,
    so the result is DEFINED as ((p0 + p1) + ...): two ranks on this one GPU (rehearsal) must produce exactly the sum of the two
    partial images rendered here in one process -- and --split auto must report both ways of sharing the fixed job."""
    import json
    import os
    import subprocess
    import sys
    from volpath import scene as vscene
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    bench = os.path.join(root, "bench.py")
    two = str(tmp_path / "two.npy")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env["VP_BENCH_REHEARSAL"] = "1"
    common = ["--steps", "1", "--warmup", "0", "--no-cpu-baseline", "--workload", "c1", "--gpus", "2", "--spp", "8"]
    r = subprocess.run([sys.executable, bench, "--scaling", "strong", "--split", "frames", "--dump-image", two] + common,
                       capture_output=True, text=True, cwd=root, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["scaling"] == "strong" and "frame-ranges x2" in line["config"]["parallelism"] and line["config"]["spp_per_step"] == 8
    P, info = vscene.setup("c1", rng_mode=vp.RNG_PHILOX7, last_frame=8)
    parts = []
    for first in (0, 4):
        buf = vp.DeviceBuffer(P.width, P.height)
        vp.render_frames(buf.ptr, first, 4, P)
        parts.append(buf.download())
        buf.free()
    got = np.load(two)
    assert np.array_equal(got, parts[0] + parts[1])
    buf = vp.DeviceBuffer(P.width, P.height)
    vp.render_frames(buf.ptr, 0, 8, P)
    one = buf.download()
    buf.free()
    assert np.allclose(got, one, rtol=1e-5, atol=1e-6) and not np.array_equal(got, one)    # same estimate, not the one-rank bits
    r = subprocess.run([sys.executable, bench, "--scaling", "both", "--split", "auto"] + common, capture_output=True, text=True, cwd=root, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert set(line["strong"]["by_split"]) == {"tiles", "frames"} and line["strong"]["split"] in ("tiles", "frames")
    assert line["scaling"] == "weak" and len(line["ranks"]["kernel_ms"]) == 2
    vp.set_camera()


@pytest.mark.parametrize("quantized", [True, False])
@pytest.mark.parametrize("linear", [True, False])
def test_density_fetch_pointwise(vp, oracle, quantized, linear):
    """The tex3D restatement point by point (no integrator around it): random positions in and slightly outside an off-centre,
    non-cubic box, device fetch == oracle fetch bit for bit.  Float texels below the first texel centre of an axis are the case
    the randomised scenes of test_fuzz_gpu.py caught: both taps are texel 0 there, but a*(1-w) + a*w is not a in binary32."""
    import ctypes as C
    rs = np.random.default_rng(11)
    g = rs.random((9, 14, 11), dtype=np.float32)
    g[rs.random(g.shape) < 0.3] = 0
    grid = np.ascontiguousarray((g * 255).astype(np.uint8)) if quantized else g
    box = ((-0.7, -1.3, 0.1), (1.6, 0.2, 1.4))
    osc = oracle.OracleScene(grid, scenes.synthetic_env(), scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER, box=box, linear=linear)
    vp.init_volume(grid, box=box, brick=1, linear=linear)
    bmin, bmax = np.array(box[0]), np.array(box[1])
    pts = (bmin + (bmax - bmin) * rs.uniform(-0.08, 1.08, (6000, 3))).astype(np.float32)
    pts[:64] = (bmin + (bmax - bmin) * rs.integers(0, 2, (64, 3))).astype(np.float32)      # the corners themselves
    got = vp.test_sample_density(pts)
    L = oracle.lib()
    ref = np.array([L.vpo_sample_density(C.byref(osc.S), (C.c_float * 3)(*p)) for p in pts], np.float32)
    bad = np.flatnonzero(got != ref)
    assert len(bad) == 0, (len(bad), pts[bad[0]], got[bad[0]], ref[bad[0]])
