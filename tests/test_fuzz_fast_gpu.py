"""The fast arithmetic mode on seeded random scenes: the generator of test_fuzz_gpu.py (tests/scenes.py
random_case), with the draws the fast mode does not build mapped, after drawing, to ones it does: the bounded estimator to the global
majorant, the sampler.h stream to Philox2x32-10, MIS to the passive environment, scalar / multi-channel tracking to spectral.

Per seed:
  1. tolerance 0 inside the fast mode: one render_frames launch equals render_kernel frame by frame with the look-ahead on (its
     CANCEL instances, LDS form 1), the sum of the case's `world` shards, and the sum of one-frame launches -- which make no approach
     walk, so they check that the walks decide null-collision neutrality in the fast arithmetic.  Odd seeds render 64 frames and more
     (the decomposition estimator's walk then reads the per-view segment table) in a context that takes no volume for dense;
  2. box-missing and light pixels (pixel classes 1 and 2) are bit-identical to the exact mode; everything is finite and >= 0;
  3. paired agreement with the exact mode over 64 one-frame renders (the same streams: d = fast - exact per sample).
A coverage test checks that the seed set really reached the kernels and walks it is meant to reach, and a fixed scene pins the
decomposition walk's neutrality test, which the random scenes rarely reach."""
import os

import numpy as np
import pytest

import scenes

pytestmark = pytest.mark.gpu

SEEDS = int(os.environ.get("VP_FUZZ_FAST_SEEDS", "32"))
PAIRED_FRAMES = 64
COVERAGE = {}        # seed -> what check 1 ran (test_fast_fuzz_coverage)


def fast_case(seed, host):
    """scenes.random_case with every draw the fast mode does not build mapped to one it does (deterministically, after drawing)"""
    c = scenes.random_case(9000 + seed, host)
    rng = np.random.default_rng(31 + seed)
    if c["est"] == 2:
        c["est"] = 0
        c["brick"] = 1
    if c["rng_mode"] == 0:
        c["rng_mode"] = 1
    c["env_mis"], c["track"] = False, 0
    if seed % 8 == 6:
        # a binary uchar volume and the decomposition estimator: at most four (max, min) brick pairs, the compact LDS table (form 2)
        c["grid"] = np.ascontiguousarray((c["grid"] > 0).astype(np.uint8) * np.uint8(255))
        c["est"], c["brick"] = 1, int(rng.choice([2, 4, 8]))
    if seed & 1:
        c["first"], c["nframes"] = int(rng.choice([0, 3, 40])), int(rng.integers(64, 81))
    c["late"] = c["est"] == 1       # (the decomposition estimator past frame 10, here and in the paired renders: precompute_opacity)
    return c


def _camera_inside(c):
    g = c["grid"]
    nz, ny, nx = g.shape
    if c["box"] is None:
        bmin, bmax = np.array([-1.0, -ny / nx, -nz / nx]), np.array([1.0, ny / nx, nz / nx])
    else:
        bmin, bmax = np.array(c["box"][0]), np.array(c["box"][1])
    pos = np.asarray(c["cam"], np.float64)[[3, 7, 11]]
    return bool(((pos > bmin) & (pos < bmax)).all())


def _setup(vp, c):
    vp.init_volume(c["grid"], box=c["box"], brick=c["brick"], linear=c["linear"])
    vp.init_envmap(c["env"])
    vp.set_sun(c["sun_dir"], c["sun_power"])
    vp.set_camera(c["cam"])
    vp.set_estimator(c["est"])
    vp.set_rng(c["rng_mode"], c["key"])
    vp.set_tracking(0)
    vp.set_envmap_sampling(vp.ENV_PASSIVE)
    vp.set_shard(0, 1)
    if c["late"]:
        vp.precompute_opacity(c["sun_dir"])
    return vp.make_param(c["W"], c["H"], **c["kw"])


def _render(vp, P, first, n):
    buf = vp.DeviceBuffer(P.width, P.height)
    try:
        vp.render_frames(buf.ptr, first, n, P)
        return buf.download()
    finally:
        buf.free()


def _context(vp, seed, monkeypatch):
    if seed & 1:
        monkeypatch.setenv("VP_DENSE_PERCENT", "101")    # (test_fuzz_gpu.py: small random grids are mostly "dense" and get no walk)
    ctx = vp.Context(0)
    monkeypatch.delenv("VP_DENSE_PERCENT", raising=False)
    return ctx


def _fast_census(vp):
    """launches so far of the fast unit's render_k and approach kernels, by name (the launch census; read, never reset)"""
    return {**vp.launch_census(vp.CENSUS_FAST, vp.CENSUS_RENDER), **vp.launch_census(vp.CENSUS_FAST, vp.CENSUS_APPROACH)}


def _tolerance_zero(vp, seed, c, what):
    """check 1 in the context at hand (fast): returns the image and what the launch ran"""
    P = _setup(vp, c)
    first, n = c["first"], c["nframes"]
    vp.set_arithmetic(vp.ARITH_FAST)
    before = _fast_census(vp)
    one = _render(vp, P, first, n)
    ran = dict(lds_form=vp.last_lds_form(), table=vp.last_approach_table(), approach=vp.last_approach_mode(),
               dtype=str(c["grid"].dtype), chromatic="sigma_t" in c["kw"], inside=_camera_inside(c), est=c["est"], frames=n)
    assert vp.last_arithmetic() == vp.ARITH_FAST
    assert ran["approach"] in (0, 1), (what, ran)      # never the exact arithmetic's throughput table
    assert np.isfinite(one).all() and (one >= 0).all(), what
    buf = vp.DeviceBuffer(c["W"], c["H"])
    try:
        vp.set_lookahead(64)
        for f in range(first, first + n):
            vp.render_kernel(buf.ptr, f, P)
        vp.synchronize()
        assert np.array_equal(buf.download(), one), (what, ran, "render_kernel with the look-ahead")
        ran["lds_form_lookahead"] = vp.last_lds_form()
        vp.set_lookahead(vp.LOOKAHEAD_DEFAULT)
        tot = np.zeros_like(one)
        for r in range(c["world"]):
            vp.set_shard(r, c["world"])
            tot += _render(vp, P, first, n)
        vp.set_shard(0, 1)
        assert np.array_equal(tot, one), (what, ran, "shards")
        buf.reset()
        for f in range(first, first + n):
            vp.render_frames(buf.ptr, f, 1, P)          # one-frame launches: no approach walk
        assert np.array_equal(buf.download(), one), (what, ran, "one-frame launches")
    finally:
        vp.set_lookahead(vp.LOOKAHEAD_DEFAULT)
        vp.set_shard(0, 1)
        buf.free()
    ran["kernels"] = {k for k, v in _fast_census(vp).items() if v > before[k]}
    return one, P, ran


def assert_paired_agreement(d, e, what):
    """check 3 (the bound: test_fast_random_scene's docstring) on d, e = (frames, H, W, 3) float64 one-frame renders of the same
    samples in the fast and in the exact arithmetic; d is overwritten with the differences"""
    frames, H, W = d.shape[:3]
    assert np.isfinite(d).all() and (d >= 0).all(), what
    d -= e
    n = frames * H * W
    mean, se = d.mean((0, 1, 2)), d.std((0, 1, 2)) / np.sqrt(n)
    tol = 5 * se + 1e-5 * np.abs(e.mean((0, 1, 2)))
    assert (np.abs(mean) <= tol).all(), (what, mean, se)
    by, bx = H // 4, W // 4
    if by and bx:
        blk = d[:, :by * 4, :bx * 4].reshape(frames, by, 4, bx, 4, 3).transpose(1, 3, 5, 0, 2, 4).reshape(by, bx, 3, -1)
        bm, bs = blk.mean(-1), blk.std(-1) / np.sqrt(blk.shape[-1])
        out = np.abs(bm) > 5 * bs + 1e-5 * np.abs(e.mean())
        assert out.mean() < 0.01, (what, float(out.mean()))


@pytest.mark.parametrize("seed", range(SEEDS))
def test_fast_random_scene(vp, seed, monkeypatch):
    """Checks 1-3 above.  Check 3: per channel, |mean d| over all samples <= 5 paired standard errors + 1e-5 of the exact mean (the
    fast helpers' rounding is a few 1e-7 per operation and unbiased; 1e-5 covers its systematic part over paths of hundreds of
    operations); and fewer than 1 % of the 4x4-pixel blocks have a mean d beyond 5 of their standard errors.
    False alarms: the paired differences are independent across pixels and frames (each sample has its own stream), so the means are
    close to normal; a 5-sigma excursion has probability 5.7e-7, i.e. 32 seeds x 3 channels x 5.7e-7 = 5.5e-5 for the image-mean
    check of the whole set, and for a block test to fail, 1 % of a seed's blocks (at least one of at most 140) would have to be
    5-sigma outliers: at most 140 x 5.7e-7 = 8e-5 per seed, 2.6e-3 for the set.  The distribution of d is heavy-tailed (most samples
    agree to an ulp, a few take another branch), which lowers |mean| / SE further."""
    from volpath import host
    c = fast_case(seed, host)
    what = dict(seed=seed, grid=c["grid"].shape, dtype=str(c["grid"].dtype), box=c["box"], est=c["est"], rng=c["rng_mode"],
                linear=c["linear"], brick=c["brick"], size=(c["W"], c["H"]), first=c["first"], nframes=c["nframes"], world=c["world"], **c["kw"])
    ctx = _context(vp, seed, monkeypatch)
    try:
        with ctx:
            one, P, ran = _tolerance_zero(vp, seed, c, what)
            COVERAGE[seed] = ran
            # 2. the classes the fast mode leaves exact
            vp.set_arithmetic(vp.ARITH_EXACT)
            ex = _render(vp, P, c["first"], c["nframes"])
            if c["linear"]:   # (point filtering has no pixel classes: every pixel runs the integrator)
                cls = vp.pixel_table(P)[..., 5].astype(int)
                assert np.array_equal(one[cls != 0], ex[cls != 0]), (what, "box-missing / light pixels")
            # 3. paired agreement, one-frame renders of the case's first frame on
            f0 = c["first"]
            H, W = c["H"], c["W"]
            d = np.empty((PAIRED_FRAMES, H, W, 3), np.float64)
            e = np.empty_like(d)
            buf = vp.DeviceBuffer(W, H)
            try:
                for i in range(PAIRED_FRAMES):
                    for m, out in ((vp.ARITH_EXACT, e), (vp.ARITH_FAST, d)):
                        vp.set_arithmetic(m)
                        buf.reset()
                        vp.render_frames(buf.ptr, f0 + i, 1, P)
                        out[i] = buf.download()[..., :3]
            finally:
                buf.free()
            assert_paired_agreement(d, e, what)
    finally:
        ctx.destroy()


def test_fast_fuzz_coverage(vp, monkeypatch):
    """Across the seed set, check 1 ran every LDS form, the segment table, both approach modes the fast mode has, uchar and float
    volumes, achromatic and chromatic media and a camera inside the box -- else a change to the generator could empty the test.
    (Seeds the run did not select are rendered here, check 1 only.)"""
    from volpath import host
    for seed in range(SEEDS):
        if seed not in COVERAGE:
            c = fast_case(seed, host)
            ctx = _context(vp, seed, monkeypatch)
            try:
                with ctx:
                    COVERAGE[seed] = _tolerance_zero(vp, seed, c, dict(seed=seed))[2]
            finally:
                ctx.destroy()
    seen = list(COVERAGE.values())
    have = lambda k: {r[k] for r in seen}
    forms = have("lds_form") | have("lds_form_lookahead")
    assert {0, 1, 2} <= forms, forms
    assert 1 in have("table")
    assert {0, 1} <= have("approach"), have("approach")
    assert {"uint8", "float32"} <= have("dtype")
    assert {True, False} <= have("chromatic")
    assert True in have("inside")
    assert any(r["frames"] >= 64 and r["est"] == 1 for r in seen)
    # ... and what the launch census recorded while check 1 ran: render_k with every LDS form (the fifth digit), a look-ahead
    # instance (CANCEL, the digit before the last), and the three kinds of approach walk
    kernels = set().union(*(r["kernels"] for r in seen))
    render = {k for k in kernels if "." in k}
    assert {k[5] for k in render} == {"0", "1", "2"}, sorted(render)
    assert any(k[-2] == "1" for k in render), sorted(render)
    assert {k[0] for k in kernels - render} == {"g", "l", "t"}, sorted(kernels - render)


@pytest.mark.parametrize("frames", [8, 64])
def test_fast_decomposition_walk_same_staged_and_single_frame(vp, monkeypatch, frames):
    """The decomposition estimator's approach walk (approach_local_k; at 64 frames approach_local_tab_k with the segment table) skips a
    null collision in empty space only where the fast arithmetic finds it neutral, segment by segment.  Julia-64 at these densities has
    segment majorants whose null collision is neutral in IEEE binary32 but not with v_rcp_f32: a walk that asked the IEEE question would
    skip collisions the fast render_k makes, and the staged launch would differ from one-frame launches (which make no walk)."""
    ctx = _context(vp, 1, monkeypatch)      # (no volume taken for dense: the walk runs)
    try:
        with ctx:
            vp.init_volume(vp.julia_volume(64), brick=1, linear=True)
            vp.init_envmap(scenes.synthetic_env())
            vp.set_sun(scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER)
            vp.set_camera()
            vp.set_estimator(vp.EST_DECOMP)
            vp.set_rng(vp.RNG_PHILOX7, (5, 6))
            vp.precompute_opacity(scenes.DEFAULT_SUN_DIR)
            vp.set_arithmetic(vp.ARITH_FAST)
            for density in (123.4, 55.5, 250.0, 1000.0):
                P = vp.make_param(48, 36, density=density)
                staged = _render(vp, P, 0, frames)
                assert vp.last_approach_mode() == 1 and vp.last_approach_table() == (1 if frames >= 64 else 0), density
                single = np.zeros_like(staged)
                for f in range(frames):
                    single += _render(vp, P, f, 1)
                assert np.array_equal(staged, single), (density, frames)
    finally:
        ctx.destroy()
