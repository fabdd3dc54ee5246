"""GPU parity on degenerate geometry (tests/degenerate_cases.py): axis-parallel camera rays and suns, cameras on a face, on an edge,
at the centre, in a face plane and in a cell-boundary plane of the box.  Bar: the HIP path equals the CPU oracle bit for bit
(tolerance 0) and does the same work; tests/test_reference_kernel_cpu.py holds the oracle to the reference's own kernel code on a
subset of these cases, which is where the NaN semantics of the slab test are decided.

Every optimisation since round 2 is a geometric claim about a ray (the slab test axis by axis, the restart crawl and the segment
table, the approach walks, the pixel classes, the exit flights' direction classes, the sun-clip table, the texel-centre cell
split); the randomised scenes hold them for rays in general position only.

What keeps the comparisons honest is asserted, not assumed: the oracle's accumulator of every case is finite (so equal_nan hides
nothing), every camera has a pixel with two exact zero direction components and W + H - 2 with one, and per grid the two-zero
pixel of some camera is integrated (pixel class 0, heat > 0), not filled.
"""
import numpy as np
import pytest

import degenerate_cases as DC
import scenes

pytestmark = pytest.mark.gpu

KEY = (0x51ED270B, 77)
COUNTERS = ("samples", "density_lookups", "bound_lookups", "opacity_lookups", "env_lookups", "scatters")
MEDIA = {"plain": dict(density=60.0), "thin": dict(density=5.0),
         "chromatic": dict(density=60.0, g=0.5, albedo=(0.95, 0.8, 0.6), sigma_t=(1.0, 0.7, 0.45))}
W, H = DC.W, DC.H


@pytest.fixture(scope="module")
def ctx(vp):
    """a context of this module's own: cameras, suns, exit-flight modes and arithmetic set here never reach another module"""
    c = vp.Context(0)
    try:
        with c:
            yield c
    finally:
        c.destroy()


# ---------------------------------------------------------------------------------------------------------------- the oracle
_ORACLE = {}


def _oracle(oracle, grid, cam, sun, est, rng_mode, brick, medium, first, n, size=(W, H)):
    """(accumulator, summed counters) of the oracle: computed once per case, shared, never written to"""
    k = (grid, None if cam is None else cam.tobytes(), sun, est, rng_mode, brick, medium, first, n, size)
    if k not in _ORACLE:
        sc = oracle.OracleScene(DC.grid(grid, oracle), scenes.synthetic_env(), sun, scenes.DEFAULT_SUN_POWER, box=DC.user_box(grid),
                                brick=brick, estimator=est, rng_mode=rng_mode, seed=KEY, inv_view=cam)
        if est == 1 and first + n - 1 > 10:
            sc.precompute_opacity()
        P = oracle.default_param(size[0], size[1], **MEDIA[medium])
        acc, cnt = None, None
        for f in range(first, first + n):
            acc, c = sc.render_frame(P, f, acc)
            d = c.as_dict()
            cnt = d if cnt is None else {q: cnt[q] + d[q] for q in d}
        assert np.isfinite(acc).all(), ("the oracle's accumulator is not finite: change the case", k[0], k[2:])
        assert oracle.lib().vpo_debug_shadow_overflow() == 0
        acc.setflags(write=False)
        _ORACLE[k] = (acc, cnt)
    return _ORACLE[k]


def _scene(vp, oracle, grid, cam, sun, est, rng_mode, brick, late):
    vp.set_arithmetic(vp.ARITH_EXACT)
    vp.set_subpixel(1)
    vp.init_volume(DC.grid(grid, oracle), box=DC.user_box(grid), brick=brick, linear=True)
    vp.init_envmap(scenes.synthetic_env())
    vp.set_sun(sun, scenes.DEFAULT_SUN_POWER)
    vp.set_camera() if cam is None else vp.set_camera(tuple(float(v) for v in cam))
    vp.set_estimator(est)
    vp.set_rng(rng_mode, KEY)
    vp.set_tracking(0)
    vp.set_envmap_sampling(vp.ENV_PASSIVE)
    vp.set_shard(0, 1)
    vp.set_lookahead(vp.LOOKAHEAD_DEFAULT)
    if late:
        vp.precompute_opacity(sun)


def _three_ways(vp, P, first, n, ref, cnt, what):
    """the staged launch, the counting launch and one render_kernel call per frame: all three equal the oracle, and the counting
    launch did the oracle's work"""
    buf = vp.DeviceBuffer(P.width, P.height)
    try:
        vp.render_frames(buf.ptr, first, n, P)
        got = buf.download()
        assert np.array_equal(got, ref, equal_nan=True), (what, "render_frames", np.argwhere(got != ref)[:4].tolist())
        vp.enable_counters(True)
        vp.read_counters(reset=True)
        buf.reset()
        vp.render_frames(buf.ptr, first, n, P)
        k = vp.read_counters()
        vp.enable_counters(False)
        got = buf.download()
        assert np.array_equal(got, ref, equal_nan=True), (what, "counting launch", np.argwhere(got != ref)[:4].tolist())
        for q in COUNTERS:
            assert k[q] == cnt[q], (what, q, k[q], cnt[q])
        buf.reset()
        for f in range(first, first + n):
            vp.render_kernel(buf.ptr, f, P)
        got = buf.download()
        assert np.array_equal(got, ref, equal_nan=True), (what, "render_kernel", np.argwhere(got != ref)[:4].tolist())
    finally:
        vp.enable_counters(False)
        buf.free()


def _census(cam, width=W, height=H):
    zeros = DC.ray_census(cam, width, height)
    assert (zeros == 2).sum() >= 1 and zeros[height // 2, width // 2] == 2, zeros
    assert (zeros == 1).sum() >= width + height - 2, zeros


# ------------------------------------------------------------------------------------------------------------------- cameras
def _camera_cases():
    """Every position x every grid, and the remaining five views of `outside` on the Julia grid.  The view, the brick size of the
    local estimators, the exit-flight mode and the medium rotate through the list: every Julia case runs all three estimators, and
    the Julia cases cover the three exit-flight modes several times over."""
    out = []
    for gi, g in enumerate(DC.GRIDS):
        for pi, p in enumerate(DC.POSITIONS):
            k = len(out)
            axis, sign = DC.VIEWS[(gi + 2 * pi) % 6]
            medium = "chromatic" if (g, p) == ("julia32", "in_cell_plane") else "thin" if (g, p) in (("julia32", "on_face"), ("odd_u8", "outside")) else "plain"
            out.append((g, p, axis, sign, (1, 4)[k % 2], k % 3, medium))
    for i, (axis, sign) in enumerate(DC.VIEWS[1:]):
        out.append(("julia32", "outside", axis, sign, (4, 1)[i % 2], (i + 1) % 3, ("thin", "plain", "thin", "chromatic", "thin")[i]))
    return out


CAMERA_CASES = _camera_cases()
_id = lambda c: f"{c[0]}-{c[1]}-{'xyz'[c[2]]}{'+' if c[3] > 0 else '-'}-b{c[4]}-x{c[5]}-{c[6]}"


def test_camera_cases_cover_what_they_claim():
    assert {(c[0], c[1]) for c in CAMERA_CASES} == {(g, p) for g in DC.GRIDS for p in DC.POSITIONS}
    julia = [c for c in CAMERA_CASES if c[0] == "julia32"]
    assert {c[5] for c in julia} == {0, 1, 2} and {(c[2], c[3]) for c in julia if c[1] == "outside"} == set(DC.VIEWS)
    assert {c[4] for c in CAMERA_CASES if c[0].startswith("odd")} == {1, 4} and {c[6] for c in CAMERA_CASES} == set(MEDIA)
    assert 60 <= len(CAMERA_CASES) + len(SUN_CASES) + len(LONG_CASES) + len(FAST_CASES) + len(DC.GRIDS) + 1 <= 100


@pytest.mark.parametrize("case", CAMERA_CASES, ids=_id)
def test_degenerate_camera_bit_exact(vp, ctx, oracle, case):
    """three estimators x sampler.h and Philox-7 over frames 0..2, and the decomposition estimator over frames 9..12 (across the
    frame-11 switch to the optical-depth table)"""
    grid, position, axis, sign, brick, exit_mode, medium = case
    cam = DC.camera(grid, position, axis, sign)
    _census(cam)
    sun = scenes.DEFAULT_SUN_DIR
    vp.set_exit_flights(exit_mode)
    for est in (vp.EST_GLOBAL, vp.EST_DECOMP, vp.EST_BOUNDED):
        b = brick if est else 1
        for rng_mode in (vp.RNG_SAMPLERH, vp.RNG_PHILOX7):
            for first, n in ((0, 3), (9, 4)) if est == vp.EST_DECOMP else ((0, 3),):
                ref, cnt = _oracle(oracle, grid, cam, sun, est, rng_mode, b, medium, first, n)
                _scene(vp, oracle, grid, cam, sun, est, rng_mode, b, late=first + n - 1 > 10)
                P = vp.make_param(W, H, **MEDIA[medium])
                _three_ways(vp, P, first, n, ref, cnt, dict(case=_id(case), est=est, rng=rng_mode, brick=b, first=first, n=n))


@pytest.mark.parametrize("grid", DC.GRIDS)
def test_the_two_zero_ray_is_integrated_not_filled(vp, ctx, oracle, grid):
    """non-vacuity: from some camera of the grid the centre pixel -- the axis-parallel ray -- is a general pixel (class 0 of
    vp_get_pixel_table) and gathers heat: the degenerate ray goes through the integrator"""
    found = []
    for c in CAMERA_CASES:
        if c[0] != grid:
            continue
        cam = DC.camera(grid, c[1], c[2], c[3])
        ref, _ = _oracle(oracle, grid, cam, scenes.DEFAULT_SUN_DIR, vp.EST_GLOBAL, vp.RNG_PHILOX7, 1, c[6], 0, 3)
        _scene(vp, oracle, grid, cam, scenes.DEFAULT_SUN_DIR, vp.EST_GLOBAL, vp.RNG_PHILOX7, 1, late=False)
        cls = vp.pixel_table(vp.make_param(W, H, **MEDIA[c[6]]))[..., 5].astype(int)
        if cls[H // 2, W // 2] == 0 and ref[H // 2, W // 2, 3] > 0:
            found.append(_id(c))
        assert (ref[..., 3] > 0).any(), (_id(c), "no ray of this camera meets the medium")
    assert found, grid


# ---------------------------------------------------------------------------------------------------------------------- suns
SUN_CASES = [(g, s, cam) for g in ("julia32", "odd_u8") for s in DC.SUNS for cam in ("axis", "default")]


@pytest.mark.parametrize("grid,sun,cam", SUN_CASES)
def test_axis_parallel_sun_bit_exact(vp, ctx, oracle, grid, sun, cam):
    """shadow rays with two zero direction components: the sun-clip table and the shadow sub-streams of Philox-7, the slab test of
    Tr_spectral on sampler.h; global majorant and decomposition (optical-depth table along the axis), frames 9..12"""
    i = list(DC.SUNS).index(sun)
    view = None if cam == "default" else DC.camera(grid, "outside", *DC.VIEWS[(i + 3) % 6])
    vp.set_exit_flights(i % 3)
    for est in (vp.EST_GLOBAL, vp.EST_DECOMP):
        for rng_mode in (vp.RNG_SAMPLERH, vp.RNG_PHILOX7):
            ref, cnt = _oracle(oracle, grid, view, DC.SUNS[sun], est, rng_mode, 1, "plain", 9, 4)
            assert (ref[..., 3] > 0).any()
            _scene(vp, oracle, grid, view, DC.SUNS[sun], est, rng_mode, 1, late=est == vp.EST_DECOMP)
            _three_ways(vp, vp.make_param(W, H, **MEDIA["plain"]), 9, 4, ref, cnt, dict(grid=grid, sun=sun, cam=cam, est=est, rng=rng_mode))


# ------------------------------------------------------------------------------------------------------------- long launches
LONG_CASES = [("julia32", "outside", 0, 1, 1), ("julia32", "in_face_plane", 1, -1, 0), ("odd_u8", "in_cell_plane", 2, 1, 1),
              ("julia32", "in_cell_plane", 2, -1, 0)]


@pytest.mark.parametrize("grid,position,axis,sign,est", LONG_CASES)
def test_degenerate_long_launch_bit_exact(vp, oracle, monkeypatch, grid, position, axis, sign, est):
    """64 frames at 8x6, Philox-7, in a context that takes no volume for dense (the pattern of
    test_random_scene_long_launch_bit_exact): the approach walk runs, and for the decomposition estimator it reads the per-view
    segment table of approach_segments_k -- built from the degenerate camera rays"""
    cam = DC.camera(grid, position, axis, sign)
    _census(cam, DC.LONG_W, DC.LONG_H)
    size = (DC.LONG_W, DC.LONG_H)
    ref, cnt = _oracle(oracle, grid, cam, scenes.DEFAULT_SUN_DIR, est, vp.RNG_PHILOX7, 1, "plain", 0, 64, size)
    assert (ref[..., 3] > 0).any()
    monkeypatch.setenv("VP_DENSE_PERCENT", "101")
    c = vp.Context(0)
    monkeypatch.delenv("VP_DENSE_PERCENT")
    try:
        with c:
            _scene(vp, oracle, grid, cam, scenes.DEFAULT_SUN_DIR, est, vp.RNG_PHILOX7, 1, late=est == vp.EST_DECOMP)
            P = vp.make_param(*size, **MEDIA["plain"])
            buf = vp.DeviceBuffer(*size)
            try:
                vp.render_frames(buf.ptr, 0, 64, P)
                got = buf.download()
                mode, table = vp.last_approach_mode(), vp.last_approach_table()
                assert np.array_equal(got, ref, equal_nan=True), (mode, table, np.argwhere(got != ref)[:4].tolist())
                assert mode != 0, "the approach walk did not run"
                assert table == (1 if est == vp.EST_DECOMP and mode == 1 else 0)       # a uchar volume: the table is read where it can be
                vp.enable_counters(True)
                vp.read_counters(reset=True)
                buf.reset()
                vp.render_frames(buf.ptr, 0, 64, P)
                k = vp.read_counters()
                vp.enable_counters(False)
                assert np.array_equal(buf.download(), ref, equal_nan=True)
                for q in COUNTERS:
                    assert k[q] == cnt[q], (q, k[q], cnt[q])
            finally:
                vp.enable_counters(False)
                buf.free()
    finally:
        c.destroy()


# ----------------------------------------------------------------------------------------------------------- fast arithmetic
FAST_CASES = [(g, p) for g in ("julia32", "odd_u8") for p in DC.POSITIONS]


@pytest.mark.parametrize("grid,position", FAST_CASES)
def test_degenerate_camera_fast_arithmetic(vp, ctx, oracle, grid, position):
    """include/volpath.h's promise for VP_ARITH_FAST on the camera cases (Philox-7, global majorant and decomposition): the image is
    finite, and the pixels of classes 1 and 2 are bit-identical to the exact mode.  No oracle comparison."""
    axis, sign = DC.VIEWS[(DC.POSITIONS.index(position) + (grid == "odd_u8")) % 6]
    cam = DC.camera(grid, position, axis, sign)
    _census(cam)
    try:
        for est in (vp.EST_GLOBAL, vp.EST_DECOMP):
            _scene(vp, oracle, grid, cam, scenes.DEFAULT_SUN_DIR, est, vp.RNG_PHILOX7, 1, late=False)
            P = vp.make_param(W, H, **MEDIA["plain"])
            img = {}
            buf = vp.DeviceBuffer(W, H)
            try:
                for mode in (vp.ARITH_FAST, vp.ARITH_EXACT):
                    vp.set_arithmetic(mode)
                    buf.reset()
                    vp.render_frames(buf.ptr, 0, 3, P)
                    assert vp.last_arithmetic() == mode
                    img[mode] = buf.download()
            finally:
                buf.free()
            cls = vp.pixel_table(P)[..., 5].astype(int)
            fast, exact = img[vp.ARITH_FAST], img[vp.ARITH_EXACT]
            assert np.isfinite(fast).all() and (fast >= 0).all(), (grid, position, est)
            assert np.array_equal(fast[cls != 0], exact[cls != 0]), (grid, position, est)
            assert (exact[..., 3] > 0).any()
    finally:
        vp.set_arithmetic(vp.ARITH_EXACT)
