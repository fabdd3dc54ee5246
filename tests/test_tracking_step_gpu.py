"""GPU parity for the tracking step's trimmed instructions (render_k / approach_k):

  - the sun's light of a shadow ray that ends in the tracking loop is added at the lane's next event visit (the collision block keeps
    the light weight, the ray's end leaves its termination bits), and the collision point is formed at the top of the collision block
    instead of in the step;
  - a Philox word becomes a float with one alignbit instead of a shift and an or (the sampler.h stream, checked beside them, keeps both);
  - the uchar cell split takes the fraction and the truncating conversion instead of a floor.

All three are required to change no bit.  The renders: a small Julia scene in a medium thick enough that paths run into the scatter
cap (800 segments: the ended path's deferred sum is flushed before the path-end chain), over frames 9..12 so that the decomposition
estimator's frame-11 switch to the optical-depth table -- a light estimate that needs no shadow ray -- sits between two deferred
sums.  Bar: the accumulator equals the CPU oracle's bit for bit; no exclusions, no tolerance."""
import ctypes as C

import numpy as np
import pytest

import scenes

pytestmark = pytest.mark.gpu

W, H, N = 24, 16, 32
FIRST, NFRAMES = 9, 4
DENSITY, G = 4000.0, 0.877
KEY = (3, 4)

SUNS = {
    "default": scenes.DEFAULT_SUN_DIR,
    "oblique": (0.48507127, 0.72760689, -0.48507127),
    "zero_component": (0.0, 0.8, -0.6),          # shadow rays that run past the box
    "tiny_component": (1.0e-9, 0.8, -0.6),
}

_REFS = {}


def _oracle(oracle, est, rng_mode, sun, chromatic):
    """the oracle's accumulator over the frames and the largest heat value a single frame added to a pixel (the scatter count of the
    decomposition estimator, a thousandth of the depth index of the global majorant); computed once per case, never modified"""
    k = (est, rng_mode, sun, chromatic)
    if k not in _REFS:
        osc = oracle.OracleScene(oracle.julia(N), scenes.synthetic_env(), SUNS[sun], scenes.DEFAULT_SUN_POWER, estimator=est,
                                 rng_mode=rng_mode, seed=KEY)
        oP = oracle.default_param(W, H, density=DENSITY, g=G)
        if chromatic:
            oracle.mat(oP, *scenes.PRESET1)
        if est == oracle.EST_DECOMP:
            osc.precompute_opacity()
        ref, deepest = None, 0.0
        for f in range(FIRST, FIRST + NFRAMES):
            before = 0.0 if ref is None else ref[..., 3].copy()
            ref, _ = osc.render_frame(oP, f, ref)
            deepest = max(deepest, float((ref[..., 3] - before).max()))
        ref.setflags(write=False)
        _REFS[k] = (ref, deepest)
    return _REFS[k]


def _render(vp, oracle, est, rng_mode, sun, chromatic, exit_mode):
    vP = vp.make_param(W, H, density=DENSITY, g=G)
    if chromatic:
        vp.mat(vP, *scenes.PRESET1)
    buf = vp.DeviceBuffer(W, H)
    try:
        vp.init_volume(oracle.julia(N), brick=1, linear=True)
        vp.init_envmap(scenes.synthetic_env())
        vp.set_sun(SUNS[sun], scenes.DEFAULT_SUN_POWER)
        vp.set_camera()
        vp.set_estimator(est)
        vp.set_rng(rng_mode, KEY)
        vp.set_tracking(0)
        vp.set_envmap_sampling(vp.ENV_PASSIVE)
        vp.set_shard(0, 1)
        vp.enable_counters(False)
        vp.set_exit_flights(exit_mode)
        if est == vp.EST_DECOMP:
            vp.precompute_opacity(SUNS[sun])
        vp.render_frames(buf.ptr, FIRST, NFRAMES, vP)
        return buf.download()
    finally:
        vp.set_exit_flights(1)
        buf.free()


def _cap(oracle, est):
    return 800.0 if est == oracle.EST_DECOMP else float(np.float32(0.8))


@pytest.mark.parametrize("exit_mode", [2, 0], ids=["exit_flights", "no_exit_flights"])
@pytest.mark.parametrize("est", [0, 1], ids=["global", "decomp"])
def test_deferred_light_sum_bit_exact_up_to_the_scatter_cap(vp, oracle, est, exit_mode):
    """exit flights on (mode 2: the decomposition estimator too) and off: the test that ends a path at once sits between the flush
    and the path-end chain"""
    ref, deepest = _oracle(oracle, est, 2, "default", False)
    print(f"est={est}: deepest heat of one frame {deepest!r}")
    assert deepest == _cap(oracle, est), f"the scene does not reach the scatter cap: {deepest}"
    got = _render(vp, oracle, est, 2, "default", False, exit_mode)
    assert np.array_equal(got, ref), f"est={est} exit={exit_mode}: max abs difference {np.abs(got - ref).max()}"


@pytest.mark.parametrize("est", [0, 1], ids=["global", "decomp"])
def test_sampler_h_kernels_unchanged(vp, oracle, est):
    """the sequential stream keeps the reference's order (collision, shadow ray, light, phase function): today's code"""
    ref, deepest = _oracle(oracle, est, 0, "default", False)
    print(f"est={est}: deepest heat of one frame {deepest!r}")
    assert deepest > (20.0 if est == oracle.EST_DECOMP else 0.020), f"the scene does not scatter deep enough: {deepest}"
    got = _render(vp, oracle, est, 0, "default", False, 1)
    assert np.array_equal(got, ref), f"est={est}: max abs difference {np.abs(got - ref).max()}"


@pytest.mark.parametrize("est", [0, 1], ids=["global", "decomp"])
def test_deferred_light_sum_chromatic_medium(vp, oracle, est):
    """three light weights per lane instead of one, three termination bits that differ"""
    ref, deepest = _oracle(oracle, est, 2, "default", True)
    print(f"est={est}: deepest heat of one frame {deepest!r}")
    assert deepest > (20.0 if est == oracle.EST_DECOMP else 0.020), f"no path scatters more than 20 times: {deepest}"
    got = _render(vp, oracle, est, 2, "default", True, 2)
    assert np.array_equal(got, ref), f"est={est}: max abs difference {np.abs(got - ref).max()}"


@pytest.mark.parametrize("sun", ["oblique", "tiny_component", "zero_component"])
@pytest.mark.parametrize("est", [0, 1], ids=["global", "decomp"])
def test_deferred_light_sum_suns(vp, oracle, est, sun):
    """(the default sun is the first test's; the path's own draws do not depend on the sun -- a shadow ray draws from a sub-stream of
    its own -- so every sun reaches the cap)"""
    ref, deepest = _oracle(oracle, est, 2, sun, False)
    print(f"est={est} sun={sun}: deepest heat of one frame {deepest!r}")
    assert deepest == _cap(oracle, est), f"the scene does not reach the scatter cap: {deepest}"
    got = _render(vp, oracle, est, 2, sun, False, 2)
    assert np.array_equal(got, ref), f"est={est} sun={sun}: max abs difference {np.abs(got - ref).max()}"


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["samplerh", "philox10", "philox7"])
def test_draws_equal_the_oracle_streams(vp, oracle, mode):
    for x, y, frame, key in [(0, 0, 0, (0, 0)), (3, 5, 7, (11, 22)), (799, 599, 1023, KEY), (65535, 65535, 0x7fffffff, (0xffffffff, 0x80000001))]:
        a = vp.test_rng(mode, x, y, frame, 4096, key=key)
        b = oracle.rng_stream(mode, x, y, frame, 4096, key=key)
        assert np.array_equal(a, b), (mode, x, y, frame, key, int(np.flatnonzero(a != b)[0]))
        assert a.min() >= 0.0 and a.max() < 1.0


def _split_positions(shape, rng):
    """world positions that probe the texel-centre split of every axis (default box: x in [-1, 1], y and z scaled by the aspect)"""
    nz, ny, nx = shape
    n = np.array([nx, ny, nz])
    bmin = np.array([-1.0, -ny / nx, -nz / nx])
    bmax = -bmin
    ext = bmax - bmin
    centre = lambda a, i: bmin[a] + (np.asarray(i, np.float64) + 0.5) / n[a] * ext[a]
    rows = []
    for a in range(3):
        base = np.array([centre(b, n[b] // 3) for b in range(3)])      # the row: the other two coordinates on a texel centre
        idx = np.arange(n[a])
        cs = centre(a, idx).astype(np.float32)
        # every texel centre of the row, each +- 1 ulp
        vals = [cs, np.nextafter(cs, np.float32(np.inf)), np.nextafter(cs, np.float32(-np.inf))]
        # fractions within 2^-9 below the next centre: the 8-bit weight rounds to 256
        for eps in (2.0 ** -9, 2.0 ** -10, 2.0 ** -12, 2.0 ** -9 + 2.0 ** -16, 2.0 ** -9 - 2.0 ** -16):
            vals.append(centre(a, idx + (1.0 - eps)).astype(np.float32))
        # below the first centre, beyond the last, and the box faces (each +- 1 ulp)
        edge = np.array([bmin[a], bmax[a], centre(a, -0.25), centre(a, -0.5 + 1e-3), centre(a, n[a] - 0.75), centre(a, n[a] - 0.5 - 1e-3),
                         bmin[a] - 0.1, bmax[a] + 0.1, bmin[a] - 100.0, bmax[a] + 100.0], np.float32)
        vals += [edge, np.nextafter(edge, np.float32(np.inf)), np.nextafter(edge, np.float32(-np.inf))]
        v = np.concatenate(vals)
        p = np.tile(base.astype(np.float32), (len(v), 1))
        p[:, a] = v
        rows.append(p)
        # the same row off the other axes' centres (weights in all three stages)
        q = p.copy()
        q[:, (a + 1) % 3] += np.float32(0.37 / n[(a + 1) % 3] * ext[(a + 1) % 3])
        q[:, (a + 2) % 3] -= np.float32(0.21 / n[(a + 2) % 3] * ext[(a + 2) % 3])
        rows.append(q)
    rows.append(rng.uniform(-1.3, 1.3, (50000, 3)).astype(np.float32))   # inside and outside the box (clamp addressing)
    return np.ascontiguousarray(np.concatenate(rows), np.float32)


@pytest.mark.parametrize("linear", [True, False], ids=["linear", "point"])
@pytest.mark.parametrize("volume", ["random_11x13x17", "julia32"])
def test_cell_split_equals_the_oracle_fetch(vp, oracle, volume, linear):
    rng = np.random.default_rng(29)
    if volume == "julia32":
        grid = oracle.julia(N)
    else:
        grid = rng.integers(0, 256, (11, 13, 17), dtype=np.uint8)
        grid[rng.random(grid.shape) < 0.3] = 0
    osc = oracle.OracleScene(grid, scenes.synthetic_env(), scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER, linear=linear)
    vp.init_volume(grid, linear=linear)
    pts = _split_positions(grid.shape, rng)
    got = vp.test_sample_density(pts)
    f = oracle.lib().vpo_sample_density
    S, base = C.byref(osc.S), pts.ctypes.data
    ref = np.array([f(S, C.c_void_p(base + 12 * i)) for i in range(len(pts))], np.float32)
    bad = np.flatnonzero(got != ref)
    assert len(bad) == 0, (len(bad), pts[bad[0]], got[bad[0]], ref[bad[0]])
