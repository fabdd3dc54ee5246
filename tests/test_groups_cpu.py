"""Light groups (include/volpath.h vp_render_frames_groups / vp_relight) without a GPU: the declared and exported
symbols, the refusals that come before the device, the groups census, the numpy restatement of vp_relight, the CLI flags, and the
oracle-built expectation of tests/groups_lib.py checked against itself -- the twins stay on the real scene's path and add up to it."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import groups_lib as GL
import layers_lib as LL
import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cuda-volpath_amd", "volpath_render")
E_STATE, E_ARG = -2, -3
F32 = np.float32
W, H = GL.W, GL.H


# ---- the interface
def test_symbols_are_declared_exported_and_typed():
    import volpath
    text = open(os.path.join(ROOT, "include", "volpath.h")).read()
    for n in ("vp_render_frames_groups", "vp_relight", "vp_test_groups_census", "vp_reserve_frames_groups"):
        assert n in volpath.PART2_SYMBOLS
        assert re.search(r"\bint\s+%s\s*\(" % n, text), n
        assert hasattr(volpath.lib(), n)
    assert re.search(r"int\s+vp_render_frames_groups\(vp_float4\*\s*d_sun,\s*vp_float4\*\s*d_sky,\s*int first_frame,\s*int n_frames,\s*const Param\*\s*p\);", text)
    assert re.search(r"int\s+vp_relight\(vp_float4\*\s*dst,\s*const vp_float4\*\s*sun,\s*const vp_float4\*\s*sky,\s*const float sun_gain\[3\],"
                     r"\s*const float sky_gain\[3\],\s*int size,\s*float scale\);", text)
    assert re.search(r"int\s+vp_test_groups_census\(uint32_t\*\s*launches,\s*uint8_t\*\s*built,\s*size_t count,\s*int reset\);", text)
    L = volpath.lib()
    assert L.vp_render_frames_groups.argtypes == [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(volpath.Param)]
    assert L.vp_relight.argtypes == [C.c_void_p] * 3 + [C.POINTER(C.c_float)] * 2 + [C.c_int, C.c_float]
    assert callable(volpath.render_frames_groups) and callable(volpath.relight) and callable(volpath.groups_census)
    for phrase in ("groups combined with layers", "statistics, adaptive rounds or vp_denoise on groups", "reducing groups across"):
        assert phrase in " ".join(text.split()).replace(" * ", " "), phrase      # what is not built is said in the header


def test_refusals_come_before_the_device():
    """VP_E_ARG for the arguments, VP_E_STATE for the modes the call is not built for: the pointers are never followed and no device
    is asked for (this machine has none)"""
    import volpath
    L = volpath.lib()
    P = volpath.make_param(16, 8)
    sun, sky = C.c_void_p(0x1000), C.c_void_p(0x2000)       # never dereferenced
    f = L.vp_render_frames_groups
    assert f(None, sky, 0, 2, C.byref(P)) == E_ARG and f(sun, None, 0, 2, C.byref(P)) == E_ARG and f(sun, sun, 0, 2, C.byref(P)) == E_ARG
    assert f(sun, sky, 0, 2, None) == E_ARG and f(sun, sky, 0, 0, C.byref(P)) == E_ARG and f(sun, sky, -1, 2, C.byref(P)) == E_ARG
    assert "vp_render_frames_groups" in L.vp_last_error().decode()
    try:
        for mode in (volpath.TRACK_SCALAR, volpath.TRACK_MULTI_CHANNEL):
            volpath.set_tracking(mode)
            assert f(sun, sky, 0, 2, C.byref(P)) == E_STATE
            assert "spectral" in L.vp_last_error().decode()
        volpath.set_tracking(volpath.TRACK_SPECTRAL)
        assert L.vp_enable_counters(1) == 0
        assert f(sun, sky, 0, 2, C.byref(P)) == E_STATE
        assert "counters" in L.vp_last_error().decode()
        L.vp_enable_counters(0)
        # (the setters of the environment mode and the arithmetic ask for the device themselves: where there is none they fail and
        # the mode stays; tests/test_groups_gpu.py makes both refusals with the buffers checked)
        if L.vp_set_envmap_sampling(volpath.ENV_MIS) == 0:
            assert f(sun, sky, 0, 2, C.byref(P)) == E_STATE
            assert "passive" in L.vp_last_error().decode()
            assert L.vp_set_envmap_sampling(volpath.ENV_PASSIVE) == 0
        if L.vp_set_arithmetic(volpath.ARITH_FAST) == 0:
            assert f(sun, sky, 0, 2, C.byref(P)) == E_STATE
            assert "exact" in L.vp_last_error().decode()
            assert L.vp_set_arithmetic(volpath.ARITH_EXACT) == 0
    finally:
        volpath.set_tracking(volpath.TRACK_SPECTRAL)
        L.vp_enable_counters(0)
    with pytest.raises(volpath.VolpathError, match="vp_render_frames_groups"):
        volpath.render_frames_groups(sun, sun, 0, 1, P)
    g = L.vp_relight
    one = (C.c_float * 3)(1.0, 1.0, 1.0)
    assert g(None, sun, sky, one, one, 4, 1.0) == E_ARG and g(sun, None, sky, one, one, 4, 1.0) == E_ARG and g(sun, sun, None, one, one, 4, 1.0) == E_ARG
    assert g(sun, sun, sky, None, one, 4, 1.0) == E_ARG and g(sun, sun, sky, one, None, 4, 1.0) == E_ARG and g(sun, sun, sky, one, one, -1, 1.0) == E_ARG
    assert "vp_relight" in L.vp_last_error().decode()


def test_groups_census_has_the_layers_set_and_leaves_the_launch_census_alone():
    import volpath
    L = volpath.lib()
    n = L.vp_test_groups_census(None, None, 0, 0)
    assert n == 10368 == L.vp_test_launch_census(0, 0, None, None, 0, 0)
    launches, built = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    for wrong in (0, n - 1, n + 1):
        assert L.vp_test_groups_census(launches.ctypes.data, built.ctypes.data, wrong, 0) == E_ARG
    assert L.vp_test_groups_census(launches.ctypes.data, built.ctypes.data, n, 0) == 0
    assert int(built.sum()) == 79 and not launches.any()
    census = volpath.groups_census()
    assert set(census) == set(volpath.launch_census(volpath.CENSUS_EXACT, volpath.CENSUS_LAYERS)) and len(census) == 79
    assert L.vp_test_launch_census(0, 3, None, None, 0, 0) == E_ARG          # no fourth kind: the groups table has a hook of its own


def test_relight_restatement_is_one_rounding_per_operation():
    sun = np.array([[0.3, 7.0, 1e-3, 5.0]], F32)
    sky = np.array([[3.0, 0.25, 2.0, 5.0]], F32)
    s = F32(1.0) / F32(3.0)
    gs, gk = np.array([2.0, 0.5, 0.0], F32), np.array([0.1, 1.0, 3.0], F32)
    want = [F32(F32(F32(sun[0, c] * s) * gs[c]) + F32(F32(sky[0, c] * s) * gk[c])) for c in range(3)] + [F32(sun[0, 3] * s)]
    assert GL.relight(sun, sky, s, gs, gk)[0].tolist() == [float(v) for v in want]
    # a gain of 0 removes a group, gains of 1 leave the scaled sum
    assert GL.relight(sun, sky, s, (1, 1, 1), (0, 0, 0))[0, :3].tolist() == [float(F32(v * s)) for v in sun[0, :3]]
    assert GL.relight(sun, sky, s)[0, :3].tolist() == [float(F32(F32(a * s) + F32(k * s))) for a, k in zip(sun[0, :3], sky[0, :3])]


def test_cli_group_flags():
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--groups-out PREFIX", "--sun-gain R G B", "--sky-gain R G B"):
        assert flag in r.stdout, flag
    for bad in (["--groups-out"], ["--sun-gain", "1", "2"], ["--sky-gain", "1", "x", "3"], ["--sun-gain", "1", "2", "nan"]):
        r = subprocess.run([EXE] + bad, capture_output=True, text=True)
        assert r.returncode == 2, (bad, r.stdout, r.stderr)
    for group in (["--groups-out", "x"], ["--sun-gain", "2", "0.5", "0"], ["--sky-gain", "0", "1", "3"]):
        for other in (["--gpus", "2"], ["--noise", "0.05"], ["--denoise"], ["--layers-out", "y"]):
            r = subprocess.run([EXE] + group + other, capture_output=True, text=True)
            assert r.returncode == 2 and group[0] in r.stderr and other[0] in r.stderr, (group, other, r.stderr)
        for other in (["--tracking", "scalar"], ["--tracking", "multichannel"], ["--env", "mis"], ["--arith", "fast", "--rng", "philox", "--estimator", "global"]):
            r = subprocess.run([EXE] + group + other, capture_output=True, text=True)
            assert r.returncode == 2 and group[0] in r.stderr, (group, other, r.stderr)


# ---- the expectation against itself
ADD_CASES = [(n, e, r) for n in ("julia", "soft") for e in (0, 1, 2) for r in (0, 2)]


@pytest.mark.parametrize("name,est,rng_mode", ADD_CASES, ids=["%s-est%d-rng%d" % c for c in ADD_CASES])
def test_the_twins_stay_on_the_path_and_add_up_to_the_real_sample(oracle, name, est, rng_mode):
    """Frames 0..2 at 16 x 12.  Per sample (asserted in groups_lib.sample): both twins report the real sample's rng_draws, scatters and
    density_lookups, and its w.  Their RGB add up to the real sample within 3 * 2^-24 of the larger of the two, per channel:
    with x = b (R + E) in exact arithmetic on the rounded R and E, the real sample is x (1 + d1)(1 + d2) (the sum, the brightness),
    the twins' are b R (1 + d3) and b E (1 + d4) (R + 0 and 0 + E are exact), all |d| <= u = 2^-24 and all terms non-negative, so
    real = x (1 + r), |r| <= 2u + u^2, and sun + sky = x (1 + s), |s| <= u, the latter formed in float64 without a rounding.
    |real - (sun + sky)| / max(real, sun + sky) = |r - s| / (1 + max(r, s)) <= (3u + u^2) / (1 + 2u + u^2) < 3u in the one extreme
    and (3u - u^2) / (1 + u) < 3u in the other: three roundings, the second-order term absorbed by the denominator.
    Measured here, with this denominator: at most 2.01 * 2^-24."""
    E = GL.expected(oracle, name, est, rng_mode, frames=(0, 1, 2))
    print("worst per-sample additivity error: %.3f * 2^-24" % (E.worst * 2.0 ** 24))
    assert E.worst <= GL.ADDITIVITY, E.worst * 2.0 ** 24
    # both groups are populated: some samples get sunlight, every pixel gets skylight in some frame; the groups carry the beauty w
    lit = E.lit_sun.any(0)
    assert 1 <= int(lit.sum()) < W * H and E.lit_sky.any(0).all(), (int(lit.sum()), int(E.lit_sky.any(0).sum()))
    assert np.array_equal(E.sun[..., 3], E.beauty[..., 3]) and np.array_equal(E.sky[..., 3], E.beauty[..., 3])
    assert np.isfinite(E.sun).all() and np.isfinite(E.sky).all() and (E.sun >= 0).all() and (E.sky >= 0).all()
    # the sun reaches a sample through a scatter event only (the default camera looks away from the disc)
    assert not (E.lit_sun & ~E.scattered).any()


def test_the_scenes_of_the_gpu_tests_reach_every_kind_of_pixel(oracle):
    """non-vacuity of tests/test_groups_gpu.py on its frames (10, 11): box-missing pixels, pixels that scatter, and at least one pixel
    with sun > 0 and sky > 0 at once"""
    for name, est in (("julia", 0), ("julia", 1), ("soft", 0), ("soft", 1), ("soft", 2)):
        E = GL.expected(oracle, name, est, 1)
        assert E.miss.any() and E.scattered.any() and not E.scattered.all(), (name, est)
        both = (E.sun[..., :3].max(-1) > 0) & (E.sky[..., :3].max(-1) > 0)
        assert both.any(), (name, est)
        assert not E.sun[E.miss][:, :3].any() and (E.sky[E.miss][:, :3].max(-1) > 0).all()      # a ray that misses the box sees the sky only


def test_sun_disc_sample_goes_to_the_sun_group(oracle):
    """A camera whose axis is the sun direction: pixel (W/2, H/2) looks into the disc.  Where its path is unscattered the sun twin's
    sample is b (thr o sun_power_original) -- thr from layers_lib's unit-background twin -- and the sky twin's is 0."""
    view = GL.sun_axis_view()
    d = LL.camera_dir(list(view.ravel()), W, H, W // 2, H // 2)
    assert np.allclose(d, np.asarray(scenes.DEFAULT_SUN_DIR, F32) / np.linalg.norm(scenes.DEFAULT_SUN_DIR), atol=1e-6)
    g = LL.soft_grid()
    kw = dict(estimator=0, rng_mode=1, seed=GL.KEY, inv_view=view)
    real, sun, sky = GL.scenes_for(oracle, g, GL.ENV, scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER, **kw)
    _, unit = LL.scenes_for(oracle, g, GL.ENV, scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER, **kw)
    P = oracle.default_param(W, H, **LL.SOFT_KW)
    Q = LL.twin_param(oracle, P)
    b, power = F32(P.brightness), np.asarray(scenes.DEFAULT_SUN_POWER, F32)
    seen = 0
    for f in range(10, 40):
        a, k, v, cnt = GL.sample(real, sun, sky, P, W // 2, H // 2, f)
        if cnt.scatters:
            continue
        thr = unit.render_sample(Q, W // 2, H // 2, f)[0][:3]
        assert np.array_equal(a[:3], np.maximum((power * thr) * b, F32(0.0))), (f, a, thr)
        assert not k[:3].any() and np.array_equal(a, v), (f, k, v)
        assert (thr != 1).all() and (thr > 0).all()         # tracked through the chromatic medium: spectral weights, not 1
        seen += 1
    assert seen >= 2, seen
