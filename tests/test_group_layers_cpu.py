"""Group layers (include/volpath.h vp_render_frames_group_layers, its _stats form and vp_relight_composite)
without a GPU: the declared and exported symbols, the refusals that come before the device, the census of the third table, the CLI
flags, the numpy restatement of vp_relight_composite against the restated three-step sequence, and the oracle-built expectation of
tests/group_layers_lib.py checked against itself."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import group_layers_lib as GLL
import groups_lib as GL
import layers_lib as LL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cuda-volpath_amd", "volpath_render")
E_STATE, E_ARG = -2, -3
F32 = np.float32
W, H, FRAMES = GLL.W, GLL.H, GLL.FRAMES
NEW = ("vp_render_frames_group_layers", "vp_render_frames_group_layers_stats", "vp_relight_composite", "vp_test_group_layers_census")


# ---- the interface
def test_symbols_are_declared_exported_and_typed():
    import volpath
    text = open(os.path.join(ROOT, "include", "volpath.h")).read()
    for n in NEW:
        assert n in volpath.PART2_SYMBOLS
        assert re.search(r"\bint\s+%s\s*\(" % n, text), n
        assert hasattr(volpath.lib(), n)
    assert re.search(r"int\s+vp_render_frames_group_layers\(vp_float4\*\s*d_sun,\s*vp_float4\*\s*d_sky,\s*vp_float4\*\s*d_trans,\s*int first_frame,"
                     r"\s*int n_frames,\s*const Param\*\s*p\);", text)
    assert re.search(r"int\s+vp_render_frames_group_layers_stats\(vp_float4\*\s*d_sun,\s*vp_float4\*\s*d_sky,\s*vp_float4\*\s*d_trans,\s*vp_pixel_stats\*\s*d_sun_stats,"
                     r"\s*vp_pixel_stats\*\s*d_sky_stats,\s*vp_pixel_stats\*\s*d_trans_stats,\s*int first_frame,\s*int n_frames,\s*const Param\*\s*p\);", text)
    assert re.search(r"int\s+vp_relight_composite\(vp_float4\*\s*dst,\s*const vp_float4\*\s*sun,\s*const vp_float4\*\s*sky,\s*const vp_float4\*\s*trans,"
                     r"\s*const float sun_gain\[3\],\s*const float sky_gain\[3\],\s*const vp_float4\*\s*plate,\s*const float plate_rgb\[3\],\s*int size,\s*float scale\);", text)
    assert re.search(r"int\s+vp_test_group_layers_census\(uint32_t\*\s*launches,\s*uint8_t\*\s*built,\s*size_t count,\s*int reset\);", text)
    L = volpath.lib()
    assert L.vp_render_frames_group_layers.argtypes == [C.c_void_p] * 3 + [C.c_int, C.c_int, C.POINTER(volpath.Param)]
    assert L.vp_render_frames_group_layers_stats.argtypes == [C.c_void_p] * 6 + [C.c_int, C.c_int, C.POINTER(volpath.Param)]
    assert L.vp_relight_composite.argtypes == [C.c_void_p] * 4 + [C.POINTER(C.c_float)] * 2 + [C.c_void_p, C.POINTER(C.c_float), C.c_int, C.c_float]
    assert all(callable(getattr(volpath, n)) for n in ("render_frames_group_layers", "render_frames_group_layers_stats", "relight_composite", "group_layers_census"))
    flat = " ".join(text.split()).replace(" * ", " ")
    section = flat[flat.index("Group layers (DESIGN.md section 2.10)"):]
    for phrase in ("adaptive rounds on three planes", "across processes", "under VP_ARITH_FAST"):      # what stays unbuilt is said
        assert phrase in section, phrase
    assert "Not built: groups combined with layers" not in flat and "not built: groups combined with layers" not in flat


def _state_refusals(volpath, call):
    """VP_E_STATE exactly where plane_state_check gives it; the modes whose setters need a device are made where there is one"""
    L = volpath.lib()
    try:
        for mode in (volpath.TRACK_SCALAR, volpath.TRACK_MULTI_CHANNEL):
            volpath.set_tracking(mode)
            assert call() == E_STATE
            assert "spectral" in L.vp_last_error().decode()
        volpath.set_tracking(volpath.TRACK_SPECTRAL)
        assert L.vp_enable_counters(1) == 0
        assert call() == E_STATE
        assert "counters" in L.vp_last_error().decode()
        L.vp_enable_counters(0)
        if L.vp_set_envmap_sampling(volpath.ENV_MIS) == 0:
            assert call() == E_STATE
            assert "passive" in L.vp_last_error().decode()
            assert L.vp_set_envmap_sampling(volpath.ENV_PASSIVE) == 0
        if L.vp_set_arithmetic(volpath.ARITH_FAST) == 0:
            assert call() == E_STATE
            assert "exact" in L.vp_last_error().decode()
            assert L.vp_set_arithmetic(volpath.ARITH_EXACT) == 0
    finally:
        volpath.set_tracking(volpath.TRACK_SPECTRAL)
        L.vp_enable_counters(0)


def test_refusals_come_before_the_device():
    """VP_E_ARG for NULL and aliased pointers, n_frames <= 0 and first_frame < 0: the pointers are never followed and no device is asked
    for (this machine has none)"""
    import volpath
    L = volpath.lib()
    P = C.byref(volpath.make_param(16, 8))
    a, b, c = (C.c_void_p(v) for v in (0x1000, 0x2000, 0x3000))       # never dereferenced
    f = L.vp_render_frames_group_layers
    for args in ((None, b, c, 0, 2, P), (a, None, c, 0, 2, P), (a, b, None, 0, 2, P), (a, b, c, 0, 2, None), (a, a, c, 0, 2, P), (a, b, a, 0, 2, P),
                 (a, b, b, 0, 2, P), (a, b, c, 0, 0, P), (a, b, c, 0, -3, P), (a, b, c, -1, 2, P)):
        assert f(*args) == E_ARG, args
        assert "vp_render_frames_group_layers" in L.vp_last_error().decode()
    _state_refusals(volpath, lambda: f(a, b, c, 0, 2, P))
    with pytest.raises(volpath.VolpathError, match="vp_render_frames_group_layers"):
        volpath.render_frames_group_layers(a, b, a, 0, 1, volpath.make_param(16, 8))


def test_stats_refusals_come_before_the_device():
    import volpath
    L = volpath.lib()
    P = C.byref(volpath.make_param(16, 8))
    a, b, c, ra, rb, rc = (C.c_void_p(v) for v in (0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000))      # never dereferenced
    f = L.vp_render_frames_group_layers_stats
    ok = [a, b, c, ra, rb, rc, 0, 2, P]
    bad = []
    for i in (0, 1, 2, 3, 4, 5, 8):                          # any NULL pointer
        bad.append(ok[:i] + [None] + ok[i + 1:])
    for i, j in ((0, 1), (0, 2), (1, 2), (3, 4), (3, 5), (4, 5)):      # any two accumulators, any two record buffers equal
        bad.append(ok[:j] + [ok[i]] + ok[j + 1:])
    bad += [ok[:7] + [0, P], ok[:7] + [-3, P], ok[:6] + [-1, 2, P]]
    for args in bad:
        assert f(*args) == E_ARG, args
        assert "vp_render_frames_group_layers_stats" in L.vp_last_error().decode()
    _state_refusals(volpath, lambda: f(*ok))


def test_relight_composite_refuses_bad_arguments():
    import volpath
    L = volpath.lib()
    a, b, c = (C.c_void_p(v) for v in (0x1000, 0x2000, 0x3000))
    one, rgb = (C.c_float * 3)(1.0, 1.0, 1.0), (C.c_float * 3)(0.1, 0.2, 0.3)
    g = L.vp_relight_composite
    ok = [a, a, b, c, one, one, None, rgb, 4, 1.0]
    for i in (0, 1, 2, 3, 4, 5):
        assert g(*(ok[:i] + [None] + ok[i + 1:])) == E_ARG, i
    assert g(*(ok[:7] + [None, 4, 1.0])) == E_ARG and g(*(ok[:8] + [-1, 1.0])) == E_ARG      # both plate pointers NULL; size < 0
    assert "vp_relight_composite" in L.vp_last_error().decode()


def test_census_has_the_layers_set_and_leaves_the_other_tables_alone():
    import volpath
    L = volpath.lib()
    n = L.vp_test_group_layers_census(None, None, 0, 0)
    assert n == L.vp_test_groups_census(None, None, 0, 0) == L.vp_test_launch_census(0, 0, None, None, 0, 0)
    launches, built = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    for wrong in (0, n - 1, n + 1):
        assert L.vp_test_group_layers_census(launches.ctypes.data, built.ctypes.data, wrong, 0) == E_ARG
    assert L.vp_test_group_layers_census(launches.ctypes.data, built.ctypes.data, n, 0) == 0
    assert not launches.any()
    census = volpath.group_layers_census()
    assert set(census) == set(volpath.groups_census()) == set(volpath.launch_census(volpath.CENSUS_EXACT, volpath.CENSUS_LAYERS)) and len(census) == int(built.sum())
    assert L.vp_test_launch_census(0, 3, None, None, 0, 0) == E_ARG          # no fourth kind: the table has a hook of its own


# ---- the output stage
def test_relight_composite_restatement_is_one_rounding_per_operation():
    sun = np.array([[0.3, 7.0, 1e-3, 5.0]], F32)
    sky = np.array([[3.0, 0.25, 2.0, 5.0]], F32)
    tr = np.array([[0.5, 0.25, 0.125, 2.0]], F32)
    s = F32(1.0) / F32(3.0)
    gs, gk, B = np.array([2.0, 0.5, 0.0], F32), np.array([0.1, 1.0, 3.0], F32), np.array([0.7, 0.1, 9.0], F32)
    want = [F32(F32(F32(F32(sun[0, c] * s) * gs[c]) + F32(F32(sky[0, c] * s) * gk[c])) + F32(F32(tr[0, c] * s) * B[c])) for c in range(3)]
    want.append(F32(F32(1.0) - F32(tr[0, 3] * s)))
    assert GLL.relight_composite(sun, sky, tr, s, gs, gk, rgb=B)[0].tolist() == [float(v) for v in want]


@pytest.mark.parametrize("seed", range(4))
def test_relight_composite_restatement_equals_the_three_steps(seed):
    """random inputs over many binades, negative zeros and denormals included, a plate and a constant: the fused form and the sequence
    vp_relight, scale, vp_composite(scale 1) have the same bits (x * 1 is x, -0 and denormals included)"""
    rng = np.random.default_rng(500 + seed)
    n = 4096

    def values():
        v = (rng.standard_normal((n, 4)) * np.exp2(rng.integers(-20, 12, (n, 4)))).astype(F32)
        v[rng.random((n, 4)) < 0.05] = F32(-0.0)
        v[rng.random((n, 4)) < 0.05] = F32(0.0)
        tiny = rng.random((n, 4)) < 0.1
        v[tiny] = (rng.integers(-(1 << 22), 1 << 22, int(tiny.sum())).astype(np.int32)).astype(F32) * F32(2.0 ** -149)       # denormals of either sign
        return v
    sun, sky, tr, plate = values(), values(), values(), values()
    assert (np.abs(sun[sun != 0]) < 2.0 ** -126).any() and np.signbit(sun[sun == 0]).any()
    for s in (F32(1.0), F32(1.0) / F32(3.0), F32(2.0 ** -30)):
        for gs, gk in (((1, 1, 1), (1, 1, 1)), ((2.0, 0.5, 0.0), (-0.0, 1.0, 3.0))):
            for kw in (dict(plate=plate), dict(rgb=(0.7, -0.0, 9.0))):
                got = GLL.relight_composite(sun, sky, tr, s, gs, gk, **kw)
                want = GLL.three_steps(sun, sky, tr, s, gs, gk, **kw)
                assert got.tobytes() == want.tobytes(), (seed, float(s), gs, kw.keys())


# ---- the command line
def test_cli_planes_flags():
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--planes-out PREFIX", "--planes-denoise"):
        assert flag in r.stdout, flag
    r = subprocess.run([EXE, "--planes-out"], capture_output=True, text=True)
    assert r.returncode == 2, (r.stdout, r.stderr)
    r = subprocess.run([EXE, "--planes-denoise"], capture_output=True, text=True)
    assert r.returncode == 2 and "--planes-denoise" in r.stderr and "--planes-out" in r.stderr, r.stderr
    for bad in (["--sun-gain", "1", "2"], ["--over", "1", "x", "3"]):
        r = subprocess.run([EXE, "--planes-out", "x"] + bad, capture_output=True, text=True)
        assert r.returncode == 2, (bad, r.stdout, r.stderr)
    for other in (["--gpus", "2"], ["--noise", "0.05"], ["--denoise"], ["--groups-out", "y"], ["--layers-out", "y"], ["--plane-noise", "0.1", "0.1"]):
        for extra in ([], ["--sun-gain", "2", "0.5", "0"], ["--over", "0.5", "0.5", "0.5"], ["--planes-denoise"]):
            r = subprocess.run([EXE, "--planes-out", "x"] + extra + other, capture_output=True, text=True)
            assert r.returncode == 2 and "--planes-out" in r.stderr and other[0] in r.stderr, (other, extra, r.stderr)
    for other in (["--tracking", "scalar"], ["--tracking", "multichannel"], ["--env", "mis"], ["--arith", "fast", "--rng", "philox", "--estimator", "global"]):
        r = subprocess.run([EXE, "--planes-out", "x"] + other, capture_output=True, text=True)
        assert r.returncode == 2 and "--planes-out" in r.stderr, (other, r.stderr)
    # what was refused before stays refused, with the words it had
    r = subprocess.run([EXE, "--groups-out", "x", "--layers-out", "y"], capture_output=True, text=True)
    assert r.returncode == 2 and "--groups-out" in r.stderr and "--layers-out" in r.stderr and "--planes-out" not in r.stderr, r.stderr


# ---- the expectation against itself
@pytest.mark.parametrize("est", (0, 1), ids=("global", "decomp"))
def test_expectation_groups_are_non_empty_on_julia(oracle, est):
    """non-vacuity of tests/test_group_layers_gpu.py: box-missing pixels, pixels unscattered in every frame, pixels scattered in every
    frame and pixels that are one in one frame and the other in the next"""
    E = GLL.expected(oracle, "julia", est, 1)
    g = E.groups()
    assert min(g.values()) >= 1, g
    assert sum(g.values()) == W * H


@pytest.mark.parametrize("name,est,rng_mode", [(n, e, r) for n in ("julia", "soft") for e in (0, 1, 2) for r in (0, 2)])
def test_the_fold_obeys_the_table_and_adds_up_to_the_layers_foreground(oracle, name, est, rng_mode):
    """Per sample: an unscattered one is (0, 0, 0, w), (0, 0, 0, w) and the layers trans sample; a scattered one the two samples of the
    groups call and a zero trans sample, and its sun + sky stays within groups_lib.ADDITIVITY of the layers fg sample (which is the
    beauty sample there: the bound and its derivation are tests/test_groups_cpu.py's).  The folded accumulators restate the equivalent
    forms: trans is layers_lib's trans accumulator, the three w are the layers fg.w."""
    E = GLL.expected(oracle, name, est, rng_mode)
    u = E.unscattered
    assert u.any() and not u.all()
    for plane in (E.sun, E.sky):
        assert not plane[u][:, :3].any() and np.array_equal(plane[u][:, 3], E.beauty[u][:, 3])
    assert np.array_equal(E.sun[~u], E.gsun[~u]) and np.array_equal(E.sky[~u], E.gsky[~u])
    assert (E.trans[u][:, 3] == 1).all() and not E.trans[~u].any()
    s64, v64 = E.sun[~u][:, :3].astype(np.float64) + E.sky[~u][:, :3].astype(np.float64), E.fg[~u][:, :3].astype(np.float64)
    den = np.maximum(np.abs(v64), np.abs(s64))
    worst = float((np.abs(s64 - v64)[den > 0] / den[den > 0]).max())
    print("worst per-sample additivity error: %.3f * 2^-24" % (worst * 2.0 ** 24))
    assert worst <= GL.ADDITIVITY, worst * 2.0 ** 24
    L = LL.expected(oracle, name, est, rng_mode)
    sun, sky, trans = E.accs()
    assert trans.tobytes() == L.trans.tobytes()
    assert np.array_equal(sun[..., 3], L.fg[..., 3]) and np.array_equal(sky[..., 3], L.fg[..., 3])
    assert np.isfinite(sun).all() and np.isfinite(sky).all() and (sun[..., :3].max() > 0) and (sky[..., :3].max() > 0)
    # the records' fold carries the same accumulators
    st = E.stats()
    assert all(st[k].acc.tobytes() == a.tobytes() for k, a in enumerate((sun, sky, trans)))
    assert all((s.n == len(FRAMES)).all() for s in st)
