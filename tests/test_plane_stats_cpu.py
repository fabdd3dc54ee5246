"""Statistics on planes (include/volpath.h vp_render_frames_groups_stats / vp_render_frames_layers_stats) without a
GPU: the declared and exported symbols, the refusals that come before the device, the CLI flags, and the oracle-built expectation of
tests/plane_stats_lib.py checked against itself."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import groups_lib as GL
import layers_lib as LL
import plane_stats_lib as PS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cuda-volpath_amd", "volpath_render")
E_STATE, E_ARG = -2, -3
W, H, FRAMES = PS.W, PS.H, PS.FRAMES
NEW = ("vp_render_frames_groups_stats", "vp_render_frames_layers_stats")


# ---- the interface
def test_symbols_are_declared_exported_and_typed():
    import volpath
    text = open(os.path.join(ROOT, "include", "volpath.h")).read()
    for n in NEW:
        assert n in volpath.PART2_SYMBOLS
        assert re.search(r"\bint\s+%s\s*\(" % n, text), n
        assert hasattr(volpath.lib(), n)
    assert re.search(r"int\s+vp_render_frames_groups_stats\(vp_float4\*\s*d_sun,\s*vp_float4\*\s*d_sky,\s*vp_pixel_stats\*\s*d_sun_stats,"
                     r"\s*vp_pixel_stats\*\s*d_sky_stats,\s*int first_frame,\s*int n_frames,\s*const Param\*\s*p\);", text)
    assert re.search(r"int\s+vp_render_frames_layers_stats\(vp_float4\*\s*d_fg,\s*vp_float4\*\s*d_trans,\s*vp_pixel_stats\*\s*d_fg_stats,"
                     r"\s*vp_pixel_stats\*\s*d_trans_stats,\s*int first_frame,\s*int n_frames,\s*const Param\*\s*p\);", text)
    L = volpath.lib()
    for n in NEW:
        assert getattr(L, n).argtypes == [C.c_void_p] * 4 + [C.c_int, C.c_int, C.POINTER(volpath.Param)]
    assert callable(volpath.render_frames_groups_stats) and callable(volpath.render_frames_layers_stats)
    flat = " ".join(text.split()).replace(" * ", " ")
    for phrase in ("adaptive rounds on planes", "groups combined with layers", "across processes"):      # what is still not built is said
        assert phrase in flat[flat.index("Statistics on planes"):], phrase


@pytest.mark.parametrize("name", NEW)
def test_refusals_come_before_the_device(name):
    """VP_E_ARG for the arguments, VP_E_STATE for the modes the underlying call is not built for: the pointers are never followed and no
    device is asked for (this machine has none)"""
    import volpath
    L = volpath.lib()
    P = C.byref(volpath.make_param(16, 8))
    a, b, ra, rb = (C.c_void_p(v) for v in (0x1000, 0x2000, 0x3000, 0x4000))      # never dereferenced
    f = getattr(L, name)
    for args in ((None, b, ra, rb, 0, 2, P), (a, None, ra, rb, 0, 2, P), (a, b, None, rb, 0, 2, P), (a, b, ra, None, 0, 2, P), (a, b, ra, rb, 0, 2, None),
                 (a, a, ra, rb, 0, 2, P), (a, b, ra, ra, 0, 2, P), (a, b, ra, rb, 0, 0, P), (a, b, ra, rb, 0, -3, P), (a, b, ra, rb, -1, 2, P)):
        assert f(*args) == E_ARG, args
        assert name + ":" in L.vp_last_error().decode()
    try:
        for mode in (volpath.TRACK_SCALAR, volpath.TRACK_MULTI_CHANNEL):
            volpath.set_tracking(mode)
            assert f(a, b, ra, rb, 0, 2, P) == E_STATE
            assert "spectral" in L.vp_last_error().decode() and name + " " in L.vp_last_error().decode()
        volpath.set_tracking(volpath.TRACK_SPECTRAL)
        assert L.vp_enable_counters(1) == 0
        assert f(a, b, ra, rb, 0, 2, P) == E_STATE
        assert "counters" in L.vp_last_error().decode() and name + " " in L.vp_last_error().decode()
        L.vp_enable_counters(0)
        # (the setters of the environment mode and the arithmetic ask for the device themselves: where there is none they fail and the
        # mode stays; tests/test_plane_stats_gpu.py makes both refusals with the four buffers checked)
        if L.vp_set_envmap_sampling(volpath.ENV_MIS) == 0:
            assert f(a, b, ra, rb, 0, 2, P) == E_STATE and "passive" in L.vp_last_error().decode()
            assert L.vp_set_envmap_sampling(volpath.ENV_PASSIVE) == 0
        if L.vp_set_arithmetic(volpath.ARITH_FAST) == 0:
            assert f(a, b, ra, rb, 0, 2, P) == E_STATE and "exact" in L.vp_last_error().decode()
            assert L.vp_set_arithmetic(volpath.ARITH_EXACT) == 0
    finally:
        volpath.set_tracking(volpath.TRACK_SPECTRAL)
        L.vp_enable_counters(0)
    wrapper = getattr(volpath, name[3:])
    with pytest.raises(volpath.VolpathError, match=name):
        wrapper(a, b, ra, ra, 0, 1, volpath.make_param(16, 8))


def test_cli_plane_denoise_flags():
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--groups-denoise", "--layers-denoise"):
        assert flag in r.stdout, flag
    planes = {"--groups-denoise": (["--groups-out", "x"], ["--sun-gain", "2", "0.5", "0"], ["--sky-gain", "0", "1", "3"]),
              "--layers-denoise": (["--layers-out", "x"], ["--over", "0.5", "0.5", "0.5"])}
    for flag, with_planes in planes.items():
        r = subprocess.run([EXE, flag], capture_output=True, text=True)                       # alone: it needs its plane flag
        assert r.returncode == 2 and flag in r.stderr and with_planes[0][0] in r.stderr, (flag, r.stderr)
        other_plane = planes["--layers-denoise" if flag == "--groups-denoise" else "--groups-denoise"][0]
        r = subprocess.run([EXE, flag] + other_plane, capture_output=True, text=True)         # ... its own, not the other's
        assert r.returncode == 2 and flag in r.stderr, (flag, other_plane, r.stderr)
        for plane in with_planes:
            for other in (["--gpus", "2"], ["--noise", "0.05"], ["--denoise"]):
                r = subprocess.run([EXE, flag] + plane + other, capture_output=True, text=True)
                assert r.returncode == 2 and flag in r.stderr and other[0] in r.stderr, (flag, plane, other, r.stderr)
        r = subprocess.run([EXE, flag] + with_planes[0] + ["--denoise-radius", "11"], capture_output=True, text=True)     # the filter's own limits
        assert r.returncode == 2, r.stderr


# ---- the expectation against itself
@pytest.mark.parametrize("name,est", (("soft", 0), ("julia", 1)), ids=("soft-global", "julia-decomp"))
def test_the_expectation_is_self_consistent(oracle, name, est):
    """16 x 12, frames (10, 11): the folded accumulators are groups_lib's and layers_lib's own; every record of every plane holds n == 2;
    a box-missing pixel's sun and fg records stay at 0 (its samples are (0, 0, 0, heat): w never enters a luminance); both ways round,
    some pixel has a trans luminance and no fg luminance and some pixel the reverse"""
    sun, sky = PS.expected(oracle, "groups", name, est, 1)
    fg, tr = PS.expected(oracle, "layers", name, est, 1)
    G, Y = GL.expected(oracle, name, est, 1), LL.expected(oracle, name, est, 1)
    assert sun.acc.tobytes() == G.sun.tobytes() and sky.acc.tobytes() == G.sky.tobytes()
    assert fg.acc.tobytes() == Y.fg.tobytes() and tr.acc.tobytes() == Y.trans.tobytes()
    for s in (sun, sky, fg, tr):
        assert (s.n == len(FRAMES)).all() and not s.flags.any() and np.isfinite(s.sum_y).all() and (s.sum_y >= 0).all() and (s.sum_y2 >= 0).all()
    assert np.array_equal(sun.n, sky.n) and np.array_equal(fg.n, tr.n)
    miss = Y.miss
    assert miss.any() and np.array_equal(miss, G.miss)
    assert not sun.sum_y[miss].any() and not fg.sum_y[miss].any() and not sun.sum_y2[miss].any() and not fg.sum_y2[miss].any()
    assert (sun.n[miss] == 2).all() and (fg.n[miss] == 2).all() and (fg.acc[miss][:, 3] == G.beauty[miss][:, 3]).all()
    assert (sky.sum_y[miss] > 0).all() and (tr.sum_y[miss] > 0).all()                 # ... it sees the sky, with a throughput of 1
    assert ((tr.sum_y > 0) & (fg.sum_y == 0)).any() and ((fg.sum_y > 0) & (tr.sum_y == 0)).any()
    assert ((sun.sum_y > 0) & (sky.sum_y > 0)).any()
    # a pixel whose two frames differ in kind: one scattered, one not -- its trans record holds ONE luminance, squared once
    mixed = Y.unscattered.any(0) & ~Y.unscattered.all(0)
    assert mixed.any()
    assert np.array_equal(tr.sum_y2[mixed], tr.sum_y[mixed] * tr.sum_y[mixed])
