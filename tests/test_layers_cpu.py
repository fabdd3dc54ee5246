"""Compositing layers (include/volpath.h vp_render_frames_layers / vp_composite) without a GPU: the declared and
exported symbols and their ctypes signatures, the refusals that come before the device, the CLI flags, and the oracle-built expectation
of tests/layers_lib.py checked against itself -- including that the scenes of tests/test_layers_gpu.py reach every kind of pixel."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import layers_lib as LL
import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cuda-volpath_amd", "volpath_render")
E_STATE, E_ARG = -2, -3
F32 = np.float32

W, H, FRAMES, ENV, KEY, JULIA_KW = LL.W, LL.H, LL.FRAMES, LL.ENV, LL.KEY, LL.JULIA_KW
expected = LL.expected


# ---- the interface
def test_symbols_are_declared_exported_and_typed():
    import volpath
    text = open(os.path.join(ROOT, "include", "volpath.h")).read()
    for n in ("vp_render_frames_layers", "vp_composite"):
        assert n in volpath.PART2_SYMBOLS
        assert re.search(r"\bint\s+%s\s*\(" % n, text), n
        assert hasattr(volpath.lib(), n)
    assert re.search(r"int\s+vp_render_frames_layers\(vp_float4\*\s*d_fg,\s*vp_float4\*\s*d_trans,\s*int first_frame,\s*int n_frames,\s*const Param\*\s*p\);", text)
    assert re.search(r"int\s+vp_composite\(vp_float4\*\s*dst,\s*const vp_float4\*\s*fg,\s*const vp_float4\*\s*trans,\s*const vp_float4\*\s*plate,"
                     r"\s*const float plate_rgb\[3\],\s*int size,\s*float scale\);", text)
    L = volpath.lib()
    assert L.vp_render_frames_layers.argtypes == [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(volpath.Param)]
    assert L.vp_composite.argtypes == [C.c_void_p] * 4 + [C.POINTER(C.c_float), C.c_int, C.c_float]
    assert callable(volpath.render_frames_layers) and callable(volpath.composite)


def test_refusals_come_before_the_device():
    """VP_E_ARG for the arguments, VP_E_STATE for the modes the switch is not built for: the pointers are never followed and no device
    is asked for (this machine has none)"""
    import volpath
    L = volpath.lib()
    P = volpath.make_param(16, 8)
    fg, tr = C.c_void_p(0x1000), C.c_void_p(0x2000)       # never dereferenced
    f = L.vp_render_frames_layers
    assert f(None, tr, 0, 2, C.byref(P)) == E_ARG and f(fg, None, 0, 2, C.byref(P)) == E_ARG and f(fg, fg, 0, 2, C.byref(P)) == E_ARG
    assert f(fg, tr, 0, 2, None) == E_ARG and f(fg, tr, 0, 0, C.byref(P)) == E_ARG and f(fg, tr, -1, 2, C.byref(P)) == E_ARG
    assert "vp_render_frames_layers" in L.vp_last_error().decode()
    try:
        for mode in (volpath.TRACK_SCALAR, volpath.TRACK_MULTI_CHANNEL):
            volpath.set_tracking(mode)
            assert f(fg, tr, 0, 2, C.byref(P)) == E_STATE
            assert "spectral" in L.vp_last_error().decode()
        volpath.set_tracking(volpath.TRACK_SPECTRAL)
        assert L.vp_enable_counters(1) == 0
        assert f(fg, tr, 0, 2, C.byref(P)) == E_STATE
        assert "counters" in L.vp_last_error().decode()
    finally:
        volpath.set_tracking(volpath.TRACK_SPECTRAL)
        L.vp_enable_counters(0)
    with pytest.raises(volpath.VolpathError, match="vp_render_frames_layers"):
        volpath.render_frames_layers(fg, fg, 0, 1, P)
    g = L.vp_composite
    rgb = (C.c_float * 3)(0.1, 0.2, 0.3)
    assert g(None, fg, tr, None, rgb, 4, 1.0) == E_ARG and g(fg, None, tr, None, rgb, 4, 1.0) == E_ARG and g(fg, fg, None, None, rgb, 4, 1.0) == E_ARG
    assert g(fg, fg, tr, None, None, 4, 1.0) == E_ARG and g(fg, fg, tr, None, rgb, -1, 1.0) == E_ARG


def test_cli_layer_flags():
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--layers-out PREFIX", "--over R G B"):
        assert flag in r.stdout, flag
    for bad in (["--layers-out"], ["--over", "1", "2"], ["--over", "1", "x", "3"], ["--over", "1", "2", "nan"]):
        r = subprocess.run([EXE] + bad, capture_output=True, text=True)
        assert r.returncode == 2, (bad, r.stdout, r.stderr)
    for layer in (["--layers-out", "x"], ["--over", "0.5", "0.5", "0.5"]):
        for other in (["--gpus", "2"], ["--noise", "0.05"], ["--denoise"]):
            r = subprocess.run([EXE] + layer + other, capture_output=True, text=True)
            assert r.returncode == 2 and layer[0].split()[0] in r.stderr and other[0] in r.stderr, (layer, other, r.stderr)
        for other in (["--tracking", "scalar"], ["--env", "mis"], ["--arith", "fast", "--rng", "philox", "--estimator", "global"]):
            r = subprocess.run([EXE] + layer + other, capture_output=True, text=True)
            assert r.returncode == 2, (layer, other, r.stderr)


def test_composite_restatement_is_one_multiply_and_one_add_per_term():
    fg = np.array([[0.3, 7.0, 1e-3, 5.0]], F32)
    tr = np.array([[3.0, 0.25, 2.0, 3.0]], F32)
    s = F32(1.0) / F32(3.0)
    B = np.array([0.7, 0.1, 9.0], F32)
    want = [F32(F32(fg[0, c] * s) + F32(F32(tr[0, c] * s) * B[c])) for c in range(3)] + [F32(F32(1.0) - F32(tr[0, 3] * s))]
    assert LL.composite(fg, tr, s, rgb=B)[0].tolist() == [float(v) for v in want]
    plate = np.array([[0.7, 0.1, 9.0, 123.0]], F32)
    assert LL.composite(fg, tr, s, plate=plate).tobytes() == LL.composite(fg, tr, s, rgb=B).tobytes()


# ---- the expectation against itself
@pytest.mark.parametrize("est", (0, 1), ids=("global", "decomp"))
def test_expectation_is_self_consistent_on_julia(oracle, est):
    E = expected(oracle, "julia", est, 1)
    real, twin = LL.scenes_for(oracle, oracle.julia(32), ENV, scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER, estimator=est, rng_mode=1, seed=KEY)
    if est == 1:
        real.precompute_opacity()
        twin.precompute_opacity()
    P = oracle.default_param(W, H, **JULIA_KW)
    b = F32(P.brightness)
    checked = 0
    for n, f in enumerate(FRAMES):
        for y in range(H):
            for x in range(W):
                fg, tr, v, cnt = LL.sample(oracle, real, twin, P, x, y, f)
                # unscattered <=> the heat channel is 0 (these two estimators count scatters, or loop indices, in it)
                assert (cnt.scatters == 0) == (v[3] == 0.0) == bool(E.unscattered[n, y, x]), (est, x, y, f)
                assert fg[3] == v[3]
                if cnt.scatters:
                    assert not tr.any() and np.array_equal(fg, v)
                    continue
                assert tr[3] == 1.0 and not fg[:3].any()
                if np.isfinite(tr[:3]).all() and (tr[:3] >= 0).all():
                    # the real scene's sample is thr x background x brightness, one multiply each (0 + x is x for x >= 0)
                    bg = LL.background(oracle, real, LL.camera_dir(list(real.S.inv_view), W, H, x, y))
                    assert np.array_equal(v[:3], np.maximum((tr[:3] * bg) * b, F32(0.0))), (est, x, y, f, v, tr, bg)
                    checked += 1
    assert checked > W * H                     # more than half of the samples are of that kind
    # fg.w is the beauty w bit for bit; fg + trans o (background x brightness) is the beauty image only up to rounding -- not asserted
    assert np.array_equal(E.fg[..., 3], E.beauty[..., 3])
    assert np.array_equal(E.trans[..., 3], E.unscattered.sum(0).astype(F32))


@pytest.mark.parametrize("name,est", (("julia", 0), ("julia", 1), ("soft", 0), ("soft", 1), ("soft", 2)))
def test_the_scenes_reach_every_kind_of_pixel(oracle, name, est):
    """non-vacuity of tests/test_layers_gpu.py: box-missing pixels, pixels unscattered in every frame, pixels scattered in every frame
    and pixels that are one in one frame and the other in the next"""
    E = expected(oracle, name, est, 1)
    g = E.groups()
    assert min(g.values()) >= 1, g
    assert sum(g.values()) == W * H
    tr = E.trans[E.unscattered.any(0) & ~E.miss]
    if name == "soft":
        assert len(np.unique(tr[:, :3])) > 20 and (tr[:, 0] != tr[:, 2]).any()     # chromatic: thr is not 1, and differs by channel
    assert (E.trans[E.miss] == F32(len(FRAMES))).all() and not E.fg[E.miss][:, :3].any()
