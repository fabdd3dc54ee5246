"""The feature pass (include/volpath.h vp_render_features) without a GPU: the ABI, the refusals that come back before the device is
touched, and the numpy restatement (tests/features_lib.py) against float64 closed forms on a homogeneous grid.

The refusal of a step that takes more than VP_FEATURE_MAX_STEPS steps across the box diagonal needs the volume's box, and a volume
needs a device: it is checked in tests/test_features_gpu.py (before it, a context without a volume answers VP_E_STATE)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import features_lib as FL
import oracle_lib as O
import scenes
import volpath as vp

VP_E_ARG, VP_E_STATE = -3, -2
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "volpath.h")


def test_error_codes_are_the_headers():
    src = open(HEADER).read()
    assert re.search(r"VP_E_ARG\s*=\s*-3\b", src) and re.search(r"VP_E_STATE\s*=\s*-2\b", src)


def test_symbol_struct_and_macros():
    L = vp.lib()
    assert hasattr(L, "vp_render_features") and "vp_render_features" in vp.PART2_SYMBOLS
    assert C.sizeof(vp.FeatureParams) == 8
    assert [n for n, _ in vp.FeatureParams._fields_] == ["step", "tau_z"]
    src = open(HEADER).read()
    assert re.search(r"typedef struct \{ float step, tau_z; \} vp_feature_params;", src)
    m = re.search(r"#define VP_FEATURE_TAU_Z_DEFAULT\s+([0-9.]+)f", src)
    assert m and np.float32(m.group(1)) == np.float32(vp.FEATURE_TAU_Z_DEFAULT) == np.float32(math.log(2.0)) == FL.TAU_Z_DEFAULT
    assert re.search(r"#define VP_FEATURE_MAX_STEPS\s+\(1u << 20\)", src) and vp.FEATURE_MAX_STEPS == 1 << 20 == FL.MAX_STEPS
    assert re.search(r"int vp_render_features\(vp_float4\* d_alpha, vp_float4\* d_depth, const Param\* p, const vp_feature_params\* fp\);", src)


def _call(alpha, depth, P, fp):
    return vp.lib().vp_render_features(alpha, depth, C.byref(P) if P is not None else None, C.byref(fp) if fp is not None else None)


# two addresses that are never dereferenced: every case below is refused from the arguments and the host's state alone
A, B = C.c_void_p(0x1000), C.c_void_p(0x2000)
GOOD = dict(step=0.01, tau_z=0.7)
INF, NAN = float("inf"), float("nan")


@pytest.mark.parametrize("name,args", [
    ("alpha NULL", lambda P, fp: (None, B, P, fp)),
    ("depth NULL", lambda P, fp: (A, None, P, fp)),
    ("Param NULL", lambda P, fp: (A, B, None, fp)),
    ("params NULL", lambda P, fp: (A, B, P, None)),
    ("one buffer", lambda P, fp: (A, A, P, fp)),
])
def test_refuses_pointers_before_the_device(name, args):
    assert _call(*args(vp.make_param(24, 16), vp.FeatureParams(**GOOD))) == VP_E_ARG, name
    assert b"vp_render_features" in vp.lib().vp_last_error()


@pytest.mark.parametrize("field", ["step", "tau_z"])
@pytest.mark.parametrize("value", [0.0, -0.0, -0.01, INF, -INF, NAN])
def test_refuses_step_and_tau_z_before_the_device(field, value):
    kw = dict(GOOD)
    kw[field] = value
    assert _call(A, B, vp.make_param(24, 16), vp.FeatureParams(**kw)) == VP_E_ARG
    assert field.encode() in vp.lib().vp_last_error()


@pytest.mark.parametrize("w,h", [(0, 16), (24, 0), (0, 0)])
def test_refuses_an_empty_image_before_the_device(w, h):
    assert _call(A, B, vp.make_param(w, h), vp.FeatureParams(**GOOD)) == VP_E_ARG


def test_no_volume_is_a_state_error_before_the_device():
    """good arguments, a context that never saw a volume: VP_E_STATE, still without a device (this machine has none)"""
    assert _call(A, B, vp.make_param(24, 16), vp.FeatureParams(**GOOD)) == VP_E_STATE
    assert b"volume" in vp.lib().vp_last_error()


# ---- the restatement against float64 closed forms: a grid of all 255 fetches exactly 1.0f everywhere, so a ray's sum is its step count
@pytest.fixture(scope="module")
def homogeneous():
    grid = np.full((8, 8, 8), 255, np.uint8)
    osc = O.OracleScene(grid, scenes.synthetic_env(), scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER, linear=True)
    W, H, step, density, sigma_t = 12, 8, 0.01, 3.0, (1.0, 0.5, 0.25)
    out = FL.features(O, osc, W, H, step, density, sigma_t)
    return osc, W, H, step, density, sigma_t, out


def test_restatement_counts_the_steps_of_a_homogeneous_chord(homogeneous):
    osc, W, H, step, density, sigma_t, (alpha, depth, steps) = homogeneous
    _, _, hit, tn, tf = FL.box_tests(O, osc, W, H)
    assert hit.any() and not hit.all()
    f32 = np.float32
    for y, x in zip(*np.nonzero(hit)):
        n = int(steps[y, x])
        assert n > 0
        # the sum of n ones is exact (n < 2^24), so tau is two float32 products of n
        assert alpha[y, x, 3] == f32(f32(f32(n) * f32(step)) * f32(density))
        # midpoint rule on a chord of length L = tf - max(tn, 0): n = the k with tn + (k + 0.5) step < tf, within one step of L / step
        L = float(tf[y, x]) - max(float(tn[y, x]), 0.0)
        assert abs(n * float(f32(step)) - L) <= float(f32(step)), (n, L)
        # the opacity against float64: expf_ within 1.5 ulp (test_helpers_gpu.py), its argument and the subtraction round once each
        tau = float(alpha[y, x, 3])
        for c in range(3):
            want = -math.expm1(-tau * float(f32(sigma_t[c])))
            assert abs(float(alpha[y, x, c]) - want) <= 3 * 2.0 ** -24, (alpha[y, x, c], want)
        # matter everywhere: first depth = the first sample, last depth = the last, the surface depth where tau_lum reaches ln 2
        zf, zt, zb, cover = (float(v) for v in depth[y, x])
        t0 = max(float(tn[y, x]), 0.0)
        assert cover == 1.0 and abs(zf - (t0 + 0.5 * step)) < 1e-5 and abs(zb - (t0 + (n - 0.5) * step)) < 1e-5
        sy = 0.2126 * sigma_t[0] + 0.7152 * sigma_t[1] + 0.0722 * sigma_t[2]
        k_reach = math.ceil(math.log(2.0) / (step * density * sy) - 1e-6)
        if k_reach <= n:
            assert abs(zt - (t0 + (k_reach - 0.5) * step)) <= step * 1.001 and zf <= zt <= zb
        else:
            assert zt == np.inf


def test_restatement_writes_the_miss_constant(homogeneous):
    osc, W, H, *_, (alpha, depth, steps) = homogeneous
    _, _, hit, _, _ = FL.box_tests(O, osc, W, H)
    assert (alpha[~hit] == 0).all() and (steps[~hit] == 0).all()
    assert np.array_equal(depth[~hit], np.broadcast_to(np.array([np.inf, np.inf, np.inf, 0], np.float32), depth[~hit].shape))


# ---- the CLI's flags (no device: --help and the argument checks come first)
EXE = os.path.join(os.path.dirname(HEADER), "..", "cuda-volpath_amd", "volpath_render")


def test_cli_documents_and_checks_the_flags():
    import subprocess
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for word in ("--features-out PREFIX", "--feature-step DT", "--depth-tau TAU", "PREFIX_alpha.hdr", "PREFIX_depth.hdr", "written as 0"):
        assert word in r.stdout, word
    for bad in (["--feature-step", "0"], ["--feature-step", "-1"], ["--feature-step", "inf"], ["--feature-step", "x"], ["--depth-tau", "0"],
                ["--depth-tau", "nan"], ["--features-out"], ["--feature-step"]):
        r = subprocess.run([EXE] + bad, capture_output=True, text=True)
        assert r.returncode == 2, (bad, r.returncode)
