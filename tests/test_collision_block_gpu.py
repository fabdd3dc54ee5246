"""GPU parity for the collision block's trimmed instructions (render_k):

  - the shadow ray's length is the root its direction's normalize takes: one square root, not two;
  - roots and reciprocal roots whose operand is in range by construction (the frame's tangent, the sampled direction, the sine of the
    phase function's polar angle) drop the compiler's range scaling, class test and fix-up (vp_math.h sqrt_inrange_, rsqrt_unit_).

Both are required to change no bit.  (A third change was built and measured with them and is not in the tree: the sun table read at the
cell index of the step's fetch, carried in the lane -- profiles/experiments/r12_collision_block.txt.  The volumes below are where
that index goes wrong -- a ragged grid, control collisions that park a lane without a fetch, point filtering, float cells, the
brick layout -- and stay as the collision block's cases: the development build of that change moved a control collision's point
twice and only the float grid showed it.)  Bar: vp_test_roots finds no mismatch on any bit pattern of the helpers' stated ranges; every
accumulator equals the CPU oracle's bit for bit.  No exclusions, no tolerance."""
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

import scenes
# the scene of the tracking step's tests, and its oracle accumulators (computed once per case, shared, read-only)
from test_tracking_step_gpu import DENSITY, FIRST, G, H, KEY, NFRAMES, SUNS, W, _oracle, _render

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------ 1. the helpers, every bit pattern
def _bits(x):
    return int(np.float32(x).view(np.uint32))


def test_sqrt_inrange_equals_sqrtf_on_its_whole_range(vp):
    """x = 0 and every binary32 in [2^-24, 2]: 25 * 2^23 + 1 patterns"""
    lo, hi = _bits(2.0 ** -24), _bits(2.0)
    assert hi - lo + 1 == 25 * 2 ** 23 + 1
    bad, first = vp.test_roots(0, lo, hi)
    print(f"sqrt_inrange_: {bad} mismatches in [{lo:#x}, {hi:#x}], first {first}")
    assert (bad, first) == (0, None)
    assert vp.test_roots(0, 0, 0) == (0, None)   # +0


def test_rsqrt_unit_equals_one_over_sqrtf_on_its_whole_range(vp):
    """every binary32 in [2^-8, 2]: 9 * 2^23 + 1 patterns"""
    lo, hi = _bits(2.0 ** -8), _bits(2.0)
    assert hi - lo + 1 == 9 * 2 ** 23 + 1
    bad, first = vp.test_roots(1, lo, hi)
    print(f"rsqrt_unit_: {bad} mismatches in [{lo:#x}, {hi:#x}], first {first}")
    assert (bad, first) == (0, None)


def test_roots_hook_refuses_the_fast_mode_and_bad_arguments(vp):
    L = vp.lib()
    import ctypes as C
    m, f = C.c_uint64(0), C.c_uint32(0)
    assert L.vp_test_roots(2, 0, 0, C.byref(m), C.byref(f)) == -3      # VP_E_ARG
    assert L.vp_test_roots(0, 2, 1, C.byref(m), C.byref(f)) == -3
    assert L.vp_test_roots(0, 0, 0, None, C.byref(f)) == -3
    vp.set_arithmetic(vp.ARITH_FAST)
    try:
        with pytest.raises(vp.VolpathError, match="vp_test_roots"):
            vp.test_roots(0, 0, 0)
    finally:
        vp.set_arithmetic(vp.ARITH_EXACT)


# ------------------------------------------------------------------------------------------ 2. the tracking step's scene
@pytest.mark.parametrize("exit_mode", [2, 0], ids=["exit_flights", "no_exit_flights"])
@pytest.mark.parametrize("rng_mode", [2, 0], ids=["philox7", "samplerh"])
@pytest.mark.parametrize("est", [0, 1], ids=["global", "decomp"])
def test_julia_renders_equal_the_oracle(vp, oracle, est, rng_mode, exit_mode):
    """thousands of collisions per pixel (the scatter cap is reached): each starts a shadow ray with the single root and samples its
    next direction with the in-range roots (sampler.h: the reference's order of events, the same roots)"""
    ref, deepest = _oracle(oracle, est, rng_mode, "default", False)
    print(f"est={est} rng={rng_mode}: deepest heat of one frame {deepest!r}")
    assert deepest > (20.0 if est == oracle.EST_DECOMP else 0.020), f"the scene does not scatter deep enough: {deepest}"
    got = _render(vp, oracle, est, rng_mode, "default", False, exit_mode if rng_mode == 2 else min(exit_mode, 1))
    assert np.array_equal(got, ref), f"est={est} rng={rng_mode} exit={exit_mode}: max abs difference {np.abs(got - ref).max()}"


@pytest.mark.parametrize("est", [0, 1], ids=["global", "decomp"])
def test_julia_chromatic_preset_equals_the_oracle(vp, oracle, est):
    ref, _ = _oracle(oracle, est, 2, "default", True)
    got = _render(vp, oracle, est, 2, "default", True, 2)
    assert np.array_equal(got, ref), f"est={est}: max abs difference {np.abs(got - ref).max()}"


@pytest.mark.parametrize("sun", list(SUNS))
@pytest.mark.parametrize("est", [0, 1], ids=["global", "decomp"])
def test_julia_suns_equal_the_oracle(vp, oracle, est, sun):
    """a zero and a 1e-9 component: shadow rays that miss or graze the box, lengths of 1e10 whatever the direction"""
    ref, _ = _oracle(oracle, est, 2, sun, False)
    got = _render(vp, oracle, est, 2, sun, False, 2)
    assert np.array_equal(got, ref), f"est={est} sun={sun}: max abs difference {np.abs(got - ref).max()}"


# ------------------------------------------------------------------------------------------ 3. two more volumes
# the default camera's orientation from a point inside both boxes (11 x 13 x 17: |y| <= 13/17, |z| <= 11/17)
CAM_INSIDE = (0.0, 0.207912, 0.978148, 0.3, 0.0, 0.978148, -0.207912, -0.1, -1.0, 0.0, 0.0, 0.03)
SUN = "oblique"


def _ragged():
    """sparse random uchar grid with three different extents: a wrong stride at the sun table reads another cell's clip distance"""
    rng = np.random.default_rng(29)
    grid = rng.integers(0, 256, (11, 13, 17), dtype=np.uint8)
    grid[rng.random(grid.shape) < 0.3] = 0
    return grid


def _rimmed():
    """16^3 of 255 inside a one-voxel empty rim: the interior bricks have a positive minimum, so the decomposition estimator makes
    control collisions -- lanes that park at distc, where the step fetched nothing"""
    grid = np.zeros((16, 16, 16), np.uint8)
    grid[1:-1, 1:-1, 1:-1] = 255
    return grid


VOLUMES = {"ragged_11x13x17": _ragged, "rimmed_16": _rimmed, "ragged_float": lambda: _ragged().astype(np.float32) * np.float32(1.0 / 255.0)}
_VREFS = {}


def _volume_oracle(oracle, volume, est, cam, linear):
    k = (volume, est, cam, linear)
    if k not in _VREFS:
        osc = oracle.OracleScene(VOLUMES[volume](), scenes.synthetic_env(), SUNS[SUN], scenes.DEFAULT_SUN_POWER, linear=linear, estimator=est,
                                 rng_mode=2, seed=KEY, inv_view=None if cam == "outside" else np.array(CAM_INSIDE, np.float32))
        oP = oracle.default_param(W, H, density=DENSITY, g=G)
        if est == oracle.EST_DECOMP:
            osc.precompute_opacity()
        ref = None
        for f in range(FIRST, FIRST + NFRAMES):
            ref, _ = osc.render_frame(oP, f, ref)
        ref.setflags(write=False)
        _VREFS[k] = ref
    return _VREFS[k]


def volume_render(vp, scenes, grid, est, cam, linear, sun, key, first, nframes, w, h, density, g):
    vP = vp.make_param(w, h, density=density, g=g)
    buf = vp.DeviceBuffer(w, h)
    try:
        vp.init_volume(grid, brick=1, linear=linear)
        vp.init_envmap(scenes.synthetic_env())
        vp.set_sun(sun, scenes.DEFAULT_SUN_POWER)
        if cam is None:
            vp.set_camera()
        else:
            vp.set_camera(cam)
        vp.set_estimator(est)
        vp.set_rng(2, key)
        vp.set_tracking(0)
        vp.set_envmap_sampling(vp.ENV_PASSIVE)
        vp.set_shard(0, 1)
        vp.enable_counters(False)
        vp.set_exit_flights(2)
        if est == vp.EST_DECOMP:
            vp.precompute_opacity(sun)
        vp.render_frames(buf.ptr, first, nframes, vP)
        return buf.download()
    finally:
        vp.set_exit_flights(1)
        vp.set_camera()
        buf.free()


def _volume_render(vp, volume, est, cam, linear):
    return volume_render(vp, scenes, VOLUMES[volume](), est, None if cam == "outside" else CAM_INSIDE, linear, SUNS[SUN], KEY, FIRST, NFRAMES,
                         W, H, DENSITY, G)


@pytest.mark.parametrize("linear", [True, False], ids=["linear", "point"])
@pytest.mark.parametrize("cam", ["outside", "inside"])
@pytest.mark.parametrize("est", [0, 1], ids=["global", "decomp"])
@pytest.mark.parametrize("volume", ["ragged_11x13x17", "rimmed_16"])
def test_volume_renders_equal_the_oracle(vp, oracle, volume, est, cam, linear):
    ref = _volume_oracle(oracle, volume, est, cam, linear)
    print(f"{volume} est={est} cam={cam} linear={linear}: largest heat {float(ref[..., 3].max())!r}")
    assert ref[..., 3].max() > 0.0, "no path collides in this view"
    got = _volume_render(vp, volume, est, cam, linear)
    assert np.array_equal(got, ref), f"max abs difference {np.abs(got - ref).max()}"


@pytest.mark.parametrize("est", [0, 1], ids=["global", "decomp"])
def test_float_volume_render_equals_the_oracle(vp, oracle, est):
    """float cells split their axes with axis_linear_f32; the sun table's cell is found with the uchar split, as it always was"""
    ref = _volume_oracle(oracle, "ragged_float", est, "outside", True)
    assert ref[..., 3].max() > 0.0, "no path collides in this view"
    got = _volume_render(vp, "ragged_float", est, "outside", True)
    assert np.array_equal(got, ref), f"max abs difference {np.abs(got - ref).max()}"


# ------------------------------------------------------------------------------------------ 4. the brick layout
def test_brick_layout_render_equals_the_oracle(oracle, tmp_path):
    """VP_CELL_BRICKS=1 (read when the context is made: a fresh child process): the fetch's index is a brick-order one, the sun table
    stays x fastest"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    grid_file, out_file = str(tmp_path / "grid.npy"), str(tmp_path / "out.npy")
    np.save(grid_file, _ragged())
    code = "import sys, numpy as np\nsys.path.insert(0, %r); sys.path.insert(0, %r)\nimport volpath as vp, scenes\n" % (
        os.path.join(root, "cuda-volpath_amd"), os.path.join(root, "tests"))
    code += inspect.getsource(volume_render)   # the child runs the same function
    code += "vp.set_device(0)\nnp.save(%r, volume_render(vp, scenes, np.load(%r), 0, None, True, %r, %r, %d, %d, %d, %d, %r, %r))\n" % (
        out_file, grid_file, tuple(SUNS[SUN]), KEY, FIRST, NFRAMES, W, H, DENSITY, G)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, VP_CELL_BRICKS="1"), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    ref = _volume_oracle(oracle, "ragged_11x13x17", 0, "outside", True)
    got = np.load(out_file)
    assert np.array_equal(got, ref), f"max abs difference {np.abs(got - ref).max()}"
