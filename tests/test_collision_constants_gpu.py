"""GPU parity for the collision block's tabulated scene constants (render_k's scatter-count table in LDS: the Hyperion-reduced
phase parameter, density, majorant and its reciprocal, one row per distinct value of hyperion_s).

A small Julia scene in a medium thick enough that paths scatter far more than 20 times, rendered over frames 9..12: the table's
clamped rows (scatter counts 0..5 read row 0, counts above 20 the last row) and both sides of the decomposition estimator's
frame-11 switch to the optical-depth table are exercised.  Bar: the accumulator equals the CPU oracle's bit for bit, for the
global-majorant and the decomposition estimator, on Philox2x32-7 (the light estimate's direction is drawn in the collision block)
and on the sequential sampler.h stream (it is drawn after the shadow ray), for three suns: the default one, one with a component
that is exactly zero and one with a tiny component."""
import numpy as np
import pytest

import scenes

pytestmark = pytest.mark.gpu

W, H, N = 24, 16, 32
FIRST, NFRAMES = 9, 4

SUNS = {
    "default": scenes.DEFAULT_SUN_DIR,
    "oblique": (0.48507127, 0.72760689, -0.48507127),
    "zero_component": (0.0, 0.8, -0.6),
    "tiny_component": (1.0e-9, 0.8, -0.6),
}


def _oracle(oracle, grid, env, sun, est, rng_mode, key):
    osc = oracle.OracleScene(grid, env, sun, scenes.DEFAULT_SUN_POWER, estimator=est, rng_mode=rng_mode, seed=key)
    oP = oracle.default_param(W, H)
    if est == oracle.EST_DECOMP:
        osc.precompute_opacity()
    ref, deepest = None, 0.0
    for f in range(FIRST, FIRST + NFRAMES):
        before = 0.0 if ref is None else ref[..., 3].copy()
        ref, _ = osc.render_frame(oP, f, ref)
        deepest = max(deepest, float((ref[..., 3] - before).max()))
    return ref, deepest


@pytest.mark.parametrize("sun", sorted(SUNS))
@pytest.mark.parametrize("rng_mode", [2, 0], ids=["philox7", "samplerh"])
@pytest.mark.parametrize("est", [0, 1], ids=["global", "decomp"])
def test_tabulated_collision_constants_bit_exact(vp, oracle, est, rng_mode, sun):
    grid = oracle.julia(N)
    env = scenes.synthetic_env()
    key = (3, 4)
    ref, deepest = _oracle(oracle, grid, env, SUNS[sun], est, rng_mode, key)
    # the heat channel of one frame: the scatter count (decomposition) or a thousandth of the depth index (global majorant)
    assert deepest > (20.0 if est == oracle.EST_DECOMP else 0.020), f"the scene does not scatter deep enough: {deepest}"
    buf = vp.DeviceBuffer(W, H)
    try:
        vp.init_volume(grid, brick=1, linear=True)
        vp.init_envmap(env)
        vp.set_sun(SUNS[sun], scenes.DEFAULT_SUN_POWER)
        vp.set_camera()
        vp.set_estimator(est)
        vp.set_rng(rng_mode, key)
        vp.set_tracking(0)
        vp.set_envmap_sampling(vp.ENV_PASSIVE)
        vp.set_shard(0, 1)
        vp.enable_counters(False)
        if est == vp.EST_DECOMP:
            vp.precompute_opacity(SUNS[sun])
        vp.render_frames(buf.ptr, FIRST, NFRAMES, vp.make_param(W, H))
        got = buf.download()
    finally:
        buf.free()
    assert np.array_equal(got, ref), f"est={est} rng={rng_mode} sun={sun}: max abs difference {np.abs(got - ref).max()}"
