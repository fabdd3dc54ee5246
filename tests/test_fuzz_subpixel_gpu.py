"""GPU parity of the sub-pixel mode, randomised: the seeded random scenes of tests/scenes.py -- volume, box, camera (outside,
inside, looking away), medium, estimator, stream, filter, brick size, tracking and environment builds, first frame -- with a random
sub-pixel factor, rendered batched and frame by frame (sharded) by the HIP path and compared with the gather of the CPU oracle's
renders of the fine image (tests/subpixel_lib.py).  Bar: bit-exact accumulators (tolerance 0).  VP_FUZZ_SUBPIXEL_SEEDS raises the
number of scenes."""
import os

import numpy as np
import pytest

import scenes
import subpixel_lib as sub

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", range(int(os.environ.get("VP_FUZZ_SUBPIXEL_SEEDS", "16"))))
def test_random_scene_with_a_subpixel_factor_bit_exact(vp, oracle, seed):
    from volpath import host
    c = scenes.random_case(9000 + seed, host)
    rng = np.random.default_rng(31000 + seed)
    s = int(rng.choice([2, 4, 8]))
    W, H = 3 + c["W"] % 14, 3 + c["H"] % 10          # small images: the oracle renders s * s times as many pixels
    grid, box, est, rng_mode, linear, brick, kw = (c[k] for k in ("grid", "box", "est", "rng_mode", "linear", "brick", "kw"))
    first, nframes, late = c["first"], c["nframes"], c["late"]
    osc = oracle.OracleScene(grid, c["env"], c["sun_dir"], c["sun_power"], box=box, brick=brick, linear=linear, estimator=est, rng_mode=rng_mode,
                             seed=c["key"], inv_view=c["cam"], env_mis=c["env_mis"], track_mode=c["track"])
    if late:
        osc.precompute_opacity()
    want = sub.oracle_expectation(vp, osc, oracle.default_param(W, H, **kw), s, first, nframes)
    assert oracle.lib().vpo_debug_shadow_overflow() == 0
    what = dict(seed=seed, s=s, grid=grid.shape, dtype=str(grid.dtype), box=box, est=est, rng=rng_mode, linear=linear, brick=brick, size=(W, H),
                first=first, nframes=nframes, env_mis=c["env_mis"], track=c["track"], world=c["world"], **kw)
    vP = vp.make_param(W, H, **kw)
    buf = vp.DeviceBuffer(W, H)
    try:
        vp.set_subpixel(1)
        vp.init_volume(grid, box=box, brick=brick, linear=linear)
        vp.init_envmap(c["env"])
        vp.set_sun(c["sun_dir"], c["sun_power"])
        vp.set_camera(c["cam"])
        vp.set_estimator(est)
        vp.set_rng(rng_mode, c["key"])
        vp.set_tracking(c["track"])
        vp.set_envmap_sampling(vp.ENV_MIS if c["env_mis"] else vp.ENV_PASSIVE)
        vp.set_shard(0, 1)
        vp.set_exit_flights(seed % 3)
        if late:
            vp.precompute_opacity(c["sun_dir"])
        vp.set_subpixel(s)
        vp.render_frames(buf.ptr, first, nframes, vP)                # batched: one staged launch
        got = buf.download()
        assert np.array_equal(got, want, equal_nan=True), (what, float(np.nanmax(np.abs(got - want))))
        # frame by frame through the reference's entry point, the image as the sum of the shards of `world` ranks
        buf.reset()
        for r in range(c["world"]):
            vp.set_shard(r, c["world"])
            for f in range(first, first + nframes):
                vp.render_kernel(buf.ptr, f, vP)
        assert np.array_equal(buf.download(), want, equal_nan=True), what
    finally:
        vp.set_subpixel(1)
        vp.set_shard(0, 1)
        vp.set_exit_flights(1)
        vp.set_tracking(0)
        vp.set_envmap_sampling(0)
        vp.set_camera()
        buf.free()
