"""GPU parity of adaptive sampling, randomised: the seeded random scenes of tests/scenes.py -- volume, box, camera (outside, inside,
looking away), medium, estimator, stream, filter, brick size, tracking and environment builds, first frame -- rendered adaptively with
random round sizes, minimum frame counts and tolerances, whole and as the shards of `world` ranks, and compared with the numpy
restatement of the definition (tests/adaptive_lib.py) fed with the library's own per-frame renders.  Bar: bit-exact accumulators,
counts, flags and float64 sums (tolerance 0).  VP_FUZZ_ADAPTIVE_SEEDS raises the number of scenes."""
import os

import numpy as np
import pytest

import adaptive_lib as A
import scenes

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", range(int(os.environ.get("VP_FUZZ_ADAPTIVE_SEEDS", "16"))))
def test_random_scene_adaptive_bit_exact(vp, seed):
    from volpath import host
    c = scenes.random_case(17000 + seed, host)
    rng = np.random.default_rng(53000 + seed)
    W, H = c["W"], c["H"]
    grid, box, est, rng_mode, linear, brick, kw = (c[k] for k in ("grid", "box", "est", "rng_mode", "linear", "brick", "kw"))
    first = c["first"]
    max_frames = int(rng.integers(6, 15))
    args = dict(rel_tol=float(rng.choice([0.02, 0.1, 0.3, 1.0])), floor_y=float(rng.choice([0.0, 1e-3, 0.5])), min_frames=int(rng.integers(2, 7)),
                round_frames=int(rng.choice([1, 2, 3, 5])))
    split = int(rng.integers(1, max_frames))          # a resumed call, too
    what = dict(seed=seed, grid=grid.shape, dtype=str(grid.dtype), box=box, est=est, rng=rng_mode, linear=linear, brick=brick, size=(W, H), first=first,
                max_frames=max_frames, split=split, env_mis=c["env_mis"], track=c["track"], world=c["world"], **kw, **args)
    P = vp.make_param(W, H, **kw)
    buf, stats = vp.DeviceBuffer(W, H), vp.StatsBuffer(W, H)
    fbuf = None
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
        if est == vp.EST_DECOMP and first + max_frames - 1 > 10:
            vp.precompute_opacity(c["sun_dir"])
        frame, fbuf = A.library_frames(vp, P)
        want = A.Stats(W, H)
        wres = [A.render_adaptive(want, frame, first, split, **args), A.render_adaptive(want, frame, first + split, max_frames - split, **args)]
        # whole
        res = [vp.render_adaptive(buf.ptr, stats.ptr, first, split, P, **args),
               vp.render_adaptive(buf.ptr, stats.ptr, first + split, max_frames - split, P, **args)]
        diff = A.same_state(want, buf.download(), stats.download())
        assert diff is None, (what, diff)
        assert res == wres, what
        # sharded: every rank its own pixels of the same two buffers
        buf.reset(); stats.reset()
        samples = [0, 0]
        for r in range(c["world"]):
            vp.set_shard(r, c["world"])
            samples[0] += vp.render_adaptive(buf.ptr, stats.ptr, first, split, P, **args)["samples"]
        for r in range(c["world"]):
            vp.set_shard(r, c["world"])
            samples[1] += vp.render_adaptive(buf.ptr, stats.ptr, first + split, max_frames - split, P, **args)["samples"]
        diff = A.same_state(want, buf.download(), stats.download())
        assert diff is None, (what, "sharded", diff)
        assert samples == [wres[0]["samples"], wres[1]["samples"]], what
    finally:
        vp.set_subpixel(1)
        vp.set_shard(0, 1)
        vp.set_exit_flights(1)
        vp.set_tracking(0)
        vp.set_envmap_sampling(0)
        vp.set_camera()
        buf.free(); stats.free()
        if fbuf:
            fbuf.free()
