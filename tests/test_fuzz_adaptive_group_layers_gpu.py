"""Adaptive sampling on group layers on the GPU, randomised (include/volpath.h vp_render_adaptive_group_layers):
the short cases of tests/planes_fuzz_lib.py -- ragged uchar, float and binary16 grids, user boxes, cameras outside, inside and looking
away, both filters, bricks 1 to 8, the three estimators and streams, late first frames, the exit-flight modes -- keep every plane sample
of every frame, from the CPU oracle alone; group_layers_lib.of_frames folds them into the three planes.  For each case the adaptive call
runs with parameters drawn from the seed (rel_tol of each plane from {0.1, 0.3, 1.0}, min_frames 2..4, round_frames 1..3, max_frames
the case's frames) and is held against the restatement of tests/adaptive_group_layers_lib.py fed by the kept samples.

Bar: tolerance 0 -- accumulators, sum_y and sum_y2 by their bits, n and flags by value, the result struct field by field.  The
admission rule is planes_fuzz_lib's own and nothing else, and a case it does not admit is skipped with its reason (of the default list:
seeds 7 and 25; tests/test_fuzz_planes_cpu.py holds the cap on how many may be).

VP_FUZZ_PLANES_SEEDS sets the number of seeds (default 32)."""
import os

import numpy as np
import pytest

import adaptive_group_layers_lib as AG
import group_layers_lib as GLL
import planes_fuzz_lib as PF

pytestmark = pytest.mark.gpu

TOLS = (0.1, 0.3, 1.0)


def params(seed):
    """the adaptive parameters of a case, from its seed"""
    rng = np.random.default_rng(53000 + seed)
    return dict(rel_tol=tuple(float(rng.choice(TOLS)) for _ in range(3)), floor_y=(1e-3, 1e-3, 1e-2), min_frames=int(rng.integers(2, 5)),
                round_frames=int(rng.integers(1, 4)))


def _set_scene(vp, c):
    """as tests/test_fuzz_planes_gpu.py sets it"""
    vp.init_volume(c["grid"], box=c["box"], brick=c["brick"], linear=c["linear"])
    vp.init_envmap(c["env"])
    vp.set_sun(c["sun_dir"], c["sun_power"])
    vp.set_camera(c["cam"])
    vp.set_estimator(c["est"])
    vp.set_rng(c["rng_mode"], c["key"])
    vp.set_tracking(vp.TRACK_SPECTRAL)
    vp.set_envmap_sampling(vp.ENV_PASSIVE)
    vp.set_shard(0, 1)
    vp.set_exit_flights(c["seed"] % 3)
    if c["late"]:
        vp.precompute_opacity(c["sun_dir"])


@pytest.mark.parametrize("seed", range(int(os.environ.get("VP_FUZZ_PLANES_SEEDS", str(PF.SHORT_SEEDS)))))
def test_random_scene_adaptive_group_layers_bit_exact(vp, oracle, seed):
    c, E = PF.expectation(oracle, False, seed)
    why = PF.admissible(E)
    if why is not None:
        pytest.skip("seed %d: the header's equivalent forms do not define this case: %s" % (seed, why))
    Wc, Hc, first, n = c["W"], c["H"], c["first"], c["nframes"]
    a = params(seed)
    what = dict(PF.what(c), **a)
    want = AG.new_triple(Wc, Hc)
    res_want = AG.render_adaptive_group_layers(want, AG.of_samples(GLL.of_frames(E)), first, n, **a)
    ctx = vp.Context(0)
    ctx.__enter__()
    acc = tuple(vp.DeviceBuffer(Wc, Hc) for _ in range(3))
    rec = tuple(vp.StatsBuffer(Wc, Hc) for _ in range(3))
    try:
        _set_scene(vp, c)
        P = vp.make_param(Wc, Hc, **c["kw"])
        err = vp.lib().vp_last_error()
        res = vp.render_adaptive_group_layers(*(b.ptr for b in acc + rec), first, n, P, a["rel_tol"], a["floor_y"], a["min_frames"], a["round_frames"])
        got = tuple(b.download() for b in acc + rec)
        bad = AG.same_triple(want, got)
        assert bad is None, (what, bad)
        assert res == res_want, (what, res, res_want)
        assert vp.lib().vp_last_error() == err, (what, vp.lib().vp_last_error())
        if os.environ.get("VP_FUZZ_VERBOSE"):
            print("seed %d: %s frozen %d of %d" % (seed, res, int((want[0].flags & 1).sum()), Wc * Hc))
    finally:
        vp.set_shard(0, 1)
        vp.set_exit_flights(1)
        vp.set_camera()
        for b in acc + rec:
            b.free()
        ctx.__exit__(None, None, None)
        ctx.destroy()
