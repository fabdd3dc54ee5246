"""binary16 volumes, randomised: the seeded random scenes of tests/scenes.py with their grid rounded to binary16 -- uint8 grids
scaled by 1/255 in float32 first, the scale the case's `density` assumes -- rendered by the HIP path from the halves and by the CPU
oracle from the widened grid.  Bar: bit-exact accumulators and equal work counters, as in test_fuzz_gpu.py.
VP_FUZZ_HALF_SEEDS sets the number of seeds (default 16)."""
import os

import numpy as np
import pytest

import scenes

pytestmark = pytest.mark.gpu


def half_case(seed, host):
    c = scenes.random_case(seed, host)
    g = c["grid"]
    if g.dtype == np.uint8:
        g = g.astype(np.float32) * np.float32(1.0 / 255.0)
    c["grid"] = np.ascontiguousarray(g.astype(np.float16))
    return c


def _oracle_render(oracle, c):
    wide = np.ascontiguousarray(c["grid"].astype(np.float32))
    osc = oracle.OracleScene(wide, c["env"], c["sun_dir"], c["sun_power"], box=c["box"], brick=c["brick"], linear=c["linear"],
                             estimator=c["est"], rng_mode=c["rng_mode"], seed=c["key"], inv_view=c["cam"], env_mis=c["env_mis"],
                             track_mode=c["track"])
    oP = oracle.default_param(c["W"], c["H"], **c["kw"])
    if c["late"]:
        osc.precompute_opacity()
    ref, cnt = None, None
    for f in range(c["first"], c["first"] + c["nframes"]):
        ref, k = osc.render_frame(oP, f, ref)
        d = k.as_dict()
        cnt = d if cnt is None else {q: cnt[q] + d[q] for q in d}
    return ref, cnt


@pytest.mark.parametrize("seed", range(int(os.environ.get("VP_FUZZ_HALF_SEEDS", "16"))))
def test_random_scene_binary16_bit_exact(vp, oracle, seed):
    from volpath import host
    c = half_case(seed, host)
    grid, W, H = c["grid"], c["W"], c["H"]
    first, nframes = c["first"], c["nframes"]
    ref, cnt = _oracle_render(oracle, c)
    vP = vp.make_param(W, H, **c["kw"])
    what = dict(seed=seed, grid=grid.shape, box=c["box"], est=c["est"], rng=c["rng_mode"], linear=c["linear"], brick=c["brick"], size=(W, H),
                first=first, nframes=nframes, env_mis=c["env_mis"], track=c["track"], world=c["world"], **c["kw"])
    ctx = vp.Context(0)
    ctx.__enter__()
    buf = vp.DeviceBuffer(W, H)
    try:
        vp.init_volume(grid, box=c["box"], brick=c["brick"], linear=c["linear"])
        info = vp.volume_info()
        assert info["format"] == vp.VOL_F16 and info["cell_bytes"] == 16 and info["cells_bytes"] == 16 * grid.size, info
        vp.init_envmap(c["env"])
        vp.set_sun(c["sun_dir"], c["sun_power"])
        vp.set_camera(c["cam"])
        vp.set_estimator(c["est"])
        vp.set_rng(c["rng_mode"], c["key"])
        vp.set_tracking(c["track"])
        vp.set_envmap_sampling(vp.ENV_MIS if c["env_mis"] else vp.ENV_PASSIVE)
        vp.set_shard(0, 1)
        vp.set_exit_flights(seed % 3)
        if c["late"]:
            vp.precompute_opacity(c["sun_dir"])
        counted = not c["track"]                  # the work counters are not built for the scalar tracking kernels
        vp.enable_counters(counted)
        vp.read_counters(reset=True)
        vp.render_frames(buf.ptr, first, nframes, vP)
        got = buf.download()
        k = vp.read_counters()
        vp.enable_counters(False)
        assert np.array_equal(got, ref, equal_nan=True), (what, float(np.nanmax(np.abs(got - ref))))
        assert oracle.lib().vpo_debug_shadow_overflow() == 0, what
        if counted:
            for q in ("samples", "density_lookups", "bound_lookups", "opacity_lookups", "env_lookups", "scatters"):
                assert k[q] == cnt[q], (what, q, k[q], cnt[q])
        # frame by frame through the reference's entry point, the image as the sum of the shards of `world` ranks
        buf.reset()
        for r in range(c["world"]):
            vp.set_shard(r, c["world"])
            for f in range(first, first + nframes):
                vp.render_kernel(buf.ptr, f, vP)
        assert np.array_equal(buf.download(), ref, equal_nan=True), what
    finally:
        vp.enable_counters(False)
        buf.free()
        ctx.__exit__(None, None, None)
        ctx.destroy()
