"""The fast arithmetic mode (include/volpath.h vp_set_arithmetic, vp_kernels_fast.hip) on the GPU: the exact default is untouched,
the fast kernels change the general pixels only, they are deterministic at tolerance 0, and their images stay within the stated
tolerance of the exact ones.  Every fast render runs in a context of its own: the session's `vp` context keeps the exact default."""
import os
import subprocess

import numpy as np
import pytest

import scenes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def ctx(vp):
    c = vp.Context(0)
    try:
        with c:
            yield c
    finally:
        c.destroy()


def _julia(vp, est, rng, n=64, W=96, H=72, key=(5, 6), opacity=False):
    vp.init_volume(vp.julia_volume(n), brick=1, linear=True)
    vp.init_envmap(scenes.synthetic_env())
    vp.set_sun(scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER)
    vp.set_camera()
    vp.set_estimator(est)
    vp.set_rng(rng, key)
    if opacity:
        vp.precompute_opacity(scenes.DEFAULT_SUN_DIR)
    return vp.make_param(W, H)


def _render(vp, P, first, n):
    buf = vp.DeviceBuffer(P.width, P.height)
    try:
        vp.render_frames(buf.ptr, first, n, P)
        return buf.download()
    finally:
        buf.free()


def _both(vp, P, first, n):
    vp.set_arithmetic(vp.ARITH_EXACT)
    ex = _render(vp, P, first, n)
    assert vp.last_arithmetic() == vp.ARITH_EXACT
    vp.set_arithmetic(vp.ARITH_FAST)
    fa = _render(vp, P, first, n)
    assert vp.last_arithmetic() == vp.ARITH_FAST
    return ex, fa


def test_default_is_exact(vp, oracle, ctx):
    import oracle_lib as O
    W, H = 64, 48
    for est in (vp.EST_DECOMP, vp.EST_GLOBAL):
        P = _julia(vp, est, vp.RNG_PHILOX, n=32, W=W, H=H, key=(1, 2))
        plain = _render(vp, P, 0, 4)
        assert vp.last_arithmetic() == vp.ARITH_EXACT
        vp.set_arithmetic(vp.ARITH_EXACT)
        assert np.array_equal(_render(vp, P, 0, 4), plain)
        osc = O.OracleScene(O.julia(32), scenes.synthetic_env(), scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER, estimator=est,
                            rng_mode=O.RNG_PHILOX, seed=(1, 2))
        ref, oP = None, O.default_param(W, H)
        for f in range(4):
            ref, _ = osc.render_frame(oP, f, ref)
        assert np.array_equal(plain, ref)


def _classes_check(vp, P, ex, fa):
    cls = vp.pixel_table(P)[..., 5].astype(int)
    gen = cls == 0
    assert gen.any()
    assert not np.array_equal(ex[gen], fa[gen]), "the fast mode changed no general pixel"
    assert np.array_equal(ex[~gen], fa[~gen]), "box-missing / light pixels must be bit-identical between the modes"
    assert np.isfinite(fa).all()


@pytest.mark.parametrize("est", [1, 0])
def test_fast_changes_general_pixels_only_julia64(vp, ctx, est):
    P = _julia(vp, est, vp.RNG_PHILOX7)
    ex, fa = _both(vp, P, 0, 8)
    _classes_check(vp, P, ex, fa)


@pytest.mark.parametrize("workload", ["c2", "c3"])
def test_fast_changes_general_pixels_only_full_size(vp, ctx, workload):
    from volpath import scene as vscene
    P, _ = vscene.setup(workload, rng_mode=vp.RNG_PHILOX7, last_frame=4)
    ex, fa = _both(vp, P, 0, 4)
    _classes_check(vp, P, ex, fa)


@pytest.mark.parametrize("est,first", [(1, 0), (0, 0), (1, 8)])
def test_fast_is_deterministic(vp, ctx, est, first):
    """two runs; render_frames against render_kernel's look-ahead; shards against one render -- bit for bit, and for the
    decomposition estimator over frames 8..15, across the switch to the optical-depth table at frame 11."""
    N = 40 if first == 0 else 8
    P = _julia(vp, est, vp.RNG_PHILOX7, opacity=est == vp.EST_DECOMP)   # (decomposition: frames beyond 10 read the table)
    vp.set_arithmetic(vp.ARITH_FAST)
    one = _render(vp, P, first, N)
    assert np.array_equal(_render(vp, P, first, N), one)
    buf = vp.DeviceBuffer(P.width, P.height)
    try:
        vp.set_lookahead(64)
        la0, _ = vp.lookahead_stats()
        for f in range(first, first + N):
            vp.render_kernel(buf.ptr, f, P)
        vp.synchronize()
        assert vp.last_arithmetic() == vp.ARITH_FAST
        if first == 0:
            assert vp.lookahead_stats()[0] > la0, "the look-ahead never staged a batch"
        assert np.array_equal(buf.download(), one)
    finally:
        buf.free()
    try:
        for world in (2, 3, 4):
            tot = np.zeros_like(one)
            for r in range(world):
                vp.set_shard(r, world)
                tot += _render(vp, P, first, N)
            assert np.array_equal(tot, one), world
    finally:
        vp.set_shard(0, 1)


def test_fast_global_walk_same_staged_and_single_frame(vp, ctx):
    """Global majorant: a staged launch hands the camera rays' walk through empty space to approach_k only where a null collision there
    is neutral in the arithmetic of the render -- else one-frame launches (no approach walk) and staged ones would differ.  density 123.4
    is a medium whose null collision in empty space is NOT neutral in IEEE binary32 (the exact mode walks with the throughput table,
    approach mode 2); the others are.  In every one of them a fast render of frames 0..7 in one launch equals eight one-frame renders."""
    for density in (123.4, 800.0, 917.3, 55.5, 333.3, 1234.5):
        P = _julia(vp, vp.EST_GLOBAL, vp.RNG_PHILOX7)
        P.density = density
        vp.set_arithmetic(vp.ARITH_EXACT)
        _render(vp, P, 0, 8)
        exact_mode = vp.last_approach_mode()
        if density == 123.4:
            assert exact_mode == 2
        vp.set_arithmetic(vp.ARITH_FAST)
        staged = _render(vp, P, 0, 8)
        assert vp.last_approach_mode() in (0, 1), density   # (never the exact arithmetic's throughput table)
        single = np.zeros_like(staged)
        for f in range(8):
            single += _render(vp, P, f, 1)
        assert np.array_equal(staged, single), (density, exact_mode)


def _rel_l2(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@pytest.mark.parametrize("workload,frames", [("c2", 1024), ("c3", 1024), ("c4s", 1024), ("c4f", 256)])
def test_fast_within_stated_tolerance(vp, ctx, workload, frames):
    from volpath import scene as vscene
    P, _ = vscene.setup(workload, rng_mode=vp.RNG_PHILOX, last_frame=frames)
    ex, fa = _both(vp, P, 0, frames)
    ie = ex[..., :3].astype(np.float64) / frames
    im = fa[..., :3].astype(np.float64) / frames
    assert np.isfinite(im).all()
    assert np.allclose(im.mean(axis=(0, 1)), ie.mean(axis=(0, 1)), rtol=2e-3), (im.mean(axis=(0, 1)), ie.mean(axis=(0, 1)))
    by, bx = P.height // 40, P.width // 40
    blocks = lambda x: x.reshape(by, 40, bx, 40, 3).mean(axis=(1, 3))
    spread = lambda x: x.reshape(by, 40, bx, 40, 3).std(axis=(1, 3)) / np.sqrt(1600.0)
    tol = 0.01 * ie.mean() + 4.0 * np.sqrt(spread(im) ** 2 + spread(ie) ** 2)
    assert (np.abs(blocks(im) - blocks(ie)) > tol).mean() < 0.01
    if frames == 1024:
        assert _rel_l2(im, ie) <= vp.ARITH_FAST_REL_L2, _rel_l2(im, ie)


def test_unsupported_combinations_refused(vp, ctx):
    P = _julia(vp, vp.EST_DECOMP, vp.RNG_PHILOX7, n=32, W=32, H=24)
    vp.set_arithmetic(vp.ARITH_FAST)
    base = _render(vp, P, 0, 2)

    def refused(setup, undo):
        setup()
        try:
            with pytest.raises(vp.VolpathError, match="error -2"):
                _render(vp, P, 0, 2)
        finally:
            undo()
        assert np.array_equal(_render(vp, P, 0, 2), base)

    refused(lambda: vp.set_rng(vp.RNG_SAMPLERH, (5, 6)), lambda: vp.set_rng(vp.RNG_PHILOX7, (5, 6)))
    refused(lambda: vp.set_estimator(vp.EST_BOUNDED), lambda: vp.set_estimator(vp.EST_DECOMP))
    refused(lambda: (vp.set_rng(vp.RNG_PHILOX, (5, 6)), vp.set_envmap_sampling(vp.ENV_MIS)),
            lambda: (vp.set_envmap_sampling(vp.ENV_PASSIVE), vp.set_rng(vp.RNG_PHILOX7, (5, 6))))
    refused(lambda: (vp.set_rng(vp.RNG_PHILOX, (5, 6)), vp.set_tracking(vp.TRACK_SCALAR)),
            lambda: (vp.set_tracking(vp.TRACK_SPECTRAL), vp.set_rng(vp.RNG_PHILOX7, (5, 6))))
    refused(lambda: vp.enable_counters(True), lambda: vp.enable_counters(False))
    assert vp.last_arithmetic() == vp.ARITH_FAST


def _ppm(path):
    raw = open(path, "rb").read()
    parts = raw.split(b"\n", 3)
    assert parts[0] == b"P6"
    w, h = (int(v) for v in parts[1].split())
    return raw, np.frombuffer(parts[3], np.uint8).reshape(h, w, 3)


def test_cli_fast(tmp_path):
    exe = os.path.join(ROOT, "cuda-volpath_amd", "volpath_render")
    imgs = {}
    for mode in ("exact", "fast"):
        out = str(tmp_path / f"{mode}.ppm")
        r = subprocess.run([exe, "--julia", "64", "--size", "160", "120", "--spp", "64", "--batch", "64", "--rng", "philox7",
                            "--arith", mode, "--out", out], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        imgs[mode] = _ppm(out)
    assert imgs["fast"][0] != imgs["exact"][0]
    me, mf = imgs["exact"][1].astype(np.float64).mean(), imgs["fast"][1].astype(np.float64).mean()
    assert abs(mf - me) <= 0.01 * me, (mf, me)
