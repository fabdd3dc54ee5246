"""The inputs of tests/long_ray_cases.py are what they claim to be -- checked with the oracle and the restatements alone, no GPU:
the far cameras straddle the crawl's cap of 700 segments and the bounded estimator's max_depth of 800, and `long_box` has general
pixels whose chain of restart segments stops at the segment table's last record next to pixels whose chain stops earlier.
tests/test_long_rays_gpu.py compares the HIP path with the same restatements and oracle renders bit for bit.
"""
import numpy as np
import pytest

import degenerate_cases as DC
import long_ray_cases as LC
import scenes

f32 = np.float32
CAP = LC.SEG_CAP_ASSUMED


def _far_geometry(oracle):
    g = oracle.julia(32)
    return LC.Geometry(g.shape, None, oracle.bounds(g, oracle.bound_radius(32), 1), 1)


def _centre_t_near(geo, cam):
    o, d = DC.camera_rays(cam, LC.W, LC.H)
    hit, near, _ = geo.intersect(o, (f32(1.0) / d[LC.H // 2, LC.W // 2]).astype(f32))
    assert hit
    return float(near)


def test_far_cameras_enter_the_box_where_they_say(oracle):
    geo = _far_geometry(oracle)
    for name, t in LC.FAR.items():
        cam = LC.far_camera(name)
        assert abs(_centre_t_near(geo, cam) - t) < 1e-4, name
        assert (DC.ray_census(cam, LC.W, LC.H) == 0).all(), "no exact zero direction component"
        o, d = DC.camera_rays(cam, LC.W, LC.H)
        hit, _, _ = geo.intersect(np.broadcast_to(o, d.shape).astype(f32), (f32(1.0) / d).astype(f32))
        assert hit.mean() > 0.6, (name, "the telephoto matrix keeps the box in the image")


def test_crawl_restatement_straddles_the_cap(oracle):
    """699 segments from 34.97 units (the crawl ends by itself), 700 from 35.2 (cut with four to go: the origin is still more than a
    segment in front of the box), and 700 for every box-hitting pixel from 38.5 on"""
    geo = _far_geometry(oracle)
    cy, cx = LC.H // 2, LC.W // 2
    for name, want in (("d34.97", 699), ("d35.2", 700), ("d38.5", 700), ("d41.5", 700), ("d60", 700)):
        cam = LC.far_camera(name)
        ro, segs, draws = LC.crawl(geo, cam, LC.W, LC.H, True)
        assert np.isfinite(ro).all()
        assert segs[cy, cx] == want, (name, segs[cy, cx])
        assert np.array_equal(draws, segs), "the Julia grid has no brick with a positive minimum: one draw per segment"
        assert segs.max() <= LC.CRAWL_CAP
        o, d = DC.camera_rays(cam, LC.W, LC.H)
        hit, near, far = geo.intersect(ro[cy, cx], (f32(1.0) / d[cy, cx]).astype(f32))
        assert hit and (near < LC.SEGMENT) == (want == 699), (name, near)          # finished, or cut short
        if LC.FAR[name] >= 35.2:
            assert abs(float(near) - (LC.FAR[name] - 35.0)) < 2e-3
    assert set(np.unique(LC.crawl(geo, LC.far_camera("d34.97"), LC.W, LC.H, True)[1])) >= {0, 699, 700}


@pytest.mark.parametrize("rng_mode", [0, 2])
def test_bounded_estimator_runs_into_max_depth_on_the_way(oracle, rng_mode):
    """the reference's segment count includes the crawl: from 41.5 units every path of a pixel that squarely meets the box ends at
    segment 800 in front of it -- heat 800 * 0.001 per frame, no radiance, whatever is drawn; from 38.5 some arrive and some do
    not; from 34.97 all arrive.  The other two estimators have no such cap: their images do not go dark."""
    g = oracle.julia(32)
    env = scenes.synthetic_env()
    P = oracle.default_param(LC.W, LC.H, density=60.0)
    cap_heat = f32(LC.MAX_DEPTH) * f32(0.001)
    dark = {}
    for name in ("d34.97", "d38.5", "d41.5", "d60"):
        cam = LC.far_camera(name)
        o, d = LC.camera_rays64(LC.W, LC.H, cam)
        hit, tmin, tmax = LC.slab64(o, d)
        square = hit & (tmax - tmin > 1e-2)
        assert square.sum() > 400
        sc = oracle.OracleScene(g, env, scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER, estimator=oracle.EST_BOUNDED, rng_mode=rng_mode,
                                seed=(3, 4), inv_view=cam)
        capped = np.ones((LC.H, LC.W), bool)
        for frame in (0, 1, 11):
            acc, _ = sc.render_frame(P, frame)
            assert np.isfinite(acc).all()
            at_cap = (acc[..., 3] == cap_heat) & (acc[..., :3] == 0).all(-1)
            assert not (acc[..., 3] > cap_heat).any()
            capped &= at_cap
        dark[name] = capped[square].mean()
        if LC.FAR[name] >= 41.5:
            assert capped[square].all(), name
    assert dark["d34.97"] == 0 and 0.05 < dark["d38.5"] < 0.95, dark
    o, d = LC.camera_rays64(LC.W, LC.H, LC.far_camera("d60"))
    hit, tmin, tmax = LC.slab64(o, d)
    square = hit & (tmax - tmin > 1e-2)
    for est in (oracle.EST_GLOBAL, oracle.EST_DECOMP):
        sc = oracle.OracleScene(g, env, scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER, estimator=est, rng_mode=rng_mode, seed=(3, 4),
                                inv_view=LC.far_camera("d60"))
        acc, _ = sc.render_frame(P, 0)
        assert np.isfinite(acc).all() and (acc[square][:, :3] > 0).all() and (acc[square][:, 3] > 0).any()


@pytest.mark.parametrize("brick", [1, 8])
@pytest.mark.parametrize("camera", list(LC.LONG_CAMERAS))
def test_long_box_chains_stop_at_the_cap_and_before_it(oracle, camera, brick):
    """the restated chains of the pixels whose float64 ray passes a non-empty cell (general pixels under any sound certificate):
    at least 50 stop at record cap - 1 for no other reason than the cap, at least 20 stop earlier, and both early reasons occur --
    the ray leaves the box, the brick has a positive minimum.  From record 1 on the capped chains' segments start inside the box (t_near = 0) and are full ones."""
    g = LC.long_box()
    assert g.shape == LC.LONG_SHAPE and not g[:, :, 20:96].any()
    radius = oracle.bound_radius(g.shape[2]) + (1 if brick > 1 else 0)
    geo = LC.Geometry(g.shape, LC.LONG_BOX, oracle.bounds(g, radius, brick), brick)
    cam = LC.long_camera(camera)
    ro, segs, draws = LC.crawl(geo, cam, LC.W, LC.H, True)
    _, d = DC.camera_rays(cam, LC.W, LC.H)
    sel = np.nonzero(LC.meets_medium(g, LC.LONG_BOX, cam, LC.W, LC.H).ravel())[0]
    rec, org, count, why = LC.chain(geo, ro.reshape(-1, 3)[sel], d.reshape(-1, 3)[sel], np.zeros(len(sel), f32), CAP)
    assert np.isfinite(rec).all() and np.isfinite(org).all()
    capped = why == LC.STOP_CAP
    early = count < CAP
    assert capped.sum() >= LC.MIN_CAPPED and early.sum() >= LC.MIN_EARLY, (capped.sum(), early.sum())
    assert ((why & LC.STOP_MISS) != 0).sum() >= 10 and ((why & LC.STOP_MINIMUM) != 0).sum() >= 10
    assert (count[capped] == CAP).all() and (rec[capped][:, :-1, 1] == LC.SEGMENT).all() and (rec[capped][:, 1:, 0] == 0).all()
    stop = rec[..., 2].view(np.uint32) >> 8
    assert all(stop[i, :count[i] - 1].max(initial=0) == 0 and stop[i, count[i] - 1] == 1 for i in range(len(sel)))


@pytest.mark.parametrize("kind", ["u8", "f32", "f16"])
def test_long_box_renders_are_finite_and_meet_both_blobs(oracle, kind):
    g = LC.long_box(kind)
    assert g.dtype == {"u8": np.uint8, "f32": f32, "f16": np.float16}[kind]
    env = scenes.synthetic_env()
    for camera in LC.LONG_CAMERAS:
        for est in (oracle.EST_GLOBAL, oracle.EST_DECOMP, oracle.EST_BOUNDED):
            sc = oracle.OracleScene(g.astype(f32) if kind == "f16" else g, env, scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER,
                                    box=LC.LONG_BOX, estimator=est, rng_mode=oracle.RNG_PHILOX7, seed=(3, 4), inv_view=LC.long_camera(camera))
            acc = None
            for frame in range(3):
                acc, _ = sc.render_frame(oracle.default_param(LC.W, LC.H), frame, acc)
            assert np.isfinite(acc).all() and (acc[..., 3] > 0).sum() > 150, (camera, est)
