"""The inputs of tests/degenerate_cases.py are what they claim to be, in binary32, and the CPU oracle defines a finite answer for
each of them (so the bit-exact GPU comparisons of tests/test_degenerate_gpu.py compare numbers, not NaNs)."""
import numpy as np
import pytest

import degenerate_cases as DC
import scenes

f32 = np.float32
CAMERAS = [(g, p, a, s) for g in DC.GRIDS for p in DC.POSITIONS for a, s in DC.VIEWS]


def test_every_camera_has_the_zero_components_it_is_there_for():
    for g, p, a, s in CAMERAS:
        for w, h in ((DC.W, DC.H), (DC.LONG_W, DC.LONG_H)):
            zeros = DC.ray_census(DC.camera(g, p, a, s), w, h)
            assert zeros[h // 2, w // 2] == 2 and (zeros == 2).sum() == 1, (g, p, a, s)
            assert (zeros[h // 2] >= 1).all() and (zeros[:, w // 2] >= 1).all() and (zeros == 1).sum() == w + h - 2, (g, p, a, s)
            o, d = DC.camera_rays(DC.camera(g, p, a, s), w, h)
            assert np.abs(d[h // 2, w // 2, a]) == 1.0 and np.sign(d[h // 2, w // 2, a]) == -s      # looks at the box, along the axis
            n = np.sqrt((d.astype(np.float64) ** 2).sum(-1))
            assert np.abs(n - 1).max() < 2e-7


def test_ray_census_is_the_oracles_camera_ray(oracle):
    """the default camera at an even width: one column with one zero component (u = 0 at x = W / 2), as the oracle's own rays"""
    import ctypes as C
    m = (C.c_float * 12)()
    oracle.lib().vpo_default_camera(m)
    zeros = DC.ray_census(np.array(m[:], f32), DC.W, DC.H)
    assert (zeros[:, DC.W // 2] == 1).all() and zeros.sum() == DC.H


def test_snapped_positions_are_exact():
    for g in DC.GRIDS:
        bmin, bmax = DC.box(g)
        n = DC.dims(g)
        for a, s in DC.VIEWS:
            b, c = (a + 1) % 3, (a + 2) % 3
            pos = lambda p: DC.camera(g, p, a, s).reshape(3, 4)[:, 3]
            snap = bmax if s > 0 else bmin
            assert pos("on_face")[a] == snap[a]
            assert pos("in_face_plane")[b] == snap[b] and bmin[c] < pos("in_face_plane")[c] < bmax[c]
            assert pos("along_edge")[b] == snap[b] and pos("along_edge")[c] == snap[c]
            assert (pos("centre") > bmin).all() and (pos("centre") < bmax).all()
            assert not bmin[a] <= pos("outside")[a] <= bmax[a]
            # in a cell-boundary plane: x * N - 0.5 is an exact integer wherever the box and N allow one (always along x)
            q = [DC.cell_coordinate(pos("in_cell_plane")[k], bmin[k], bmax[k], n[k]) for k in (b, c)]
            exact = [float(v) == round(float(v)) for v in q]
            assert any(exact), (g, a, q)
            if g in ("julia32", "solid7", "user_u8"):
                assert all(exact), (g, a, q)
    assert DC.cell_plane_coordinate(-1.0, 1.0, 32) == f32(-0.03125) and DC.cell_plane_coordinate(-1.0, 1.0, 48) == f32(-0.0625)


def test_in_plane_rays_make_nan_in_the_binary32_slab_test():
    """what the in_face_plane and along_edge cameras are for: inv * (bmax - o) = inf * 0 on the centre row (and column)"""
    for g in DC.GRIDS:
        bmin, bmax = DC.box(g)
        for p, rows in (("in_face_plane", 1), ("along_edge", 2)):
            for a, s in DC.VIEWS:
                o, d = DC.camera_rays(DC.camera(g, p, a, s), DC.W, DC.H)
                with np.errstate(divide="ignore", invalid="ignore"):
                    tt = (f32(1.0) / d) * ((bmax if s > 0 else bmin) - o)       # ttop from the positive side, tbot from the negative
                nan = np.isnan(tt).any(-1)
                assert nan[DC.H // 2].all() and (rows == 1 or nan[:, DC.W // 2].all()) and nan.sum() == (DC.W, DC.W + DC.H - 1)[rows - 1]


def test_user_grid_has_another_dominant_axis_in_cell_units():
    bmin, bmax = DC.box("user_u8")
    e = np.array([1.0, 1.0, 0.0]) * DC.dims("user_u8") / (bmax - bmin).astype(np.float64)
    assert abs(e[1]) > abs(e[0]) > 0
    assert len(set(((bmax - bmin) / DC.dims("user_u8")).tolist())) == 3


@pytest.mark.parametrize("grid", DC.GRIDS)
def test_oracle_is_finite_and_meets_the_medium(oracle, grid):
    """every position (one view each) and, on the uchar grids, every axis sun: finite accumulators, and rays that scatter"""
    g = DC.grid(grid, oracle)
    assert g.max() > 0
    P = oracle.default_param(DC.W, DC.H, density=60.0)
    for i, p in enumerate(DC.POSITIONS):
        a, s = DC.VIEWS[i]
        for est in (oracle.EST_GLOBAL, oracle.EST_DECOMP, oracle.EST_BOUNDED):
            sc = oracle.OracleScene(g, scenes.synthetic_env(), scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER, box=DC.user_box(grid),
                                    estimator=est, rng_mode=oracle.RNG_PHILOX7, seed=(3, 4), inv_view=DC.camera(grid, p, a, s))
            acc = None
            for f in range(3):
                acc, _ = sc.render_frame(P, f, acc)
            assert np.isfinite(acc).all() and (acc[..., 3] > 0).any(), (grid, p, est)
    if grid in ("odd_u8", "solid7"):
        for name, sun in DC.SUNS.items():
            sc = oracle.OracleScene(g, scenes.synthetic_env(), sun, scenes.DEFAULT_SUN_POWER, estimator=oracle.EST_DECOMP,
                                    rng_mode=oracle.RNG_SAMPLERH, inv_view=DC.camera(grid, "outside", 0, 1))
            sc.precompute_opacity()
            assert np.isfinite(sc.opacity).all()
            acc = None
            for f in range(9, 13):
                acc, _ = sc.render_frame(P, f, acc)
            assert np.isfinite(acc).all() and (acc[..., 3] > 0).any(), (grid, name)
