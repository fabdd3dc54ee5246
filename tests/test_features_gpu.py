"""The feature pass (include/volpath.h vp_render_features) on the GPU against its numpy restatement (tests/features_lib.py), bit for
bit unless a test says otherwise: 24 x 16 images, step 0.01 (at most ~350 steps per ray)."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import degenerate_cases as D
import features_lib as FL
import scenes

pytestmark = pytest.mark.gpu

F32 = np.float32
W, H, STEP = 24, 16, 0.01
MEDIUM = dict(density=40.0, sigma_t=(1.0, 0.6, 0.3))
VP_E_ARG, VP_E_STATE = -3, -2
SENTINEL = F32(-7.25)


@pytest.fixture
def ctx(vp):
    c = vp.Context(0)
    try:
        with c:
            yield c
    finally:
        c.destroy()


def _scene(vp, grid, box=None, brick=1, linear=True, est=0, cam=None, with_lights=False):
    vp.init_volume(grid, box=box, brick=brick, linear=linear)
    vp.set_camera(vp.DEFAULT_CAMERA if cam is None else tuple(float(v) for v in cam))
    vp.set_estimator(est)
    vp.set_shard(0, 1)
    if with_lights:
        vp.init_envmap(scenes.synthetic_env())
        vp.set_sun(scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER)


_REF = {}


def _ref(oracle, key, grid, box=None, linear=True, cam=None, size=(W, H), step=STEP, tau_z=FL.TAU_Z_DEFAULT, medium=MEDIUM):
    """the restatement of a case, computed once per session and read-only"""
    if key not in _REF:
        g = np.ascontiguousarray(grid.astype(F32)) if grid.dtype == np.float16 else grid
        kw = {} if cam is None else {"inv_view": cam}
        osc = oracle.OracleScene(g, scenes.synthetic_env(), scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER, box=box, linear=linear, **kw)
        a, d, n = FL.features(oracle, osc, size[0], size[1], step, medium["density"], medium["sigma_t"], tau_z)
        for v in (a, d, n):
            v.setflags(write=False)
        _REF[key] = (a, d, n, osc)
    return _REF[key]


def _same(got, ref, what):
    (ga, gd), (ra, rd) = got, ref
    bad = np.argwhere((FL.bits(ga) != FL.bits(ra)).any(-1) | (FL.bits(gd) != FL.bits(rd)).any(-1))
    assert len(bad) == 0, (what, len(bad), bad[:4].tolist(), [(ga[y, x], ra[y, x], gd[y, x], rd[y, x]) for y, x in bad[:2]])


def _features(vp, size=(W, H), step=STEP, tau_z=FL.TAU_Z_DEFAULT, medium=MEDIUM):
    return vp.render_features(vp.make_param(size[0], size[1], **medium), step, float(tau_z))


# ---------------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("linear", [True, False], ids=["linear", "point"])
def test_parity_julia(vp, oracle, ctx, linear):
    grid = oracle.julia(32)
    ra, rd, steps, osc = _ref(oracle, ("julia", linear), grid, linear=linear)
    assert steps.max() > 100 and (rd[..., 3] == 1).any() and (rd[..., 3] == 0).any()
    out = {}
    for est in (vp.EST_GLOBAL, vp.EST_DECOMP):
        for brick in (1, 4):
            _scene(vp, grid, brick=brick, linear=linear, est=est)
            if not out:
                # the restated rays and box tests are the device's (vp_test_camera_ray, exact mode): once
                pix = np.array([(y << 16) | x for y in range(H) for x in range(W)], np.uint32)
                d, tn, tf, hit = vp.test_camera_ray(W, H, pix)
                _, rrd, rhit, rtn, rtf = FL.box_tests(oracle, osc, W, H)
                assert np.array_equal(FL.bits(d), FL.bits(rrd.reshape(-1, 3))) and np.array_equal(hit, rhit.ravel())
                assert np.array_equal(FL.bits(tn), FL.bits(rtn.ravel())) and np.array_equal(FL.bits(tf), FL.bits(rtf.ravel()))
            out[(est, brick)] = _features(vp)
            _same(out[(est, brick)], (ra, rd), (linear, est, brick))
    for brick in (1, 4):
        for k in range(2):
            assert np.array_equal(FL.bits(out[(vp.EST_GLOBAL, brick)][k]), FL.bits(out[(vp.EST_DECOMP, brick)][k]))


# ---------------------------------------------------------------------------------------------------- 2. formats
USER_BOX = ((-0.5, -1.0, 0.25), (1.5, 0.0, 1.0))
CAM_USER = None


def _cam_at(vp_host, box):
    bmin, bmax = np.array(box[0]), np.array(box[1])
    c = (bmin + bmax) / 2
    pos = c + np.array([0.4, 0.9, 3.0])
    fwd = c - pos
    fwd /= np.linalg.norm(fwd)
    return vp_host.camera_matrix(pos.astype(F32), fwd.astype(F32), np.array([0, 1, 0], F32))


def test_formats_f32_and_f16(vp, oracle, ctx):
    import volpath.host as host
    cam = tuple(float(v) for v in _cam_at(host, USER_BOX))
    g32 = oracle.cloud(16)
    g16 = g32.astype(np.float16)
    wide = np.ascontiguousarray(g16.astype(F32))
    assert not np.array_equal(wide, g32)
    got = {}
    for name, grid in (("f32", g32), ("f16", g16), ("wide", wide)):
        ra, rd, _, _ = _ref(oracle, ("cloud16", "f32" if name == "f32" else "wide"), grid, box=USER_BOX, cam=cam)
        _scene(vp, grid, box=USER_BOX, cam=cam)
        assert vp.volume_info()["format"] == (vp.VOL_F16 if name == "f16" else vp.VOL_F32)
        got[name] = _features(vp)
        _same(got[name], (ra, rd), name)
    assert (got["f32"][1][..., 3] == 1).any()
    for k in range(2):
        assert np.array_equal(FL.bits(got["f16"][k]), FL.bits(got["wide"][k]))
    assert not np.array_equal(FL.bits(got["f16"][0]), FL.bits(got["f32"][0]))


# ---------------------------------------------------------------------------------------------------- 3. cameras
def _away(m):
    m = np.array(m, F32).reshape(3, 4).copy()
    m[:, 0] *= -1                      # half a turn about `up`: right and forward change sign
    m[:, 2] *= -1
    return m.ravel()


CAMERAS = {
    "inside": lambda: D.camera("julia32", "centre", 0, 1),
    "away": lambda: _away(D.camera("julia32", "outside", 0, 1)),
    "axis_parallel": lambda: D.camera("julia32", "outside", 1, -1),
    "in_cell_plane": lambda: D.camera("julia32", "in_cell_plane", 2, 1),
}


@pytest.mark.parametrize("name", list(CAMERAS))
def test_cameras(vp, oracle, ctx, name):
    cam = tuple(float(v) for v in CAMERAS[name]())
    grid = oracle.julia(32)
    ra, rd, steps, osc = _ref(oracle, ("cam", name), grid, cam=cam)
    _, _, hit, tn, _ = FL.box_tests(oracle, osc, W, H)
    if name == "inside":
        assert hit.all() and (tn < 0).all(), "the camera is inside: every ray starts at the clamp"
    elif name == "away":
        assert not hit.any() and (ra == 0).all()
    else:
        assert D.ray_census(list(cam), W, H).max() >= 2, "no axis-parallel ray in this view"
    for est in (vp.EST_GLOBAL, vp.EST_DECOMP):
        _scene(vp, grid, cam=cam, est=est)
        _same(_features(vp), (ra, rd), (name, est))


# ---------------------------------------------------------------------------------------------------- 4. classes and the shortcuts
CHILD = """import sys, numpy as np
sys.path.insert(0, %r)
import volpath as vp
vp.set_device(0)
grid = np.load(%r)
vp.init_volume(grid, brick=1, linear=True)
vp.set_camera()
out = {}
for est in (vp.EST_GLOBAL, vp.EST_DECOMP):
    vp.set_estimator(est)
    a, d = vp.render_features(vp.make_param(%d, %d, density=%r, sigma_t=%r), %r, %r)
    out["a%%d" %% est], out["d%%d" %% est] = a, d
np.savez(%r, **out)
"""


def test_classes_and_shortcuts(vp, oracle, ctx, tmp_path):
    grid = oracle.julia(32)
    ra, rd, _, _ = _ref(oracle, ("julia", True), grid)
    mine = {}
    for est in (vp.EST_GLOBAL, vp.EST_DECOMP):
        _scene(vp, grid, est=est)
        P = vp.make_param(W, H, **MEDIUM)
        general, light, miss = vp.pixel_lists(P)
        assert len(general) and len(light) and len(miss), (est, len(general), len(light), len(miss))
        table = vp.pixel_table(P)
        assert (table[..., 4][table[..., 5] == 0] > 0).any(), "no general pixel has a certified-empty stretch to skip"
        mine[est] = _features(vp)
        _same(mine[est], (ra, rd), ("shortcuts on", est))
    # the second leg: a fresh process whose context reads VP_NO_FEATURE_SKIP=1 -- no class fills, no skip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    grid_file, out_file = str(tmp_path / "grid.npy"), str(tmp_path / "out.npz")
    np.save(grid_file, grid)
    code = CHILD % (os.path.join(root, "cuda-volpath_amd"), grid_file, W, H, MEDIUM["density"], MEDIUM["sigma_t"], STEP, float(FL.TAU_Z_DEFAULT), out_file)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, VP_NO_FEATURE_SKIP="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with np.load(out_file) as z:
        for est in (vp.EST_GLOBAL, vp.EST_DECOMP):
            _same((z["a%d" % est], z["d%d" % est]), mine[est], ("VP_NO_FEATURE_SKIP=1", est))


# ---------------------------------------------------------------------------------------------------- 5. tau_z
def test_tau_z(vp, oracle, ctx):
    grid = oracle.julia(32)
    _scene(vp, grid)
    a0, d0 = _features(vp)
    cover = d0[..., 3] == 1
    assert cover.any() and not cover.all()
    a1, d1 = _features(vp, tau_z=1e-30)
    assert np.array_equal(FL.bits(d1[..., 1][cover]), FL.bits(d1[..., 0][cover])) and np.isinf(d1[..., 1][~cover]).all()
    a2, d2 = _features(vp, tau_z=1e30)
    assert (d2[..., 1] == np.inf).all()
    for a, d in ((a1, d1), (a2, d2)):       # tau_z moves zt and nothing else
        assert np.array_equal(FL.bits(a), FL.bits(a0)) and np.array_equal(FL.bits(d[..., [0, 2, 3]]), FL.bits(d0[..., [0, 2, 3]]))
    fin = np.isfinite(d0[..., 1])
    assert fin.any() and (fin <= cover).all()
    assert (d0[..., 0][fin] <= d0[..., 1][fin]).all() and (d0[..., 1][fin] <= d0[..., 2][fin]).all()


# ---------------------------------------------------------------------------------------------------- 6. shards
@pytest.mark.parametrize("world", [2, 3])
def test_shards(vp, oracle, world):
    grid = oracle.julia(32)
    ra, rd, _, _ = _ref(oracle, ("julia", True), grid)
    P = vp.make_param(W, H, **MEDIUM)
    owner = np.array([[vp.tile_owner(x // 8, y // 8, world) for x in range(W)] for y in range(H)])
    union_a, union_d = np.full((H, W, 4), SENTINEL, F32), np.full((H, W, 4), SENTINEL, F32)
    ctxs = [vp.Context(0) for _ in range(world)]
    try:
        for rank, c in enumerate(ctxs):
            with c:
                _scene(vp, grid)
                vp.set_shard(rank, world)
                a, d = vp.DeviceBuffer(W, H), vp.DeviceBuffer(W, H)
                try:
                    a.upload(np.full((H, W, 4), SENTINEL, F32))
                    d.upload(np.full((H, W, 4), SENTINEL, F32))
                    vp.render_features(P, STEP, alpha_ptr=a.ptr, depth_ptr=d.ptr)
                    vp.synchronize()
                    ga, gd = a.download(), d.download()
                finally:
                    a.free()
                    d.free()
                mine = owner == rank
                assert mine.any()
                assert (ga[~mine] == SENTINEL).all() and (gd[~mine] == SENTINEL).all(), "a rank wrote a pixel it does not own"
                assert np.array_equal(FL.bits(ga[mine]), FL.bits(ra[mine])) and np.array_equal(FL.bits(gd[mine]), FL.bits(rd[mine]))
                union_a[mine], union_d[mine] = ga[mine], gd[mine]
    finally:
        for c in ctxs:
            c.destroy()
    _same((union_a, union_d), (ra, rd), "union of the shards")


# ---------------------------------------------------------------------------------------------------- 7. leaves nothing behind
def _frames(vp, P, first, n):
    b = vp.DeviceBuffer(P.width, P.height)
    try:
        vp.render_frames(b.ptr, first, n, P)
        return b.download()
    finally:
        b.free()


@pytest.mark.parametrize("est", [0, 1], ids=["global", "decomp"])
def test_leaves_nothing_behind_render_frames(vp, oracle, ctx, est):
    _scene(vp, oracle.julia(32), est=est, with_lights=True)
    vp.set_rng(vp.RNG_PHILOX7, (5, 6))
    P = vp.make_param(W, H, **MEDIUM)
    before = _frames(vp, P, 0, 4)
    a, d = _features(vp)
    after = _frames(vp, P, 0, 4)
    assert np.array_equal(FL.bits(before), FL.bits(after)) and before[..., 3].max() > 0
    ra, rd, _, _ = _ref(oracle, ("julia", True), oracle.julia(32))
    _same((a, d), (ra, rd), "between two renders")


def test_leaves_nothing_behind_adaptive(vp, oracle, ctx):
    _scene(vp, oracle.julia(32), est=0, with_lights=True)
    vp.set_rng(vp.RNG_PHILOX7, (5, 6))
    P = vp.make_param(W, H, **MEDIUM)

    def job(between):
        buf, st = vp.DeviceBuffer(W, H), vp.StatsBuffer(W, H)
        try:
            r1 = vp.render_adaptive(buf.ptr, st.ptr, 0, 32, P, 0.05, min_frames=8, round_frames=16)
            if between:
                _features(vp)
            r2 = vp.render_adaptive(buf.ptr, st.ptr, r1["frames_used"], 32, P, 0.05, min_frames=8, round_frames=16)
            return buf.download(), st.download(), r1, r2
        finally:
            buf.free()
            st.free()

    plain, with_features = job(False), job(True)
    assert np.array_equal(FL.bits(plain[0]), FL.bits(with_features[0])) and plain[1].tobytes() == with_features[1].tobytes()
    assert plain[2] == with_features[2] and plain[3] == with_features[3] and plain[2]["samples"] > 0


# ---------------------------------------------------------------------------------------------------- 8. refusals
def _raw(vp, a, d, P, step, tau_z=0.7):
    fp = vp.FeatureParams(step, tau_z)
    return vp.lib().vp_render_features(a, d, C.byref(P), C.byref(fp))


def test_state_and_step_refusals(vp, oracle, ctx):
    P = vp.make_param(W, H, **MEDIUM)
    a, d = vp.DeviceBuffer(W, H), vp.DeviceBuffer(W, H)
    try:
        fill = np.full((H, W, 4), SENTINEL, F32)
        a.upload(fill)
        d.upload(fill)
        assert _raw(vp, a.ptr, d.ptr, P, STEP) == VP_E_STATE, "no volume"
        grid = oracle.julia(32)
        _scene(vp, grid)
        vp.set_subpixel(2)
        assert _raw(vp, a.ptr, d.ptr, P, STEP) == VP_E_STATE and b"sub-pixel" in vp.lib().vp_last_error()
        vp.set_subpixel(1)
        # the box is [-1, 1]^3: its diagonal takes 2 sqrt(3) / step steps
        diag = 2.0 * math.sqrt(3.0)
        assert _raw(vp, a.ptr, d.ptr, P, diag / (FL.MAX_STEPS * 1.001)) == VP_E_ARG and b"steps" in vp.lib().vp_last_error()
        vp.synchronize()
        assert (a.download() == SENTINEL).all() and (d.download() == SENTINEL).all(), "a refused call wrote"
        # the context stays usable
        ra, rd, _, _ = _ref(oracle, ("julia", True), grid)
        assert _raw(vp, a.ptr, d.ptr, P, STEP, float(FL.TAU_Z_DEFAULT)) == 0
        vp.synchronize()
        _same((a.download(), d.download()), (ra, rd), "after the refusals")
    finally:
        a.free()
        d.free()


# ---------------------------------------------------------------------------------------------------- 9. random scenes
@pytest.mark.parametrize("seed", range(8))
def test_random_scenes(vp, oracle, ctx, seed):
    import volpath.host as host
    c = scenes.random_case(seed, host)
    cam = tuple(float(v) for v in c["cam"])
    medium = dict(density=c["kw"]["density"], sigma_t=c["kw"].get("sigma_t", (1.0, 1.0, 1.0)))
    size = (min(c["W"], W), min(c["H"], H))
    # a step that takes about 300 steps across the box diagonal
    g = c["grid"]
    nz, ny, nx = g.shape
    box = c["box"] if c["box"] is not None else ((-1.0, -ny / nx, -nz / nx), (1.0, ny / nx, nz / nx))
    step = float(F32(np.linalg.norm(np.array(box[1]) - np.array(box[0])) / 300.0))
    ra, rd, _, _ = _ref(oracle, ("random", seed), g, box=c["box"], linear=c["linear"], cam=cam, size=size, step=step, medium=medium)
    _scene(vp, g, box=c["box"], brick=c["brick"], linear=c["linear"], est=c["est"], cam=cam)
    _same(_features(vp, size=size, step=step, medium=medium), (ra, rd), (seed, str(g.dtype), c["linear"], c["est"], c["brick"]))


# ---------------------------------------------------------------------------------------------------- 10. closed form, oracle-free
def test_closed_form_homogeneous(vp, ctx):
    grid = np.full((8, 8, 8), 255, np.uint8)
    _scene(vp, grid)
    density, sigma_t = 3.0, (1.0, 0.5, 0.25)
    a, d = vp.render_features(vp.make_param(W, H, density=density, sigma_t=sigma_t), STEP)
    pix = np.array([(y << 16) | x for y in range(H) for x in range(W)], np.uint32)
    _, tn, tf, hit = vp.test_camera_ray(W, H, pix)
    tn, tf, hit = tn.reshape(H, W).astype(np.float64), tf.reshape(H, W).astype(np.float64), hit.reshape(H, W)
    assert hit.any() and not hit.all() and (a[~hit] == 0).all()
    step = float(F32(STEP))
    tau = a[..., 3].astype(np.float64)[hit]
    N = np.rint(tau / (density * step))
    L = (tf - np.maximum(tn, 0.0))[hit]
    print("closed form: N", N.min(), N.max(), "max |tau - density N step|", np.abs(tau - density * N * step).max(),
          "max |tau - density L| / (density step)", (np.abs(tau - density * L) / (density * step)).max())
    # every fetch is exactly 1.0f: tau = density x N x step up to the two products' roundings
    assert (np.abs(tau - density * N * step) <= 2.0 ** -22 * tau).all()
    # the midpoint rule is within one step of the chord, plus the float sum's rounding N x 2^-24 x N (zero here: the sum of N ones is exact)
    assert (np.abs(tau - density * L) <= density * step + density * step * (N * 2.0 ** -24 * N) + 2.0 ** -22 * tau).all()
    # alpha against float64: expf_ is within 1.5 ulp (test_helpers_gpu.py), its argument and the subtraction round once each
    for c in range(3):
        want = -np.expm1(-tau * float(F32(sigma_t[c])))
        err = np.abs(a[..., c].astype(np.float64)[hit] - want)
        print("closed form: channel", c, "max |alpha - (1 - exp(-tau sigma))| in 2^-24:", err.max() * 2.0 ** 24)
        assert (err <= 3 * 2.0 ** -24).all()


# ---------------------------------------------------------------------------------------------------- 11. the layers render converges
def test_layers_render_converges_to_the_march(vp, oracle, ctx):
    """256 frames of vp_render_frames_layers_stats: per pixel with n >= 2 the trans record's mean luminance lies within 6 SE + d of the
    luminance of 1 - alpha.xyz; d is the one-step bound of the march through the exponential: |d exp(-tau sigma)| <= sigma density step"""
    grid = oracle.julia(32)
    step, density, sigma = 0.001, 20.0, 0.8
    medium = dict(density=density, sigma_t=(sigma, sigma, sigma))
    _scene(vp, grid, est=vp.EST_GLOBAL, with_lights=True)
    vp.set_rng(vp.RNG_PHILOX7, (3, 4))
    P = vp.make_param(W, H, **medium)
    a, _ = vp.render_features(P, step)
    fg, tr, fs, ts = vp.DeviceBuffer(W, H), vp.DeviceBuffer(W, H), vp.StatsBuffer(W, H), vp.StatsBuffer(W, H)
    try:
        vp.render_frames_layers_stats(fg.ptr, tr.ptr, fs.ptr, ts.ptr, 0, 256, P)
        rec = ts.download()
    finally:
        for b in (fg, tr, fs, ts):
            b.free()
    n = rec["n"].astype(np.float64)
    ok = n >= 2
    assert ok.sum() >= W * H // 2
    mean = rec["sum_y"][ok] / n[ok]
    var = np.maximum(rec["sum_y2"][ok] / n[ok] - mean * mean, 0.0) * n[ok] / (n[ok] - 1.0)
    se = np.sqrt(var / n[ok])
    t = 1.0 - a[..., :3].astype(np.float64)
    want = ((0.2126 * t[..., 0] + 0.7152 * t[..., 1]) + 0.0722 * t[..., 2])[ok]
    d = sigma * density * step
    excess = np.abs(mean - want) - (6.0 * se + d)
    print("layers vs march: pixels", int(ok.sum()), "max |mean - want|", np.abs(mean - want).max(), "max SE", se.max(), "d", d, "max excess", excess.max())
    assert (want < 0.99).any() and (want > 0.999).any(), "the view has no contrast"
    assert (excess <= 0).all(), (int((excess > 0).sum()), excess.max())
