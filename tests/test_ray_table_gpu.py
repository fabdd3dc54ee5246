"""The per-view ray table of the global-majorant integrator (ray_table_k -> render_k, LaunchDev::ray): per
general pixel the camera ray's direction, the raw outputs of its box test and its certified-empty distance, read by a fresh sample
instead of being computed.  Memoisation of deterministic functions of the pixel: the tolerance is 0 everywhere.

  - the table against the device functions it replaces (vp_test_camera_ray in both arithmetic units, vp_test_intersect_box, the pixel
    table's word 4), bit for bit, for cameras outside and inside the box, along an axis and half past the box;
  - staleness: a moved camera, another image size, another shard, each without vp_prepare, against a fresh context;
  - images and work counters against the CPU oracle with the table on and with VP_NO_RAY_TABLE=1, each setting in a child process of
    its own (tests/ray_table_cases.py; the knob is read when the device is first used); the decomposition estimator on and off.

Shapes: Julia 32^3, 24 x 16 and 37 x 19 (partial edge tiles, list slots outside the image), frames 9..12, density 4000, g 0.877,
key (3, 4), as in tests/test_tracking_step_gpu.py."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest

import layers_lib as L
import ray_table_cases as RC
import scenes
import subpixel_lib as SL

pytestmark = pytest.mark.gpu

F32 = np.float32
FRAMES = range(RC.FIRST, RC.FIRST + RC.NFRAMES)


def _same(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = np.argwhere(got.view(np.uint32) != ref.view(np.uint32))
    assert len(bad) == 0, (what, len(bad), bad[:4].tolist())


@contextlib.contextmanager
def _context(vp, **env):
    """a context created under `env` (the knobs are read at creation)"""
    env = dict({"VP_NO_RAY_TABLE": "0"}, **env)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        c = vp.Context(0)
    finally:
        for k, v in old.items():
            os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)
    try:
        with c:
            yield c
    finally:
        c.destroy()


@pytest.fixture(scope="module")
def ctx(vp):
    with _context(vp) as c:
        yield c


# ------------------------------------------------------------------------------------------- the table against the functions
CAMERAS = ["default", "orbit0", "orbit1", "orbit2", "orbit3", "inside", "axis", "partial"]


@pytest.mark.parametrize("camera", CAMERAS)
def test_table_equals_the_device_functions(vp, ctx, camera):
    cam = RC.cameras(vp)[camera]
    RC.scene(vp, cam=cam)
    for W, H in RC.SIZES:
        P = vp.make_param(W, H, density=RC.DENSITY, g=RC.G)
        general, light, miss = vp.pixel_lists(P)
        tab = vp.ray_table(P)
        ptab = vp.pixel_table(P)
        assert tab.shape == (len(general), 8)
        x, y = (general & 0xffff).astype(np.intp), (general >> 16).astype(np.intp)
        inside = (x < W) & (y < H)                       # (slots of a partial edge tile outside the image are never read)
        n = int(inside.sum())
        print(f"{camera} {W}x{H}: {n} general pixels in the image of {len(general)} slots, {len(light)} light, {len(miss)} missing the box")
        assert n >= 32, (camera, W, H, n)
        px, t = general[inside], tab[inside]
        # the camera ray, as the exact and as the fast unit compile it, and its float32 restatement
        vp.set_arithmetic(vp.ARITH_EXACT)
        rd, tn, tf, hit = vp.test_camera_ray(W, H, px)
        vp.set_arithmetic(vp.ARITH_FAST)
        try:
            rd_f, tn_f, tf_f, hit_f = vp.test_camera_ray(W, H, px)
        finally:
            vp.set_arithmetic(vp.ARITH_EXACT)
        _same(rd_f, rd, (camera, "camera ray: fast unit against exact unit"))
        _same(tn_f, tn, (camera, "t_near: fast unit against exact unit"))
        _same(tf_f, tf, (camera, "t_far: fast unit against exact unit"))
        assert np.array_equal(hit_f, hit)
        restated = np.array([L.camera_dir(cam, W, H, int(a), int(b)) for a, b in zip(x[inside], y[inside])], F32)
        _same(rd, restated, (camera, "camera ray against its float32 restatement"))
        # the box test of that ray through the existing hook
        ro = np.tile(np.array([cam[3], cam[7], cam[11]], F32), (n, 1))
        hit_b, tn_b, tf_b = vp.test_intersect_box(ro, rd)
        _same(tn_b, tn, (camera, "t_near: the two hooks"))
        _same(tf_b, tf, (camera, "t_far: the two hooks"))
        # the table
        _same(t[:, :3], rd, (camera, W, H, "rd"))
        _same(t[:, 3], tn_b, (camera, W, H, "t_near"))
        _same(t[:, 4], tf_b, (camera, W, H, "t_far"))
        _same(t[:, 5], ptab[y[inside], x[inside], 4], (camera, W, H, "t_empty"))
        assert not t[:, 6:].view(np.uint32).any()
        # no hit flag is stored: the reader's two compares are the function's
        with np.errstate(invalid="ignore"):
            assert np.array_equal((t[:, 4] > t[:, 3]) & (t[:, 4] >= F32(1e-3)), hit_b)
        assert hit_b.all(), "a general pixel's camera ray meets the box"
        if camera == "inside":
            assert (t[:, 3] < 0).all()
        if camera == "axis" and (W, H) == RC.SIZES[0]:     # (u = 0 needs an even width: column W / 2)
            assert (rd == 0).any(), "no direction component is zero: the camera does not look along an axis"
        if camera == "partial":
            assert len(miss) > 0, "every camera ray meets the box"


def test_hook_says_where_there_is_no_table(vp, ctx):
    P = vp.make_param(*RC.SIZES[0], density=RC.DENSITY, g=RC.G)
    RC.scene(vp, est=vp.EST_DECOMP)
    with pytest.raises(vp.VolpathError):
        vp.ray_table(P)
    RC.scene(vp, subpixel=2)
    try:
        with pytest.raises(vp.VolpathError):
            vp.ray_table(P)
    finally:
        vp.set_subpixel(1)
    RC.scene(vp)
    assert vp.ray_table(P).shape[0] >= 32
    with _context(vp, VP_NO_RAY_TABLE="1"):
        RC.scene(vp)
        with pytest.raises(vp.VolpathError):
            vp.ray_table(P)


# ---------------------------------------------------------------------------------------------------------------- staleness
def _frames(vp, size, buf=None):
    P = vp.make_param(*size, density=RC.DENSITY, g=RC.G)
    b = buf if buf is not None else vp.DeviceBuffer(*size)
    try:
        b.reset()
        vp.render_frames(b.ptr, RC.FIRST, RC.NFRAMES, P)
        assert vp.last_ray_table() == 1
        return b.download()
    finally:
        if buf is None:
            b.free()


def _fresh(vp, size, **kw):
    with _context(vp):
        RC.scene(vp, **kw)
        return _frames(vp, size)


def test_moved_camera_rebuilds_the_table(vp, ctx):
    cams = RC.cameras(vp)
    RC.scene(vp, cam=cams["default"])
    first = _frames(vp, RC.SIZES[0])
    vp.set_camera(cams["orbit2"])                      # no vp_prepare: the render call finds the table stale
    second = _frames(vp, RC.SIZES[0])
    assert not np.array_equal(first, second)
    _same(second, _fresh(vp, RC.SIZES[0], cam=cams["orbit2"]), "after set_camera")


def test_changed_image_size_rebuilds_the_table(vp, ctx):
    RC.scene(vp)
    _frames(vp, RC.SIZES[0])
    _same(_frames(vp, RC.SIZES[1]), _fresh(vp, RC.SIZES[1]), "after a change of the image size")
    _same(_frames(vp, RC.SIZES[0]), _fresh(vp, RC.SIZES[0]), "and back")


def test_changed_shard_rebuilds_the_table(vp, ctx):
    size = RC.SIZES[1]
    RC.scene(vp, shard=(0, 2))
    a = _frames(vp, size)
    vp.set_shard(1, 2)
    try:
        b = _frames(vp, size)
        _same(b, _fresh(vp, size, shard=(1, 2)), "after set_shard")
        assert ((a[..., 3] > 0) & (b[..., 3] > 0)).sum() == 0, "two shards rendered the same pixel"
    finally:
        vp.set_shard(0, 1)
    _same(a + b, _fresh(vp, size), "the two shards make up the image")


# ------------------------------------------------------------------------- the renders, table on and off, each in a child process
@pytest.fixture(scope="module")
def renders(tmp_path_factory):
    """{setting: {case/key: array}} of tests/ray_table_cases.py, run once per setting in a fresh process"""
    out = {}
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ray_table_cases.py")
    for setting, knob in (("on", "0"), ("off", "1")):
        path = str(tmp_path_factory.mktemp("ray_table") / f"{setting}.npz")
        r = subprocess.run([sys.executable, script, path], env=dict(os.environ, VP_NO_RAY_TABLE=knob), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (setting, r.stdout[-2000:], r.stderr[-4000:])
        with np.load(path) as z:
            out[setting] = {k: z[k] for k in z.files}
    return out


_ORACLE = {}


def _scene_of(oracle, name, inv_view=None):
    c = RC.RENDERS[name]
    g = RC.grid_of(c.get("volume", "u8"), oracle.julia(RC.N))
    g = np.ascontiguousarray(g.astype(F32)) if g.dtype == np.float16 else g        # a binary16 volume renders as the widened floats
    kw = {} if inv_view is None else {"inv_view": inv_view}
    osc = oracle.OracleScene(g, scenes.synthetic_env(), scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER, brick=c.get("brick", 1),
                             estimator=c.get("est", 0), rng_mode=c.get("rng", 2), seed=RC.KEY, **kw)
    if c.get("est", 0) == oracle.EST_DECOMP:
        osc.precompute_opacity()
    return osc, RC.param(oracle, c.get("size", RC.SIZES[0]), c.get("chromatic", False), c.get("layers", False))


def _oracle(oracle, name):
    """(accumulator, summed counters) of the oracle for a plain case: once per session, never written to"""
    if name not in _ORACLE:
        osc, P = _scene_of(oracle, name)
        acc, cnt = None, None
        for f in FRAMES:
            acc, c = osc.render_frame(P, f, acc)
            d = c.as_dict()
            cnt = d if cnt is None else {q: cnt[q] + d[q] for q in d}
        assert np.isfinite(acc).all()
        acc.setflags(write=False)
        _ORACLE[name] = (acc, cnt)
    return _ORACLE[name]


@pytest.mark.parametrize("name", ["p7", "p7_37x19", "p10", "samplerh", "chromatic", "half"])
def test_images_and_counters_equal_the_oracle(oracle, renders, name):
    ref, cnt = _oracle(oracle, name)
    assert (ref[..., 3] > 0).sum() >= 32
    for setting, flag in (("on", 1), ("off", 0)):
        r = renders[setting]
        assert int(r[f"{name}/table"][0]) == flag, (name, setting)
        _same(r[f"{name}/img"], ref, (name, setting, "timed launch"))
        if RC.RENDERS[name].get("counters"):
            assert int(r[f"{name}/table_counting"][0]) == flag, (name, setting)
            _same(r[f"{name}/img_counting"], ref, (name, setting, "counting launch"))
            got = dict(zip(RC.COUNTERS, r[f"{name}/counters"].tolist()))
            assert got == {q: cnt[q] for q in RC.COUNTERS}, (name, setting)


def test_layers_launch_equals_the_expectation(oracle, renders):
    def make():
        osc, P = _scene_of(oracle, "layers")
        del osc
        real, twin = L.scenes_for(oracle, oracle.julia(RC.N), L.ENV, scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER, estimator=0, rng_mode=2,
                                  seed=RC.KEY)
        return real, twin, P, list(FRAMES)
    e = L.expectation(oracle, ("ray_table", "layers"), make)
    assert e.unscattered.any() and not e.unscattered.all()
    for setting, flag in (("on", 1), ("off", 0)):
        r = renders[setting]
        assert int(r["layers/table"][0]) == flag
        _same(r["layers/fg"], e.fg, (setting, "foreground"))
        _same(r["layers/trans"], e.trans, (setting, "transmittance"))


def test_fast_arithmetic_reads_the_same_bits(renders):
    assert int(renders["on"]["fast/table"][0]) == 1 and int(renders["off"]["fast/table"][0]) == 0
    assert (renders["on"]["fast/img"][..., 3] > 0).sum() >= 32
    _same(renders["on"]["fast/img"], renders["off"]["fast/img"], "fast arithmetic, table on against off")


def test_subpixel_factor_does_not_use_the_table(vp, oracle, renders):
    osc, P = _scene_of(oracle, "sub2")
    ref = SL.oracle_expectation(vp, osc, P, 2, RC.FIRST, RC.NFRAMES)
    for setting in ("on", "off"):
        assert int(renders[setting]["sub2/table"][0]) == 0, setting
        _same(renders[setting]["sub2/img"], ref, (setting, "sub-pixel factor 2"))


def test_lookahead_sequence_with_a_camera_move(vp, oracle, renders):
    cams = RC.cameras(vp)
    acc = None
    for n, cam in enumerate((cams["default"], cams["orbit1"])):
        osc, P = _scene_of(oracle, "lookahead", inv_view=cam)
        for f in range(RC.FIRST + n * RC.LA_FRAMES, RC.FIRST + (n + 1) * RC.LA_FRAMES):
            acc, _ = osc.render_frame(P, f, acc)
    for setting in ("on", "off"):
        r = renders[setting]
        print(setting, "look-ahead batches launched, cancelled:", r["lookahead/la"].tolist())
        assert int(r["lookahead/la"][0]) >= 1, "no look-ahead batch ran: the sequence is too short"
        _same(r["lookahead/img"], acc, (setting, "render_kernel sequence"))


@pytest.mark.parametrize("name", ["c3", "c3ref"])
def test_decomposition_estimator_is_untouched(oracle, renders, name):
    ref, _ = _oracle(oracle, name)
    assert int(renders["on"][f"{name}/table"][0]) == 0 and int(renders["off"][f"{name}/table"][0]) == 0
    _same(renders["on"][f"{name}/img"], renders["off"][f"{name}/img"], (name, "table on against off"))
    _same(renders["on"][f"{name}/img"], ref, (name, "against the oracle"))
