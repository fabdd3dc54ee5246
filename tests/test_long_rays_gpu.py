"""GPU parity on long rays (tests/long_ray_cases.py): cameras 35 to 60 units in front of the box -- the restart crawl's cap of 700
segments, the bounded estimator's max_depth of 800 reached on the way -- and a box seven units long, empty between its ends, in which
the chains of the per-view segment table (approach_segments_k -> approach_local_tab_k) run into the table's cap.  Bar: the HIP path
equals the CPU oracle bit for bit (tolerance 0) and does the same work; the per-pixel tables equal their binary32 restatements bit
for bit.  tests/test_reference_kernel_cpu.py holds the oracle to the reference's own kernel code on a subset of these cases, and
tests/test_long_rays_cpu.py shows that the inputs reach the caps they are named after.

The segment table's cap is taken from the library (vp_get_segment_table), never written down here: raising it makes the census
asserts fail instead of emptying them.  Every oracle accumulator is asserted finite before anything is compared with it.
"""
import contextlib
import os

import numpy as np
import pytest

import degenerate_cases as DC
import long_ray_cases as LC
import scenes

pytestmark = pytest.mark.gpu

f32 = np.float32
KEY = (0x10C0FFEE, 41)
COUNTERS = ("samples", "density_lookups", "bound_lookups", "opacity_lookups", "env_lookups", "scatters")
W, H = LC.W, LC.H
LONG_FRAMES = (3, 70)           # frames 3..72: a full block of 64 and a ragged one, across the frame-11 switch


@contextlib.contextmanager
def _context(vp, **env):
    """a context created under `env` (knobs are read at creation) that takes no volume for dense: the approach walks always run"""
    env = dict(env, VP_DENSE_PERCENT="101")
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


# ------------------------------------------------------------------------------------------------------------------- scenes
def _grid(oracle, scene):
    return oracle.julia(32) if scene == "far" else LC.long_box(scene[5:] or "u8")          # "long", "long_f32", "long_f16"


def _box(scene):
    return None if scene == "far" else LC.LONG_BOX


def _camera(scene, camera):
    return LC.far_camera(camera) if scene == "far" else LC.long_camera(camera)


_ORACLE = {}


def _oracle(oracle, scene, camera, est, rng_mode, brick, density, first, n):
    """(accumulator, summed counters) of the oracle: computed once per case, shared, never written to"""
    k = (scene, camera, est, rng_mode, brick, density, first, n)
    if k not in _ORACLE:
        g = _grid(oracle, scene)
        sc = oracle.OracleScene(g.astype(f32) if g.dtype == np.float16 else g, scenes.synthetic_env(), scenes.DEFAULT_SUN_DIR,
                                scenes.DEFAULT_SUN_POWER, box=_box(scene), brick=brick, estimator=est, rng_mode=rng_mode, seed=KEY,
                                inv_view=_camera(scene, camera))
        if est == oracle.EST_DECOMP and first + n - 1 > 10:
            sc.precompute_opacity()
        P = oracle.default_param(W, H, density=density)
        acc, cnt = None, None
        for f in range(first, first + n):
            acc, c = sc.render_frame(P, f, acc)
            d = c.as_dict()
            cnt = d if cnt is None else {q: cnt[q] + d[q] for q in d}
        assert np.isfinite(acc).all(), ("the oracle's accumulator is not finite: change the case", k)
        assert oracle.lib().vpo_debug_shadow_overflow() == 0
        acc.setflags(write=False)
        _ORACLE[k] = (acc, cnt)
    return _ORACLE[k]


def _scene(vp, oracle, scene, camera, est, rng_mode, brick, late, arith=None):
    vp.set_arithmetic(vp.ARITH_EXACT if arith is None else arith)
    vp.set_subpixel(1)
    vp.init_volume(_grid(oracle, scene), box=_box(scene), brick=brick, linear=True)
    vp.init_envmap(scenes.synthetic_env())
    vp.set_sun(scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER)
    vp.set_camera(tuple(float(v) for v in _camera(scene, camera)))
    vp.set_estimator(est)
    vp.set_rng(rng_mode, KEY)
    vp.set_tracking(0)
    vp.set_envmap_sampling(vp.ENV_PASSIVE)
    vp.set_exit_flights(1)
    vp.set_shard(0, 1)
    vp.set_lookahead(vp.LOOKAHEAD_DEFAULT)
    if late:
        vp.precompute_opacity(scenes.DEFAULT_SUN_DIR)


def _same(got, ref, what):
    assert got.tobytes() == ref.tobytes(), (what, int((got != ref).any(-1).sum()), np.argwhere((got != ref).any(-1))[:4].tolist())


def _counting_launch(vp, buf, P, first, n, ref, cnt, what, monkeypatch, walk):
    """a counting launch; walk: with the approach kernels tallying their own steps (VP_COUNT_APPROACH), else the integrator walks"""
    if walk:
        monkeypatch.setenv("VP_COUNT_APPROACH", "1")
    try:
        vp.enable_counters(True)
        vp.read_counters(reset=True)
        buf.reset()
        vp.render_frames(buf.ptr, first, n, P)
        k = vp.read_counters()
        _same(buf.download(), ref, (what, "counting launch", walk))
        for q in COUNTERS:
            assert k[q] == cnt[q], (what, walk, q, k[q], cnt[q])
    finally:
        vp.enable_counters(False)
        if walk:
            monkeypatch.delenv("VP_COUNT_APPROACH")
    return vp.last_approach_mode()


# --------------------------------------------------------------------------------------------------------------- far cameras
@pytest.mark.parametrize("brick", [1, 4])
@pytest.mark.parametrize("camera", list(LC.FAR))
def test_far_camera_bit_exact(vp, ctx, oracle, monkeypatch, camera, brick):
    """three estimators x sampler.h and Philox-7 over frames 7..12 (across the frame-11 switch to the optical-depth table): the
    staged launch, the counting launch with and without the walk tallied, and one render_kernel call per frame equal the oracle --
    accumulators and the six work counters"""
    first, n = 7, 6
    for est in (vp.EST_GLOBAL, vp.EST_DECOMP, vp.EST_BOUNDED):
        b = brick if est else 1
        for rng_mode in (vp.RNG_SAMPLERH, vp.RNG_PHILOX7):
            ref, cnt = _oracle(oracle, "far", camera, est, rng_mode, b, 60.0, first, n)
            assert (ref[..., 3] > 0).sum() > 100
            _scene(vp, oracle, "far", camera, est, rng_mode, b, late=est == vp.EST_DECOMP)
            P = vp.make_param(W, H, density=60.0)
            what = dict(camera=camera, est=est, rng=rng_mode, brick=b)
            buf = vp.DeviceBuffer(W, H)
            try:
                vp.render_frames(buf.ptr, first, n, P)
                _same(buf.download(), ref, (what, "render_frames"))
                if est != vp.EST_BOUNDED:
                    assert vp.last_approach_mode() == 1, what
                assert _counting_launch(vp, buf, P, first, n, ref, cnt, what, monkeypatch, walk=False) == 0
                _counting_launch(vp, buf, P, first, n, ref, cnt, what, monkeypatch, walk=True)
                buf.reset()
                for f in range(first, first + n):
                    vp.render_kernel(buf.ptr, f, P)
                _same(buf.download(), ref, (what, "render_kernel"))
            finally:
                buf.free()


def _geometry(vp, scene, brick):
    tab, b, _ = vp.bound_table()
    assert b == brick
    return LC.Geometry(LC.LONG_SHAPE if scene != "far" else (32, 32, 32), _box(scene), tab, brick)


CRAWL_CASES = [("far", c) for c in LC.FAR] + [("long", c) for c in LC.LONG_CAMERAS]


@pytest.mark.parametrize("scene,camera", CRAWL_CASES)
def test_crawl_table_is_the_restatement_bit_for_bit(vp, ctx, oracle, scene, camera):
    """columns 0..3 of vp_get_pixel_table -- the origin after up to 700 additions, segments | draws << 16 -- equal the numpy
    restatement of crawl_table_k for the decomposition estimator (which would draw a control distance where the entry brick had a
    positive minimum) and the bounded one, bricks 1 and 4 (the Julia grid has no such brick and its two tables are
    the same: one estimator per brick there)"""
    P = vp.make_param(W, H)
    for brick in (1, 4):
        for est in ((vp.EST_DECOMP, vp.EST_BOUNDED) if scene == "long" else (vp.EST_DECOMP,) if brick == 1 else (vp.EST_BOUNDED,)):
            _scene(vp, oracle, scene, camera, est, vp.RNG_PHILOX7, brick, late=False)
            t = vp.pixel_table(P)
            ro, segs, draws = LC.crawl(_geometry(vp, scene, brick), _camera(scene, camera), W, H, control_draw=est == vp.EST_DECOMP)
            assert np.isfinite(ro).all()
            assert t[..., :3].tobytes() == ro.tobytes(), (brick, est, np.argwhere((t[..., :3] != ro).any(-1))[:4].tolist())
            packed = t[..., 3].view(np.uint32)
            assert np.array_equal(packed & 0xffff, segs) and np.array_equal(packed >> 16, draws), (brick, est)
            assert segs.max() <= LC.CRAWL_CAP
            if scene == "far":
                assert segs[H // 2, W // 2] == (699 if camera == "d34.97" else LC.CRAWL_CAP)


@pytest.mark.parametrize("est", [0, 1])
@pytest.mark.parametrize("camera", ["d35.2", "d60"])
def test_far_certificates_hold_in_float64(vp, ctx, oracle, camera, est):
    """checks (a) and (b) of test_pins_gpu.py::_pixel_table_certificates from beyond the crawl's cap, against the raw volume in
    float64: (b) class 2 = the ray misses the box; (a) from the box entry up to the certified-empty distance -- measured from where
    the crawl ended: the RESTATED origin (700 additions of binary32 drift off o + d * 35 by more than that helper's 2e-4 would
    allow, which is why it is not reused here) -- every point of the ray, walked at 1/20 cell, lies in a cell whose 2x2x2 texels
    are all zero; class 1 = certified to the end of the chord."""
    brick = 4 if est else 1
    _scene(vp, oracle, "far", camera, est, vp.RNG_PHILOX7, brick, late=False)
    cam = LC.far_camera(camera)
    t = vp.pixel_table(vp.make_param(W, H))
    cls, t_left = t[..., 5].astype(int), t[..., 4].astype(np.float64)
    o, d = LC.camera_rays64(W, H, cam)
    hit, tmin, tmax = LC.slab64(o, d)
    decided = np.abs(tmax - tmin) > 1e-4
    assert np.array_equal((cls == 2)[decided], ~hit[decided]) and set(np.unique(cls)) == {0, 1, 2}
    if est:
        origin, segs, _ = LC.crawl(_geometry(vp, "far", brick), cam, W, H, control_draw=True)
        assert t[..., :3].tobytes() == origin.tobytes() and np.median(segs[hit & decided]) == LC.CRAWL_CAP
        start = ((origin.astype(np.float64) - o) * d).sum(-1)           # where on the float64 ray the crawl ended
        # 700 additions to coordinates below 64, each rounded by at most half an ulp(64) = 1.9e-6, and as many rounded products
        # of 0.05: the origin lies within 700 * 2e-6 = 1.4e-3 of the float64 ray, against the certificate's margin of 3/4 cell = 0.047
        cut = hit & decided & (segs == LC.CRAWL_CAP)
        assert np.abs(start[cut] - 35.0).max() < 2e-3 and np.abs(origin - (o + d * start[..., None])).max() < 2e-3
    else:
        assert t[..., :3].tobytes() == np.broadcast_to(o, d.shape).astype(f32).tobytes()
        start = np.zeros_like(tmin)
    grid = oracle.julia(32)
    cells = LC.nonempty_cells(grid)
    bmin, bmax = LC.box_of(None, grid.shape)
    checked = walked = 0
    for y, x in zip(*np.nonzero(hit & decided & (t_left > 0))):
        t0, t1 = max(tmin[y, x], 0.0), min(start[y, x] + t_left[y, x], tmax[y, x])
        if cls[y, x] == 1:
            assert t_left[y, x] > 1e29
        if t1 <= t0:
            continue
        on_ray = LC.cells_on_ray(cells, bmin, bmax, o[y, x], d[y, x], t0, t1)
        assert not on_ray.any(), (y, x)
        checked += len(on_ray)
        walked += 1
    assert walked > 200 and checked > 20000 and (cls[hit] == 1).sum() > 20


# ------------------------------------------------------------------------------------------------------------- segment table
TABLE_CASES = [("long", c, b) for c in LC.LONG_CAMERAS for b in (1, 8)] + [("far", "d60", 1)]


@pytest.mark.parametrize("scene,camera,brick", TABLE_CASES)
def test_segment_table_is_the_restatement_bit_for_bit(vp, ctx, oracle, scene, camera, brick):
    """vp_get_segment_table: for every general pixel (in the order of vp_get_pixel_lists) the records (t_near, t_far, maximum byte |
    stop << 8, t_empty) and the segment origins up to the chain's stop record equal the numpy restatement of approach_segments_k,
    started at the restated crawl origin with the certified-empty distance of the pixel table.  long_box: at least 50 chains stop at
    record cap - 1 for no other reason than the cap, at least 20 earlier, for both early reasons.  The camera at 60 units: every
    chain reaches the cap OUTSIDE the box (the crawl was cut at 700 segments, 500 in front of it)."""
    _scene(vp, oracle, scene, camera, vp.EST_DECOMP, vp.RNG_PHILOX7, brick, late=False)
    P = vp.make_param(W, H)
    rec, org, cap = vp.segment_table(P)
    general = vp.pixel_lists(P)[0]
    assert cap >= 2 and rec.shape == (len(general), cap, 4) and org.shape == rec.shape
    assert cap == LC.SEG_CAP_ASSUMED, "tests/test_long_rays_cpu.py counts its chains under another cap than the library's: update SEG_CAP_ASSUMED"
    ys, xs = (general >> 16).astype(int), (general & 0xffff).astype(int)
    t = vp.pixel_table(P)
    assert (t[ys, xs, 5] == 0).all() and len(general) == (t[..., 5] == 0).sum()
    cam = _camera(scene, camera)
    geo = _geometry(vp, scene, brick)
    origin, _, _ = LC.crawl(geo, cam, W, H, control_draw=True)
    assert t[..., :3].tobytes() == origin.tobytes()
    _, d = DC.camera_rays(cam, W, H)
    want, want_org, count, why = LC.chain(geo, origin[ys, xs], d[ys, xs], t[ys, xs, 4], cap)
    assert np.isfinite(want).all() and np.isfinite(want_org).all()
    bad = [i for i in range(len(general)) if rec[i, :count[i]].tobytes() != want[i, :count[i]].tobytes()
           or org[i, :count[i], :3].tobytes() != want_org[i, :count[i]].tobytes() or org[i, :count[i], 3].any()]
    assert not bad, (len(bad), len(general), [(int(ys[i]), int(xs[i]), int(count[i])) for i in bad[:4]])
    capped, early = int((why == LC.STOP_CAP).sum()), int((count < cap).sum())
    print(f"\n{scene} {camera} brick {brick}: {len(general)} general pixels, cap {cap}: {capped} chains stopped by the cap alone, {early} earlier "
          f"({int(((why & LC.STOP_MISS) != 0).sum())} left the box, {int(((why & LC.STOP_MINIMUM) != 0).sum())} met a positive minimum)")
    if scene == "long":
        assert capped >= LC.MIN_CAPPED and early >= LC.MIN_EARLY, (capped, early)
        assert ((why & LC.STOP_MISS) != 0).sum() >= 10 and ((why & LC.STOP_MINIMUM) != 0).sum() >= 10
        meets = LC.meets_medium(LC.long_box(), LC.LONG_BOX, cam, W, H)
        assert (t[..., 5][meets] == 0).all(), "a ray that passes a non-empty cell is a general pixel"
    else:
        assert capped == len(general) > 100 and (want[:, :, 0] >= LC.SEGMENT).all()


def test_segment_table_hook_says_where_there_is_no_table(vp, oracle):
    """VP_E_STATE for float and binary16 volumes, the other estimators and VP_NO_APPROACH_TABLE=1"""
    P = vp.make_param(W, H)
    with _context(vp):
        for scene, est in (("long_f32", vp.EST_DECOMP), ("long_f16", vp.EST_DECOMP), ("long", vp.EST_GLOBAL), ("long", vp.EST_BOUNDED)):
            _scene(vp, oracle, scene, "axis", est, vp.RNG_PHILOX7, 1, late=False)
            with pytest.raises(vp.VolpathError, match="volpath error -2"):
                vp.segment_table(P)
        _scene(vp, oracle, "long", "axis", vp.EST_DECOMP, vp.RNG_PHILOX7, 1, late=False)
        assert vp.segment_table(P)[2] >= 2
    with _context(vp, VP_NO_APPROACH_TABLE="1"):
        _scene(vp, oracle, "long", "axis", vp.EST_DECOMP, vp.RNG_PHILOX7, 1, late=False)
        with pytest.raises(vp.VolpathError, match="volpath error -2"):
            vp.segment_table(P)


# ------------------------------------------------------------------------------------------------------------- long launches
def _long_launch(vp, oracle, monkeypatch, scene, camera, brick, density, rng_mode, table):
    first, n = LONG_FRAMES
    ref, cnt = _oracle(oracle, scene, camera, vp.EST_DECOMP, rng_mode, brick, density, first, n)
    assert (ref[..., 3] > 0).sum() > 100
    _scene(vp, oracle, scene, camera, vp.EST_DECOMP, rng_mode, brick, late=True)
    P = vp.make_param(W, H, density=density)
    what = dict(scene=scene, camera=camera, brick=brick, density=density, rng=rng_mode)
    buf = vp.DeviceBuffer(W, H)
    try:
        vp.render_frames(buf.ptr, first, n, P)
        _same(buf.download(), ref, what)
        assert vp.last_approach_mode() == 1 and vp.last_approach_table() == table, what
        assert _counting_launch(vp, buf, P, first, n, ref, cnt, what, monkeypatch, walk=True) == 1
        assert vp.last_approach_table() == table, what
    finally:
        buf.free()


# the camera on the axis: bricks 1 and 8 x densities 800 and 209 x sampler.h and Philox-7; the one from above: a diagonal of that cross
LONG_LAUNCHES = [("axis", b, d, r) for b in (1, 8) for d in (800.0, 209.0) for r in (0, 2)] + [("above", 8, 800.0, 0), ("above", 8, 800.0, 2),
                                                                                               ("above", 1, 209.0, 2), ("above", 1, 800.0, 2)]


@pytest.mark.parametrize("camera,brick,density,rng_mode", LONG_LAUNCHES)
def test_long_box_long_launch_reads_capped_chains(vp, ctx, oracle, monkeypatch, camera, brick, density, rng_mode):
    """70 frames of the decomposition estimator on long_box: approach_local_tab_k walks chains that end at the table's cap and hands
    over there (density 209: a majorant whose null collision is not neutral ends the walk at the first non-empty brick instead);
    image == oracle, the table was read, the counters with the walk tallied == oracle"""
    _long_launch(vp, oracle, monkeypatch, "long", camera, brick, density, rng_mode, table=1)


@pytest.mark.parametrize("rng_mode", [0, 2])
def test_far_long_launch_reads_a_chain_outside_the_box(vp, ctx, oracle, monkeypatch, rng_mode):
    """the same from 60 units: the crawl was cut at 700 segments, the chain's 96 records lie in front of the box and the integrator
    walks the remaining 400 segments to it"""
    _long_launch(vp, oracle, monkeypatch, "far", "d60", 1, 60.0, rng_mode, table=1)


@pytest.mark.parametrize("scene,camera,brick,density", [("long", "axis", 8, 800.0), ("far", "d60", 1, 60.0)])
def test_long_rays_through_render_kernel(vp, ctx, oracle, scene, camera, brick, density):
    """100 render_kernel calls, one frame each: the look-ahead's batches -- 64 frames and more from the third on -- read the
    segment table; the accumulator after the last call equals the oracle's"""
    ref, _ = _oracle(oracle, scene, camera, vp.EST_DECOMP, vp.RNG_PHILOX7, brick, density, 0, 100)
    _scene(vp, oracle, scene, camera, vp.EST_DECOMP, vp.RNG_PHILOX7, brick, late=True)
    P = vp.make_param(W, H, density=density)
    before = vp.lookahead_stats()[0]
    buf = vp.DeviceBuffer(W, H)
    try:
        read_table = 0
        for f in range(100):
            vp.render_kernel(buf.ptr, f, P)
            read_table |= vp.last_approach_table()
        _same(buf.download(), ref, (scene, camera))
        assert read_table == 1, "no look-ahead batch of 64 frames and more read the segment table"
        assert vp.lookahead_stats()[0] > before, "no look-ahead batch was launched"
    finally:
        buf.free()


# --------------------------------------------------------------------------------------------------------------------- knobs
KNOBS = [dict(VP_NO_APPROACH_TABLE="1"), dict(VP_NO_APPROACH="1"), dict(VP_APPROACH_STEPS="50"), dict(VP_APPROACH_STEPS="200")]
_FAST = {}


def _fast_reference(vp, oracle, scene, camera, brick, density):
    """the library's own fast-arithmetic render with every approach kernel switched off: computed once, shared, never written to"""
    k = (scene, camera, brick, density)
    if k not in _FAST:
        with _context(vp, VP_NO_APPROACH="1"):
            _FAST[k] = _render_long(vp, oracle, scene, camera, brick, density, vp.ARITH_FAST)[0]
            _FAST[k].setflags(write=False)
    return _FAST[k]


def _render_long(vp, oracle, scene, camera, brick, density, arith):
    first, n = LONG_FRAMES
    _scene(vp, oracle, scene, camera, vp.EST_DECOMP, vp.RNG_PHILOX7, brick, late=True, arith=arith)
    P = vp.make_param(W, H, density=density)
    buf = vp.DeviceBuffer(W, H)
    try:
        vp.render_frames(buf.ptr, first, n, P)
        assert vp.last_arithmetic() == arith
        return buf.download(), vp.last_approach_mode(), vp.last_approach_table()
    finally:
        buf.free()
        vp.set_arithmetic(vp.ARITH_EXACT)


@pytest.mark.parametrize("knob", KNOBS, ids=lambda k: "-".join(f"{a}={b}" for a, b in k.items()))
@pytest.mark.parametrize("scene,camera,brick,density", [("long", "above", 1, 800.0), ("far", "d60", 1, 60.0)])
def test_knobs_render_the_same_bits_on_long_rays(vp, oracle, knob, scene, camera, brick, density):
    """contexts created with the table off, with every approach kernel off, with the walk cut at 50 steps (before the table's cap)
    and at 200 (the cap first): 70 frames in the exact arithmetic == oracle, in the fast arithmetic == the library's own render
    without approach kernels"""
    first, n = LONG_FRAMES
    ref, _ = _oracle(oracle, scene, camera, vp.EST_DECOMP, vp.RNG_PHILOX7, brick, density, first, n)
    fast_ref = _fast_reference(vp, oracle, scene, camera, brick, density)
    assert np.isfinite(fast_ref).all() and (fast_ref[..., 3] > 0).sum() > 100
    with _context(vp, **knob):
        got, mode, table = _render_long(vp, oracle, scene, camera, brick, density, vp.ARITH_EXACT)
        _same(got, ref, (knob, "exact"))
        assert mode == (0 if "VP_NO_APPROACH" in knob else 1) and table == (1 if "VP_APPROACH_STEPS" in knob else 0), (knob, mode, table)
        got, mode, table = _render_long(vp, oracle, scene, camera, brick, density, vp.ARITH_FAST)
        _same(got, fast_ref, (knob, "fast"))
        assert mode == (0 if "VP_NO_APPROACH" in knob else 1) and table == (1 if "VP_APPROACH_STEPS" in knob else 0), (knob, mode, table)


# ------------------------------------------------------------------------------------- other volume formats and estimators
@pytest.mark.parametrize("scene,camera,brick", [("long_f32", "axis", 1), ("long_f16", "above", 8), ("long_f16", "axis", 1), ("long_f32", "above", 8)])
def test_float_long_box_walks_without_the_table(vp, ctx, oracle, monkeypatch, scene, camera, brick):
    """float32 and binary16 long_box, 70 frames: approach_local_k sets 110 and more segments up per sample (float bound tables have
    no segment table); image and counters == oracle"""
    _long_launch(vp, oracle, monkeypatch, scene, camera, brick, 800.0, vp.RNG_PHILOX7, table=0)


@pytest.mark.parametrize("density", [209.0, 950.0])
@pytest.mark.parametrize("camera", list(LC.LONG_CAMERAS))
def test_global_majorant_crosses_the_long_box(vp, ctx, oracle, monkeypatch, camera, density):
    """approach_k on long_box, frames 7..12: 5.5 units of empty space in front of the far blob are 209 * 5.5 = 1150 null
    collisions per ray, and 950 * 5.5 = 5200 at density 950.  Neither majorant's null collision in empty space is neutral (mode 2:
    the walked throughput is looked up by the number of steps); at 950 the number lies beyond the table's 4096 entries and the
    recurrence is run on from the last one."""
    first, n = 7, 6
    for rng_mode in (vp.RNG_SAMPLERH, vp.RNG_PHILOX7):
        ref, cnt = _oracle(oracle, "long", camera, vp.EST_GLOBAL, rng_mode, 1, density, first, n)
        assert (ref[..., 3] > 0).sum() > 100
        _scene(vp, oracle, "long", camera, vp.EST_GLOBAL, rng_mode, 1, late=False)
        P = vp.make_param(W, H, density=density)
        assert vp.null_collision_table(P, 2)[1] != 1.0, "this majorant's null collision is neutral: not a mode-2 case"
        what = dict(camera=camera, density=density, rng=rng_mode)
        buf = vp.DeviceBuffer(W, H)
        try:
            vp.render_frames(buf.ptr, first, n, P)
            _same(buf.download(), ref, what)
            assert vp.last_approach_mode() == 2, what
            assert _counting_launch(vp, buf, P, first, n, ref, cnt, what, monkeypatch, walk=False) == 0
            assert _counting_launch(vp, buf, P, first, n, ref, cnt, what, monkeypatch, walk=True) == 2
            # per ray: the samples of frame 7 that make more null collisions than the throughput table has entries (oracle's count)
            if density == 950.0 and rng_mode == vp.RNG_PHILOX7:
                sc = oracle.OracleScene(LC.long_box(), scenes.synthetic_env(), scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER, box=LC.LONG_BOX,
                                        estimator=oracle.EST_GLOBAL, rng_mode=rng_mode, seed=KEY, inv_view=LC.long_camera(camera))
                oP = oracle.default_param(W, H, density=density)
                far = LC.meets_medium(LC.long_box(), LC.LONG_BOX, LC.long_camera(camera), W, H) & (vp.pixel_table(P)[..., 5] == 0)
                lookups = np.array([sc.render_sample(oP, int(x), int(y), first)[1].as_dict()["density_lookups"] for y, x in zip(*np.nonzero(far))])
                assert (lookups > 4096 + 64).sum() >= 10, (len(lookups), int(lookups.max(initial=0)))
        finally:
            buf.free()
