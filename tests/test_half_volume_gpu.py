"""binary16 density volumes on the GPU (include/volpath.h vp_init_volume(VP_VOL_F16)).

THE DEFINITION under test: a binary16 volume h renders, in every mode, exactly what the float volume widen(h) = h.astype(float32)
renders.  Every comparison here is at tolerance 0, against the CPU oracle fed widen(h) or against the library itself fed widen(h).
The Python init_volume used to convert a float16 array to float32, so an image comparison alone would pass without the feature: every
test also asserts (_is_half) that the device holds 16-byte cells.  Each test runs in a context of its own."""
import ctypes as C

import numpy as np
import pytest

import scenes

pytestmark = pytest.mark.gpu

SHAPE = (7, 9, 13)            # nz, ny, nx: odd, no multiple of the 4^3 cell bricks or of any bound brick
SPECIALS = (0.0, -0.0, 2.0 ** -24, 3e-5, 6.1e-5, 0.333, 1.0, 1.5, 65504.0)   # smallest subnormal, a subnormal, just above 2^-14, ...
ENV = scenes.synthetic_env()
W, H = 24, 16


def special_grid():
    """13 x 9 x 7 halves: random values in [0, 1], the special values at the corners, on faces and inside, and an empty slab"""
    rng = np.random.default_rng(16)
    g = rng.random(SHAPE, dtype=np.float32).astype(np.float16)
    g[:, :, 9:11] = 0.0
    flat = g.reshape(-1)
    where = rng.permutation(flat.size)[:4 * len(SPECIALS)].reshape(len(SPECIALS), 4)
    for v, idx in zip(SPECIALS, where):
        flat[idx] = np.float16(v)
    g[0, 0, 0], g[0, 0, 1], g[0, 1, 0], g[1, 0, 0] = np.float16(2.0 ** -24), np.float16(-0.0), np.float16(3e-5), np.float16(6.1e-5)
    g[-1, -1, -1], g[-1, -1, -2] = np.float16(65504.0), np.float16(1.5)
    bits = g.view(np.uint16)
    assert {0x0000, 0x8000, 0x0001, 0x7bff, 0x3c00, 0x3e00} <= set(bits.reshape(-1).tolist())
    assert np.all(np.isfinite(g.astype(np.float32)))
    return np.ascontiguousarray(g)


def blob_grid(n=20):
    return np.ascontiguousarray(scenes.blob_volume_f32(n).astype(np.float16))


GRIDS = {"special": special_grid(), "blob": blob_grid()}
PARAM = {"special": dict(density=0.02, g=0.6), "blob": dict(density=300.0, g=0.877)}


def _param(name, est):
    """Param.density for the special grid: its 65504 is the local majorant of its bricks -- 0.02 keeps the walk there as long as 800
    does in a grid whose maximum is 1; the global majorant knows nothing of the grid's values: 5 gives its paths ~3000 fetches in four
    frames, and the throughput of those that meet the 1.5 and the 65504 (a density above the majorant) stays finite"""
    if name == "special" and est == 0:
        return dict(PARAM[name], density=5.0)
    return PARAM[name]


@pytest.fixture
def ctx(vp):
    c = vp.Context(0)
    try:
        with c:
            yield c
    finally:
        c.destroy()


def _env_ctx(vp, monkeypatch, name, value):
    """a context made while `name` is set (the knobs are read when a context is made)"""
    monkeypatch.setenv(name, value)
    c = vp.Context(0)
    monkeypatch.delenv(name)
    return c


def _is_half(vp, grid, padded=None):
    info = vp.volume_info()
    assert info["format"] == vp.VOL_F16 and info["cell_bytes"] == 16, info
    assert info["cells_bytes"] == 16 * (grid.size if padded is None else padded), info
    assert (info["nz"], info["ny"], info["nx"]) == grid.shape


def _is_float(vp, grid):
    info = vp.volume_info()
    assert info["format"] == vp.VOL_F32 and info["cell_bytes"] == 32 and info["cells_bytes"] == 32 * grid.size, info


def _scene(vp, grid, est, rng_mode, brick=1, linear=True, key=(11, 22), opacity=False, env_mis=False, track=0):
    vp.init_volume(grid, brick=brick, linear=linear)
    if grid.dtype == np.float16:
        _is_half(vp, grid)
    else:
        _is_float(vp, grid)
    vp.init_envmap(ENV)
    vp.set_sun(scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER)
    vp.set_camera()
    vp.set_estimator(est)
    vp.set_rng(rng_mode, key)
    vp.set_tracking(track)
    vp.set_envmap_sampling(vp.ENV_MIS if env_mis else vp.ENV_PASSIVE)
    vp.set_shard(0, 1)
    if opacity:
        vp.precompute_opacity(scenes.DEFAULT_SUN_DIR)


_ORACLE = {}


def _oracle_render(oracle, name, est, rng_mode, first, nframes, brick=1, env_mis=False, track=0, size=(W, H)):
    """the oracle's render of widen(h), computed once per configuration"""
    k = (name, est, rng_mode, first, nframes, brick, env_mis, track, size)
    if k not in _ORACLE:
        wide = np.ascontiguousarray(GRIDS[name].astype(np.float32))
        osc = oracle.OracleScene(wide, ENV, scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER, brick=brick, estimator=est, rng_mode=rng_mode,
                                 seed=(11, 22), env_mis=env_mis, track_mode=track)
        oP = oracle.default_param(size[0], size[1], **_param(name, est))
        if est == 1 and first + nframes - 1 > 10:
            osc.precompute_opacity()
        ref, cnt = None, None
        for f in range(first, first + nframes):
            ref, c = osc.render_frame(oP, f, ref)
            d = c.as_dict()
            cnt = d if cnt is None else {q: cnt[q] + d[q] for q in d}
        ref.setflags(write=False)
        _ORACLE[k] = (ref, cnt)
    return _ORACLE[k]


COUNTERS = ("samples", "density_lookups", "bound_lookups", "opacity_lookups", "env_lookups", "scatters")


# ---------------------------------------------------------------------------------------------------------------- the fetch
def _positions(n=50_000):
    """inside the box, on its faces (exactly), on texel centres and cell planes, and outside"""
    rng = np.random.default_rng(50)
    nz, ny, nx = SHAPE
    ext = np.array([1.0, ny / nx, nz / nx], np.float32)          # the default box is +-ext
    p = (rng.uniform(-1.0, 1.0, (n, 3)) * ext).astype(np.float32)
    q = n // 10
    face = rng.integers(0, 3, q)
    p[np.arange(q), face] = (np.where(rng.random(q) < 0.5, -1.0, 1.0) * ext[face]).astype(np.float32)        # on the faces
    p[q:2 * q] *= np.float32(1.3)                                                                           # partly outside
    p[2 * q:3 * q] = (rng.uniform(-3.0, 3.0, (q, 3))).astype(np.float32)                                    # mostly outside
    # texel centres and cell planes: ((i + 0.5) / n and i / n in box coordinates), where the weights are 0 and the `low` rule begins
    dims = np.array([nx, ny, nz])
    i = rng.integers(-1, dims + 2, (q, 3))
    half = rng.integers(0, 2, (q, 3)) * 0.5
    p[3 * q:4 * q] = (((i + half) / dims * 2.0 - 1.0) * ext).astype(np.float32)
    # the half texel below the first texel centre of each axis, where both taps are texel 0
    low = rng.uniform(0.0, 0.5, (q, 3)) / dims
    keep = rng.random((q, 3)) < 0.5
    p[4 * q:5 * q] = np.where(keep, p[4 * q:5 * q], ((low * 2.0 - 1.0) * ext)).astype(np.float32)
    return np.ascontiguousarray(p)


@pytest.mark.parametrize("linear", (True, False), ids=("linear", "point"))
@pytest.mark.parametrize("bricks", (0, 1), ids=("xfastest", "cellbricks"))
def test_fetch_point_by_point(vp, monkeypatch, bricks, linear):
    """vp_test_sample_density on the binary16 volume == the same call on widen(h), as bit patterns: a flushed subnormal, a lost sign
    of zero or a swapped tap shows here"""
    h = GRIDS["special"]
    pos = _positions()
    c = _env_ctx(vp, monkeypatch, "VP_CELL_BRICKS", str(bricks))
    try:
        with c:
            vp.init_volume(h, linear=linear)
            nz, ny, nx = SHAPE
            padded = ((nx + 3) // 4) * ((ny + 3) // 4) * ((nz + 3) // 4) * 64
            _is_half(vp, h, padded if bricks else None)
            got = vp.test_sample_density(pos)
            vp.init_volume(h.astype(np.float32), linear=linear)
            assert vp.volume_info()["format"] == vp.VOL_F32 and vp.volume_info()["cell_bytes"] == 32
            want = vp.test_sample_density(pos)
    finally:
        c.destroy()
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (bad.size, pos[bad[:4]], got[bad[:4]], want[bad[:4]])
    # the test means something: subnormal, huge and zero results occur (the sign of a zero is part of the bit patterns compared above)
    assert ((want != 0.0) & (np.abs(want) < 6e-5)).any() and (want > 1.0).any() and (want == 0.0).any()
    if not linear:
        assert (want == np.float32(2.0 ** -24)).any()        # the smallest subnormal comes through as it is


# --------------------------------------------------------------------------------------------------------------- the tables
def test_bound_and_opacity_tables_are_the_float_volumes(vp, ctx):
    for name, bricks in (("special", (1, 2, 8)), ("blob", (1, 2, 8))):
        h = GRIDS[name]
        for brick in bricks:
            vp.init_volume(h, brick=brick)
            _is_half(vp, h)
            th = vp.bound_table(quantized=False)
            vp.init_volume(h.astype(np.float32), brick=brick)
            tf = vp.bound_table(quantized=False)
            assert th[1:] == tf[1:] and th[0].shape == tf[0].shape
            assert th[0].tobytes() == tf[0].tobytes(), (name, brick)
    h = GRIDS["blob"]
    suns = (scenes.DEFAULT_SUN_DIR, (0.48, 0.6, 0.64))
    tabs = []
    for g in (h, h.astype(np.float32)):
        vp.init_volume(g)
        if g.dtype == np.float16:
            _is_half(vp, g)
        for s in suns:
            vp.precompute_opacity(s)
            tabs.append(vp.opacity_table(g.shape))
    assert tabs[0].tobytes() == tabs[2].tobytes() and tabs[1].tobytes() == tabs[3].tobytes()
    assert tabs[0].max() > 0 and tabs[0].tobytes() != tabs[1].tobytes()


# ---------------------------------------------------------------------------------------------------- renders against the oracle
def _render_all_ways(vp, oracle, name, est, rng_mode, env_mis=False, track=0):
    h = GRIDS[name]
    late = est == 1                                       # the decomposition estimator runs across its frame-11 switch
    first, nframes = (9, 4) if late else (0, 4)
    ref, cnt = _oracle_render(oracle, name, est, rng_mode, first, nframes, env_mis=env_mis, track=track)
    what = dict(grid=name, est=est, rng=rng_mode, env_mis=env_mis, track=track)
    _scene(vp, h, est, rng_mode, opacity=late, env_mis=env_mis, track=track)
    P = vp.make_param(W, H, **_param(name, est))
    buf = vp.DeviceBuffer(W, H)
    try:
        counted = not track                               # the float path has no counters in the scalar tracking kernels either
        vp.enable_counters(counted)
        vp.read_counters(reset=True)
        vp.render_frames(buf.ptr, first, nframes, P)      # batched
        got = buf.download()
        k = vp.read_counters()
        vp.enable_counters(False)
        assert np.array_equal(got, ref, equal_nan=True), (what, float(np.nanmax(np.abs(got - ref))))
        if counted:
            for q in COUNTERS:
                assert k[q] == cnt[q], (what, q, k[q], cnt[q])
        buf.reset()
        vp.render_frames(buf.ptr, first, nframes, P)      # batched, timed instance
        assert np.array_equal(buf.download(), ref, equal_nan=True), what
        buf.reset()
        for r in range(2):                                # frame by frame, two shards (disjoint tiles: the sum is exact)
            vp.set_shard(r, 2)
            for f in range(first, first + nframes):
                vp.render_kernel(buf.ptr, f, P)
        vp.set_shard(0, 1)
        assert np.array_equal(buf.download(), ref, equal_nan=True), what
        _is_half(vp, h)
    finally:
        vp.enable_counters(False)
        buf.free()
    assert np.isfinite(ref[..., :3]).all() and ref[..., :3].max() > 0


@pytest.mark.parametrize("name", ("special", "blob"))
@pytest.mark.parametrize("rng_mode", (0, 1, 2), ids=("samplerh", "philox", "philox7"))
@pytest.mark.parametrize("est", (0, 1, 2), ids=("global", "decomp", "bounded"))
def test_render_equals_the_oracle_on_the_widened_grid(vp, oracle, ctx, est, rng_mode, name):
    _render_all_ways(vp, oracle, name, est, rng_mode)


@pytest.mark.parametrize("est,rng_mode,env_mis,track", ((1, 0, True, 0), (0, 1, True, 0), (2, 1, True, 0),
                                                          (1, 1, False, 1), (0, 0, False, 2), (2, 1, False, 2), (1, 0, False, 2), (0, 1, False, 1)))
def test_mis_and_scalar_tracking_builds_equal_the_oracle(vp, oracle, ctx, est, rng_mode, env_mis, track):
    _render_all_ways(vp, oracle, "blob", est, rng_mode, env_mis=env_mis, track=track)


@pytest.mark.parametrize("est,dense_off", ((0, False), (0, True), (1, False), (1, True)))
def test_long_launch_equals_the_oracle(vp, oracle, monkeypatch, est, dense_off):
    """one launch of 64...100 frames: the approach walks run (global majorant: approach_k; decomposition: approach_local_k on the
    float bound table -- the segment table stays the uchar volumes').  dense_off: a context that never takes the volume for dense
    (VP_DENSE_PERCENT=101), so that the walk runs whatever the grid's fill."""
    h = GRIDS["blob"]
    size = (12, 8)
    first, nframes = (5, 70) if est == 1 else (0, 96)
    ref, cnt = _oracle_render(oracle, "blob", est, 1, first, nframes, brick=2 if est else 1, size=size)
    c = _env_ctx(vp, monkeypatch, "VP_DENSE_PERCENT", "101") if dense_off else vp.Context(0)
    try:
        with c:
            _scene(vp, h, est, 1, brick=2 if est else 1, opacity=est == 1)
            P = vp.make_param(size[0], size[1], **PARAM["blob"])
            buf = vp.DeviceBuffer(*size)
            try:
                vp.render_frames(buf.ptr, first, nframes, P)
                assert np.array_equal(buf.download(), ref, equal_nan=True), (est, dense_off)
                assert vp.last_approach_table() == 0           # the segment table is the uchar volumes'
                vp.enable_counters(True)
                vp.read_counters(reset=True)
                buf.reset()
                vp.render_frames(buf.ptr, first, nframes, P)
                k = vp.read_counters()
                vp.enable_counters(False)
                assert np.array_equal(buf.download(), ref, equal_nan=True), (est, dense_off)
                for q in COUNTERS:
                    assert k[q] == cnt[q], (est, dense_off, q, k[q], cnt[q])
                _is_half(vp, h)
            finally:
                vp.enable_counters(False)
                buf.free()
    finally:
        c.destroy()


# -------------------------------------------------------------------------------------- against the library's own float renders
def _twice(vp, name, fn, **scene):
    """fn() after the scene is set up on h and on widen(h)"""
    out = []
    for g in (GRIDS[name], np.ascontiguousarray(GRIDS[name].astype(np.float32))):
        _scene(vp, g, **scene)
        out.append(fn())
    return out


@pytest.mark.parametrize("rng_mode", (1, 2), ids=("philox", "philox7"))
@pytest.mark.parametrize("est", (0, 1), ids=("global", "decomp"))
def test_fast_arithmetic_equals_the_fast_render_of_the_widened_grid(vp, ctx, est, rng_mode):
    first, n = (9, 4) if est == 1 else (0, 4)
    P = vp.make_param(W, H, **PARAM["blob"])

    def render():
        vp.set_arithmetic(vp.ARITH_FAST)
        buf = vp.DeviceBuffer(W, H)
        try:
            vp.render_frames(buf.ptr, first, n, P)
            batched = buf.download()
            assert vp.last_arithmetic() == vp.ARITH_FAST
            buf.reset()
            for f in range(first, first + n):
                vp.render_kernel(buf.ptr, f, P)
            single = buf.download()
            buf.reset()
            vp.render_frames(buf.ptr, 0, 80, P) if est == 0 else vp.render_frames(buf.ptr, 5, 70, P)     # a long launch: the approach walk
            return batched, single, buf.download()
        finally:
            buf.free()

    (hb, hs, hl), (fb, fs, fl) = _twice(vp, "blob", render, est=est, rng_mode=rng_mode, opacity=est == 1)
    assert np.array_equal(hb, fb) and np.array_equal(hs, fs) and np.array_equal(hl, fl)
    assert np.array_equal(hb, hs), "batched and frame by frame differ in the fast mode"
    assert hb[..., :3].max() > 0


def test_statistics_adaptive_sampling_and_subpixel_sampling(vp, ctx):
    P = vp.make_param(W, H, **PARAM["blob"])

    def products():
        out = []
        buf, st = vp.DeviceBuffer(W, H), vp.StatsBuffer(W, H)
        try:
            vp.render_frames_stats(buf.ptr, st.ptr, 0, 6, P)
            out += [buf.download(), st.download().copy()]
            buf.reset(); st.reset()
            res = vp.render_adaptive(buf.ptr, st.ptr, 0, 24, P, rel_tol=0.25, min_frames=4, round_frames=4)
            rec = st.download().copy()
            out += [buf.download(), rec, res]
            vp.set_subpixel(2)
            buf.reset()
            vp.render_frames(buf.ptr, 0, 4, P)
            out.append(buf.download())
            vp.set_subpixel(1)
            return out
        finally:
            vp.set_subpixel(1)
            buf.free(); st.free()

    hp, fp = _twice(vp, "blob", products, est=0, rng_mode=1)
    assert np.array_equal(hp[0], fp[0]) and hp[1].tobytes() == fp[1].tobytes()                 # statistics: accumulator, records
    assert np.array_equal(hp[2], fp[2]) and hp[3].tobytes() == fp[3].tobytes() and hp[4] == fp[4]   # adaptive: + frozen set, result
    assert (hp[3]["n"] > 0).all()
    assert np.array_equal(hp[5], fp[5]) and not np.array_equal(hp[5], hp[0])                   # sub-pixel sampling


def test_init_cuda_after_a_binary16_volume_is_untouched(vp, oracle, ctx):
    """Part 1: init_cuda(float) directly after a binary16 volume renders what it renders in a fresh context -- the oracle's image"""
    name, est = "blob", 0
    ref, _ = _oracle_render(oracle, name, est, 1, 0, 4)
    h = GRIDS[name]
    wide = np.ascontiguousarray(h.astype(np.float32))
    _scene(vp, h, est, 1)
    P = vp.make_param(W, H, **_param(name, est))
    buf = vp.DeviceBuffer(W, H)
    try:
        vp.render_frames(buf.ptr, 0, 2, P)
        nz, ny, nx = wide.shape
        vp.lib().init_cuda(wide.ctypes.data_as(C.c_void_p), vp.Extent(nx, ny, nz), False, None, None)
        _is_float(vp, wide)
        buf.reset()
        vp.render_frames(buf.ptr, 0, 4, P)
        assert np.array_equal(buf.download(), ref)
        # ... and a uchar volume after it: the 8-byte cells, as ever
        q = scenes.blob_volume_u8(20)
        vp.lib().init_cuda(q.ctypes.data_as(C.c_void_p), vp.Extent(20, 20, 20), True, None, None)
        info = vp.volume_info()
        assert info["format"] == vp.VOL_U8 and info["cell_bytes"] == 8 and info["cells_bytes"] == 8 * q.size
    finally:
        buf.free()
