"""GPU parity on extreme media (tests/extreme_media.py): g = +-1 and both sides of the |g| > 1e-6f switch, dead, underflowing and
amplifying channels, media that are achromatic under == but not in bits, sigma_t with a zero channel, sigma_t' zero and subnormal.
Bar: the HIP path equals the CPU oracle bit for bit (np.array_equal(..., equal_nan=True), tolerance 0);
tests/test_extreme_media_cpu.py holds the oracle to the reference's own kernel code on every one of these media.

What the HIP path has beside the oracle's straight-line arithmetic and these media reach: the collision-constant rows (coll_row_fill:
div_(0.5, g) infinite at g = 0, rcp_(0) in the rows where the Hyperion reduction takes sigma_t' to 0 at g = 1), the in-range roots
behind the clamp of cos theta (0 / 0 at g = +-1: fmaxf(0, fminf(1, NaN)) is 1), the achromatic instance chosen with ==, the
identity checks of a null collision in empty space (light_identity_k, null_collision_is_identity, the null-collision table of
approach mode 2, the light class as constants) and the deferred light sum.  Which form ran is asserted from vp_last_approach_mode,
vp_last_light_const and vp_last_lds_form against numpy restatements of the checks.

The fast arithmetic is not oracle-defined: its tests assert what include/volpath.h promises and print the relative L2 against exact.
"""
import ctypes as C

import numpy as np
import pytest

import extreme_media as EM
import ref_cases as RC
import scenes

pytestmark = pytest.mark.gpu

KEY = (0x51ED270B, 77)
COUNTERS = ("samples", "density_lookups", "bound_lookups", "opacity_lookups", "env_lookups", "scatters")
FIRST, N = EM.FRAMES[0], len(EM.FRAMES)
assert EM.FRAMES == tuple(range(FIRST, FIRST + N))
ALL = EM.CASES + [EM.nudged(c) for c in EM.tagged("ach_compare")]
BY_NAME = {c["name"]: c for c in ALL}
VARIANT_CASES = [c["name"] for c in EM.CASES if set(c["tags"]) & {"g_pm1", "dead", "amplifying"}]
LONG_FRAMES = 64
f32 = np.float32


@pytest.fixture(scope="module")
def ctx(vp):
    """a context of this module's own: what is set here never reaches another module"""
    c = vp.Context(0)
    try:
        with c:
            yield c
    finally:
        c.destroy()


@pytest.fixture
def sparse_ctx(vp, monkeypatch):
    """a context that takes no volume for dense (the pattern of test_degenerate_long_launch_bit_exact): the approach walk runs"""
    monkeypatch.setenv("VP_DENSE_PERCENT", "101")
    c = vp.Context(0)
    monkeypatch.delenv("VP_DENSE_PERCENT")
    try:
        with c:
            yield c
    finally:
        c.destroy()


# ---------------------------------------------------------------------------------------------------------------- volumes
def _grid(name, oracle):
    if name == "blob_f16":
        return np.ascontiguousarray(scenes.blob_volume_f32().astype(np.float16))
    return RC.grid(name, oracle)


# ---------------------------------------------------------------------------------------------------------------- the oracle
_SCENES, _ORACLE = {}, {}


def _oracle(oracle, c, est, rng_mode, brick=1, first=FIRST, n=N, grid=None, variant="", size=None):
    """(accumulator, summed counters) of the oracle: computed once per case, shared, never written to.  One OracleScene per volume,
    brick size and build: the optical-depth table depends on none of Param, the estimator or the stream."""
    grid = grid or c["grid"]
    size = size or c["size"]
    k = (c["name"], est, rng_mode, brick, first, n, grid, variant, size)
    if k not in _ORACLE:
        sk = (grid, brick, variant)
        if sk not in _SCENES:
            _SCENES[sk] = oracle.OracleScene(_grid(grid, oracle), scenes.synthetic_env(), scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER,
                                             brick=brick, seed=KEY, env_mis=variant == "_mis", track_mode=RC.TRACK_OF_VARIANT[variant])
            _SCENES[sk].precompute_opacity()
        sc = _SCENES[sk]
        sc.S.estimator, sc.S.rng_mode = est, rng_mode
        P = oracle.default_param(size[0], size[1], **c["kw"])
        acc, cnt = None, None
        for f in range(first, first + n):
            acc, d = sc.render_frame(P, f, acc)
            d = d.as_dict()
            cnt = d if cnt is None else {q: cnt[q] + d[q] for q in d}
        assert oracle.lib().vpo_debug_shadow_overflow() == 0, k
        acc.setflags(write=False)
        _ORACLE[k] = (acc, cnt)
    return _ORACLE[k]


def _scene(vp, oracle, c, est, rng_mode, brick=1, grid=None, variant="", exit_mode=1):
    vp.set_arithmetic(vp.ARITH_EXACT)
    vp.set_subpixel(1)
    vp.init_volume(_grid(grid or c["grid"], oracle), brick=brick, linear=True)
    vp.init_envmap(scenes.synthetic_env())
    vp.set_sun(scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER)
    vp.set_camera()
    vp.set_estimator(est)
    vp.set_rng(rng_mode, KEY)
    vp.set_tracking(RC.TRACK_OF_VARIANT[variant])
    vp.set_envmap_sampling(vp.ENV_MIS if variant == "_mis" else vp.ENV_PASSIVE)
    vp.set_shard(0, 1)
    vp.set_exit_flights(exit_mode)
    vp.set_lookahead(vp.LOOKAHEAD_DEFAULT)
    vp.precompute_opacity(scenes.DEFAULT_SUN_DIR)


def _diff(got, ref):
    bad = np.argwhere(~((got == ref) | (np.isnan(got) & np.isnan(ref))))
    return len(bad), [(tuple(int(v) for v in b), float(got[tuple(b)]), float(ref[tuple(b)])) for b in bad[:4]]


def _both_ways(vp, P, ref, what, first=FIRST, n=N):
    """vp_render_frames frame by frame (direct accumulation) and as one staged batch of the same frames"""
    buf = vp.DeviceBuffer(P.width, P.height)
    try:
        for f in range(first, first + n):
            vp.render_frames(buf.ptr, f, 1, P)
        got = buf.download()
        assert np.array_equal(got, ref, equal_nan=True), (what, "frame by frame", _diff(got, ref))
        buf.reset()
        vp.render_frames(buf.ptr, first, n, P)
        got = buf.download()
        assert np.array_equal(got, ref, equal_nan=True), (what, "staged", _diff(got, ref))
        assert vp.last_arithmetic() == vp.ARITH_EXACT
    finally:
        buf.free()


def _streams(vp):
    return (vp.RNG_SAMPLERH, vp.RNG_PHILOX, vp.RNG_PHILOX7)


# ---------------------------------------------------------------------------------------------------------------- every case
@pytest.mark.parametrize("name", [c["name"] for c in ALL])
def test_extreme_medium_bit_exact(vp, ctx, oracle, name):
    """three estimators (the decomposition estimator with bricks of 1 and of 4) x sampler.h, Philox-10 and Philox-7, frames 10 and 11
    (the decomposition estimator's first read of the optical-depth table), frame by frame and staged.  Beside the table's cases the
    `_nudged` ones: an equal-by-compare medium with one albedo channel one ulp away -- the achromatic instance is chosen for the one,
    the chromatic instance for the other, and each is held to the oracle's render of its own medium"""
    c = BY_NAME[name]
    P = vp.make_param(*c["size"], **c["kw"])
    for est, brick in ((vp.EST_GLOBAL, 1), (vp.EST_DECOMP, 1), (vp.EST_DECOMP, 4), (vp.EST_BOUNDED, 1)):
        for rng_mode in _streams(vp):
            ref, _ = _oracle(oracle, c, est, rng_mode, brick)
            _scene(vp, oracle, c, est, rng_mode, brick)
            _both_ways(vp, P, ref, dict(case=name, est=est, brick=brick, rng=rng_mode))


# ------------------------------------------------------------------------------------------------------------- long launches
def null_collision_is_neutral(sigma_t_prime):
    """light_identity_k for one sigma_t' in numpy binary32: a null collision in empty space leaves a throughput of 1 at exactly 1"""
    with np.errstate(all="ignore"):
        sp = f32(sigma_t_prime)
        inv = f32(1) / sp
        m = abs(sp * f32(1))
        pn = (m + m) + m
        return bool(f32(1) * (sp * ((inv * pn) / pn)) == f32(1))


def expected_identity(kw, local, maxima=()):
    """the answer of light_identity_k: global majorant: the one sigma_t' of an unscattered path; local majorants: that of every byte
    that occurs as a maximum in the bound table"""
    p = EM.full(kw)
    s = f32(max(f32(0), min(f32(1), f32(-5) * f32(0.066666666666666666667))))
    max_sig = max(f32(v) for v in p["sigma_t"])
    d, g = f32(p["density"]), f32(p["g"])
    with np.errstate(all="ignore"):
        if not local:
            return null_collision_is_neutral(max_sig * ((f32(1) - s) * d + s * d * (f32(1) - g)))
        cur = ((f32(1) - s) + s * (f32(1) - g)) * d
        return all(null_collision_is_neutral(max_sig * cur * max(f32(0.0001), f32(int(b)) * f32(0.003921569))) for b in maxima)


LONG = [(c["name"], est) for c in EM.tagged("long") for est in (0, 1)]
_GLOBAL_IDENTITY = {c["name"]: expected_identity(c["kw"], False) for c in EM.tagged("long")}
# static, from the restatement: among the long cases the global majorant's walk runs in mode 1 (neutral) and in mode 2 (looked up), and
# the light class is written as constants (neutral) and integrated (not); every test below asserts its own case's answers and mode 0
assert set(_GLOBAL_IDENTITY.values()) == {True, False}, _GLOBAL_IDENTITY


@pytest.mark.parametrize("name,est", LONG)
def test_extreme_medium_long_launch_bit_exact(vp, oracle, sparse_ctx, name, est):
    """one launch of 64 frames at 16x12: Philox-7 and sampler.h, exit flights 0, 1 and 2; the approach walk runs (mode 1, or 2 where
    the global majorant's null collision is not neutral: then render_k looks the walked throughput up in the null-collision table);
    a counting launch walks itself (mode 0) and does the oracle's work"""
    c = BY_NAME[name]
    P = vp.make_param(*c["size"], **c["kw"])
    buf = vp.DeviceBuffer(*c["size"])
    try:
        for rng_mode in (vp.RNG_PHILOX7, vp.RNG_SAMPLERH):
            ref, cnt = _oracle(oracle, c, est, rng_mode, 1, 0, LONG_FRAMES)
            for exit_mode in (0, 1, 2):
                _scene(vp, oracle, c, est, rng_mode, 1, exit_mode=exit_mode)
                buf.reset()
                vp.render_frames(buf.ptr, 0, LONG_FRAMES, P)
                got = buf.download()
                mode, const, lds = vp.last_approach_mode(), vp.last_light_const(), vp.last_lds_form()
                what = dict(case=name, est=est, rng=rng_mode, exit=exit_mode, mode=mode, light_const=const, lds_form=lds)
                assert np.array_equal(got, ref, equal_nan=True), (what, _diff(got, ref))
                n_light = len(vp.pixel_lists(P)[1])
                maxima = np.unique(vp.bound_table()[0][..., 0])
                identity = expected_identity(c["kw"], est != vp.EST_GLOBAL, maxima)
                assert mode == (1 if est == vp.EST_DECOMP or identity else 2), what
                assert n_light > 0 and const == identity, (what, n_light)
                if est == vp.EST_DECOMP:     # 32^3 byte pairs fit LDS: codes for the counter-based stream, global memory for sampler.h
                    assert lds == (2 if rng_mode == vp.RNG_PHILOX7 else 0), what
                    assert vp.last_approach_table() == 1, what
            vp.enable_counters(True)
            vp.read_counters(reset=True)
            buf.reset()
            vp.render_frames(buf.ptr, 0, LONG_FRAMES, P)
            k = vp.read_counters()
            vp.enable_counters(False)
            got = buf.download()
            assert np.array_equal(got, ref, equal_nan=True), (name, est, rng_mode, "counting launch", _diff(got, ref))
            assert vp.last_approach_mode() == 0 and not vp.last_light_const()
            for q in COUNTERS:
                assert k[q] == cnt[q], (name, est, rng_mode, q, k[q], cnt[q])
    finally:
        vp.enable_counters(False)
        buf.free()


# --------------------------------------------------------------------------------------------------------- other render paths
@pytest.mark.parametrize("est", (0, 1))
@pytest.mark.parametrize("name", ("g_one", "albedo_subnormal"))
def test_render_kernel_with_lookahead_equals_render_frames(vp, ctx, oracle, name, est):
    """the reference's call pattern, one render_kernel per frame with the frame look-ahead (256) on, over frames 0..23"""
    c = BY_NAME[name]
    n = 24
    ref, _ = _oracle(oracle, c, est, vp.RNG_PHILOX7, 1, 0, n)
    P = vp.make_param(*c["size"], **c["kw"])
    _scene(vp, oracle, c, est, vp.RNG_PHILOX7)
    vp.set_lookahead(256)
    a, b = vp.DeviceBuffer(*c["size"]), vp.DeviceBuffer(*c["size"])
    try:
        for f in range(n):
            vp.render_kernel(a.ptr, f, P)
        got = a.download()
        vp.render_frames(b.ptr, 0, n, P)
        staged = b.download()
        assert np.array_equal(got, staged, equal_nan=True), (name, est, _diff(got, staged))
        assert np.array_equal(got, ref, equal_nan=True), (name, est, _diff(got, ref))
    finally:
        a.free()
        b.free()


@pytest.mark.parametrize("variant", ("_mis", "_scalar", "_multichannel"))
@pytest.mark.parametrize("name", VARIANT_CASES)
def test_extreme_medium_other_builds_bit_exact(vp, ctx, oracle, name, variant):
    """active environment sampling (MIS), scalar tracking and one channel per sample on g = +-1, the dead channel and the amplifying
    medium: three estimators, sampler.h and Philox-10 (Philox-7 is the shipped build's only)"""
    c = BY_NAME[name]
    P = vp.make_param(*c["size"], **c["kw"])
    try:
        for est in (vp.EST_GLOBAL, vp.EST_DECOMP, vp.EST_BOUNDED):
            for rng_mode in (vp.RNG_SAMPLERH, vp.RNG_PHILOX):
                ref, _ = _oracle(oracle, c, est, rng_mode, variant=variant)
                _scene(vp, oracle, c, est, rng_mode, variant=variant)
                _both_ways(vp, P, ref, dict(case=name, variant=variant, est=est, rng=rng_mode))
    finally:
        vp.set_tracking(vp.TRACK_SPECTRAL)
        vp.set_envmap_sampling(vp.ENV_PASSIVE)


@pytest.mark.parametrize("grid", ("blob_u8", "blob_f32", "blob_f16"))
@pytest.mark.parametrize("name", ("g_minus_one", "albedo_subnormal", "sigma_t_zero_channel"))
def test_extreme_medium_on_other_volumes_bit_exact(vp, ctx, oracle, name, grid):
    """a soft uchar volume, a float volume and a binary16 volume (the float kernels: no brick codes, no byte mask for the identity
    checks): global majorant and decomposition, Philox-7 and sampler.h"""
    c = BY_NAME[name]
    P = vp.make_param(*c["size"], **c["kw"])
    for est in (vp.EST_GLOBAL, vp.EST_DECOMP):
        for rng_mode in (vp.RNG_PHILOX7, vp.RNG_SAMPLERH):
            ref, _ = _oracle(oracle, c, est, rng_mode, grid=grid)
            assert (ref[..., 3] > 0).any(), (name, grid, "no sample met the medium")
            _scene(vp, oracle, c, est, rng_mode, grid=grid)
            _both_ways(vp, P, ref, dict(case=name, grid=grid, est=est, rng=rng_mode))


# ------------------------------------------------------------------------------------------------ the NaN before the clamp
NAN_CLAMP_SIZE, NAN_CLAMP_FRAMES = EM.NAN_CLAMP_SIZE, EM.NAN_CLAMP_FRAMES     # (found with the stream key KEY)
assert KEY == EM.NAN_CLAMP_KEY


@pytest.mark.parametrize("rng_mode,frame", [(r, f) for r in sorted(NAN_CLAMP_FRAMES) for f in NAN_CLAMP_FRAMES[r]])
def test_nan_before_the_clamp_bit_exact(vp, ctx, oracle, rng_mode, frame):
    """g = 1 and a draw of exactly 0: cos(theta) is 0 / 0 before the clamp of the phase-function sample makes it 1 (the frames:
    tests/extreme_media.py NAN_CLAMP_FRAMES); the frame alone, and staged with the frame before it"""
    c = dict(BY_NAME["g_one"], size=NAN_CLAMP_SIZE)
    before = oracle.lib().vpo_debug_hg_nan_clamp()
    ref, _ = _oracle(oracle, c, vp.EST_GLOBAL, rng_mode, 1, frame, 1)
    assert oracle.lib().vpo_debug_hg_nan_clamp() > before, "this frame no longer clamps a NaN"
    pair, _ = _oracle(oracle, c, vp.EST_GLOBAL, rng_mode, 1, frame - 1, 2)
    P = vp.make_param(*NAN_CLAMP_SIZE, **c["kw"])
    _scene(vp, oracle, c, vp.EST_GLOBAL, rng_mode)
    _both_ways(vp, P, ref, dict(frame=frame, rng=rng_mode), frame, 1)
    _both_ways(vp, P, pair, dict(frames=(frame - 1, frame), rng=rng_mode), frame - 1, 2)


def test_phase_function_helper_on_extreme_g(vp, oracle):
    """vp_test_hg (HGPhaseFunction::sample through Frame, ::evaluate) against the oracle's, bit for bit, NaN for NaN: g = +-1, +-0.999,
    the six neighbours of +-1e-6f, 1e-7, +-0; first variates 0 (0 / 0 at g = 1), the smallest and the largest draw, 1/2"""
    gs = sorted({float(c["kw"]["g"]) for c in EM.CASES if c["group"] == "g"} | {0.0})
    r0s = (0.0, float(2.0 ** -23), 0.5, float(1 - 2.0 ** -23))
    normals = ((0.0, 0.0, 1.0), (0.6, 0.0, 0.8), (0.05, -0.8, 0.6))
    rows = [(g, r0, r1, n, cq) for g in gs + [-0.0] for r0 in r0s for r1 in (0.0, 0.3) for n in normals for cq in (-1.0, 0.25, 1.0)]
    g, r0, r1, n, cq = (np.array([r[i] for r in rows], f32) for i in range(5))
    d, ev = vp.test_hg(g, r0, r1, n, cq)
    L = oracle.lib()
    want_d, want_ev = np.empty_like(d), np.empty_like(ev)
    for i in range(len(rows)):
        out = (C.c_float * 3)()
        L.vpo_hg_sample(float(g[i]), (C.c_float * 3)(*[float(v) for v in n[i]]), float(r0[i]), float(r1[i]), out)
        want_d[i] = out[:]
        want_ev[i] = L.vpo_hg_eval(float(g[i]), float(cq[i]))
    assert np.array_equal(d, want_d, equal_nan=True), _diff(d, want_d)
    assert np.array_equal(ev, want_ev, equal_nan=True), _diff(ev, want_ev)
    clamped = (g == 1.0) & (r0 == 0.0)
    assert clamped.any() and np.isfinite(want_d[clamped]).all()        # cos(theta) = 1: the direction is the normal's


# ----------------------------------------------------------------------------------------------------- null-collision table
@pytest.mark.parametrize("name", EM.NAMES)
def test_null_collision_table_on_extreme_media(vp, name):
    """vp_get_null_collision_table against the numpy binary32 restatement of tests/test_pins_gpu.py
    (test_null_collision_table_is_the_float32_recurrence), for every medium of the table: sigma_t' = 0 gives 1, NaN, NaN, ...;
    sigma_t' subnormal (its reciprocal overflows) 1, inf, NaN, ...  The expected values are what the restatement gives."""
    p = EM.full(BY_NAME[name]["kw"])
    n = 4200        # beyond the 4096 entries the kernel keeps
    got = vp.null_collision_table(vp.make_param(8, 8, **BY_NAME[name]["kw"]), n)
    ref = EM.null_collision_recurrence(p["sigma_t"], p["density"], p["g"], n)
    assert np.array_equal(got, ref, equal_nan=True), (name, int(np.argmax(~((got == ref) | (np.isnan(got) & np.isnan(ref))))))
    assert got[0] == 1.0
    if name == "sigma_t_zero":
        assert np.isnan(got[1:]).all()
    if name == "density_1e-40":
        assert np.isinf(got[1]) and np.isnan(got[2:]).all()


# ----------------------------------------------------------------------------------------------------------- fast arithmetic
@pytest.mark.parametrize("name", EM.NAMES)
def test_extreme_medium_fast_arithmetic(vp, ctx, oracle, name):
    """include/volpath.h's promise for VP_ARITH_FAST (Philox-7, global majorant and decomposition, frames 10 and 11): two runs give the
    same bits, a staged run equals a frame-by-frame run, the pixels of classes 1 and 2 are bit-identical to the exact mode, and
    where the exact image is finite so is the fast one.  No tolerance: the relative L2 against exact is printed."""
    c = BY_NAME[name]
    P = vp.make_param(*c["size"], **c["kw"])
    buf = vp.DeviceBuffer(*c["size"])

    def render(mode, staged):
        vp.set_arithmetic(mode)
        buf.reset()
        if staged:
            vp.render_frames(buf.ptr, FIRST, N, P)
        else:
            for f in range(FIRST, FIRST + N):
                vp.render_frames(buf.ptr, f, 1, P)
        assert vp.last_arithmetic() == mode, (name, "this configuration has no fast kernels")
        return buf.download()

    try:
        for est in (vp.EST_GLOBAL, vp.EST_DECOMP):
            _scene(vp, oracle, c, est, vp.RNG_PHILOX7)
            exact = render(vp.ARITH_EXACT, True)
            fast = render(vp.ARITH_FAST, True)
            again = render(vp.ARITH_FAST, True)
            single = render(vp.ARITH_FAST, False)
            cls = vp.pixel_table(P)[..., 5].astype(int)
            assert np.array_equal(fast, again, equal_nan=True), (name, est, "two runs differ")
            assert np.array_equal(fast, single, equal_nan=True), (name, est, "staged differs from frame by frame", _diff(fast, single))
            assert np.array_equal(fast[cls != 0], exact[cls != 0], equal_nan=True), (name, est)
            assert np.isfinite(fast[np.isfinite(exact)]).all(), (name, est)
            rgb = np.isfinite(exact[..., :3]) & np.isfinite(fast[..., :3])
            den = float(np.sqrt((exact[..., :3][rgb].astype(np.float64) ** 2).sum()))
            num = float(np.sqrt(((fast[..., :3][rgb].astype(np.float64) - exact[..., :3][rgb]) ** 2).sum()))
            print(f"\nfast arithmetic {name} est {est}: relative L2 against exact {num / den if den else 0.0:.3e} (2 frames, 16x12)", end="")
    finally:
        vp.set_arithmetic(vp.ARITH_EXACT)
        buf.free()
