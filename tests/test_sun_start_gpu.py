"""The start of a sun shadow ray from the row of per-launch constants (csrc/vp_device.h sun_start; render_k start_shadow, stage 0).

1. Hook level (vp_test_sun_start): the start as built and as it stood, kept word for word in the test kernels, on scripted
   collision points -- direction, length, tnear, tfar and hit agree bit for bit in both arithmetic modes, for every sun and origin
   below; and the branches a wave of 64 consecutive origins took are the ones tests/sun_start_cases.py predicts from the operands'
   bits (finite suns: the prediction restates binary32 subtraction, multiplication and addition only, which the two modes share).
2. Image level: Julia 32^3, 24 x 16, frames 9..12, global majorant and decomposition, Philox2x32-7 and sampler.h: accumulators
   and work counters equal the CPU oracle's (tolerance 0), for the default box with each finite sun and for a box placed across the
   bench sun's absorption boundaries (|y| = 512, |z| = 128), where the lanes of a wave disagree.  The fast mode, which has no
   oracle: a staged launch equals frame-by-frame launches and two runs give equal bits (what tests/test_arith_fast_gpu.py promises).
"""
import contextlib

import numpy as np
import pytest

import scenes
import sun_start_cases as SC

pytestmark = pytest.mark.gpu

f32, u32 = np.float32, np.uint32
VP_E_ARG = -3


@contextlib.contextmanager
def _arith(vp, mode):
    vp.set_arithmetic(mode)
    try:
        yield
    finally:
        vp.set_arithmetic(vp.ARITH_EXACT)


# ----------------------------------------------------------------------------------------------------------------- origins
def _inside(rng, n, box=SC.DEFAULT_BOX):
    lo, hi = np.array(box[0], f32), np.array(box[1], f32)
    return (lo + (hi - lo) * rng.random((n, 3), dtype=f32)).astype(f32)


def _origins(seed=5):
    """{name: (origins [n, 3], box)}; n is never a multiple of 64 and spans several workgroups of 256"""
    rng = np.random.default_rng(seed)
    out = {}
    out["inside"] = (_inside(rng, 3001), SC.DEFAULT_BOX)
    # exactly +0 / -0 in one axis, a wave each per axis and sign (waves 0..5), then mixed waves
    z = _inside(rng, 64 * 6 + 2000 + 37)
    for a in range(3):
        z[64 * (2 * a):64 * (2 * a + 1), a] = 0.0
        z[64 * (2 * a + 1):64 * (2 * a + 2), a] = -0.0
    tail = z[64 * 6:]
    pick = rng.integers(0, 4, tail.shape)
    tail[pick == 0] = 0.0
    tail[pick == 1] = -0.0
    out["zeros"] = (z, SC.DEFAULT_BOX)
    # across the bench sun's absorption boundaries: |y| = 512 (half an ulp of end.y), |z| = 128 (of end.z)
    box = ((-1.0, 511.0, 127.0), (1.0, 513.0, 129.0))
    s = _inside(rng, 2500 + 19, box)
    s[:64, 1], s[:64, 2] = 511.5, 127.5                      # a wave wholly inside both
    s[64:128, 1], s[64:128, 2] = 512.5, 128.5                # ... wholly outside both
    s[128:192, 1], s[128:192, 2] = 511.5, 127.5              # ... inside, but for one odd lane in y
    s[128 + 17, 1] = 512.75
    s[192:256, 1], s[192:256, 2] = 511.5, 127.5              # ... and one odd lane in z (the last lane)
    s[255, 2] = 128.75
    s[256:320, 1], s[256:320, 2] = 512.0, 128.0              # ... exactly on the ties
    s[320:384] *= f32(-1.0)                                  # ... and the mirror image
    out["straddle"] = (s, box)
    # the default box with one odd lane far outside it in an otherwise constant wave (lane 0, lane 63, a middle lane)
    o = _inside(rng, 64 * 4 + 5)
    o[0] = (0.3, 600.0, 0.1)
    o[64 + 63] = (0.3, 0.2, -140.0)
    o[128 + 31] = (1.0e8, 0.0, 0.0)     # (its square is not absorbed: the length moves)
    out["odd_lane"] = (o, SC.DEFAULT_BOX)
    # far cameras' magnitudes
    m = (10.0 ** rng.uniform(5.0, 7.0, (2100 + 7, 3))).astype(f32) * rng.choice(np.array([-1.0, 1.0], f32), (2107, 3))
    out["far"] = (m.astype(f32), SC.DEFAULT_BOX)
    return out


def _suns():
    return {"bench": SC.bench_sun(), "oblique": SC.OBLIQUE, "plus_zero": SC.PLUS_ZERO, "minus_zero": SC.MINUS_ZERO, "tiny": SC.TINY,
            "nan": (float("nan"), 0.8, -0.6), "inf": (0.6, float("inf"), -0.8), "minus_inf": (0.6, 0.8, float("-inf"))}


FINITE = ("bench", "oblique", "plus_zero", "minus_zero", "tiny")


# -------------------------------------------------------------------------------------------------------------- hook level
@pytest.mark.parametrize("arith", [0, 1], ids=["exact", "fast"])
@pytest.mark.parametrize("sun", ["bench", "oblique", "plus_zero", "minus_zero", "tiny", "nan", "inf", "minus_inf"])
def test_start_equals_the_earlier_form_bit_for_bit(vp, sun, arith):
    direction = _suns()[sun]
    with _arith(vp, vp.ARITH_FAST if arith else vp.ARITH_EXACT):
        for name, (ro, box) in _origins().items():
            new, ref = vp.test_sun_start(ro, direction, np.array(box, f32).ravel())
            bad = np.argwhere(new[:, :7] != ref[:, :7])
            assert bad.size == 0, (sun, name, len(bad), bad[:4].tolist(), ro[bad[0, 0]].tolist(), new[bad[0, 0]].tolist(), ref[bad[0, 0]].tolist())
            assert (ref[:, 7] == 0).all()
            if sun in FINITE:
                want = SC.taken(direction, ro)
                diff = np.argwhere(new[:, 7] != want).ravel()
                assert diff.size == 0, (sun, name, "branches", int(diff[0]), int(new[diff[0], 7]), int(want[diff[0]]))


def test_the_branches_the_cases_are_there_for(vp):
    """what the cases above must exercise -- asserted on the hook's own report, not on the prediction alone"""
    cases = _origins()
    box = np.array(SC.DEFAULT_BOX, f32).ravel()
    # the bench sun inside the default box: length, factor, y and z read; x divided -- in every wave
    new, _ = vp.test_sun_start(cases["inside"][0], SC.bench_sun(), box)
    assert (new[:, 7] == (1 | 4 | 8)).all()
    assert (new[:, 6] == 1).mean() > 0.99   # (a ray from inside the box leaves it: a hit unless tfar < 1e-3)
    # the oblique sun: everything read
    new, _ = vp.test_sun_start(cases["inside"][0], SC.OBLIQUE, box)
    assert (new[:, 7] == 15).all()
    # +0 and -0: origins of exactly +0 in x keep the far end's bits under both suns; origins of -0 under the +0 sun only
    # (-0 - -0 is +0): the two suns take different branches on the same wave, and both matched above
    z = cases["zeros"][0]
    assert (SC.bits(z[:64, 0]) == 0).all() and (SC.bits(z[64:128, 0]) == 0x80000000).all()
    plus, _ = vp.test_sun_start(z, SC.PLUS_ZERO, box)
    minus, _ = vp.test_sun_start(z, SC.MINUS_ZERO, box)
    assert (plus[:64, 7] & 2).all() and (plus[64:128, 7] & 2).all()
    assert (minus[:64, 7] & 2).all() and not (minus[64:128, 7] & 2).any()
    assert not (plus[128:192, 7] & 2).any()   # a wave of non-zero x
    # across the boundaries: a wave inside reads y and z, a wave outside nothing, one odd lane sends its whole wave the general way
    s, sbox = cases["straddle"]
    new, _ = vp.test_sun_start(s, SC.bench_sun(), np.array(sbox, f32).ravel())
    assert (new[:64, 7] == 13).all() and (new[64:128, 7] & 12 == 0).all()
    assert (new[128:192, 7] & 4 == 0).all() and (new[192:256, 7] & 8 == 0).all()
    new, _ = vp.test_sun_start(cases["odd_lane"][0], SC.bench_sun(), box)
    assert (new[:64, 7] & 4 == 0).all() and (new[64:128, 7] & 8 == 0).all() and (new[128:192, 7] == 0).all() and (new[192:256, 7] == 13).all()


def test_hook_refuses_bad_arguments(vp):
    import ctypes as C
    L = vp.lib()
    ro, sun, box = np.zeros((1, 3), f32), np.array(SC.OBLIQUE, f32), np.array(SC.DEFAULT_BOX, f32).ravel()
    new, ref = np.zeros(8, u32), np.zeros(8, u32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.vp_test_sun_start(-1, p(ro), p(sun), p(box), p(new), p(ref)) == VP_E_ARG
    assert L.vp_test_sun_start(1, None, p(sun), p(box), p(new), p(ref)) == VP_E_ARG
    assert L.vp_test_sun_start(1, p(ro), None, p(box), p(new), p(ref)) == VP_E_ARG
    assert L.vp_test_sun_start(1, p(ro), p(sun), None, p(new), p(ref)) == VP_E_ARG
    assert L.vp_test_sun_start(1, p(ro), p(sun), p(box), None, p(ref)) == VP_E_ARG
    assert L.vp_test_sun_start(0, p(ro), p(sun), p(box), p(new), p(ref)) == 0


# ------------------------------------------------------------------------------------------------------------- image level
W, H, N = 24, 16, 32
FIRST, NFRAMES = 9, 4
KEY = (3, 4)
COUNTERS = ("samples", "density_lookups", "bound_lookups", "opacity_lookups", "env_lookups", "scatters")
# a box of the default size around (0, 512, 128): the bench sun's y and z differences change their bits inside it
OFF_CENTRE = ((-1.0, 511.0, 127.0), (1.0, 513.0, 129.0))
SCENES = [(s, "default") for s in FINITE] + [("bench", "off_centre")]


def _camera(vp, where):
    m = list(vp.DEFAULT_CAMERA)
    if where == "off_centre":
        m[7] = float(f32(m[7]) + f32(512.0))
        m[11] = float(f32(m[11]) + f32(128.0))
    return tuple(float(f32(v)) for v in m)


_ORACLE = {}


def _oracle(vp, oracle, sun, where, est, rng_mode):
    """(accumulator, summed counters): computed once per case, shared, never written to"""
    k = (sun, where, est, rng_mode)
    if k not in _ORACLE:
        direction = _suns()[sun]
        osc = oracle.OracleScene(oracle.julia(N), scenes.synthetic_env(), direction, scenes.DEFAULT_SUN_POWER, box=OFF_CENTRE if where == "off_centre" else None,
                                 estimator=est, rng_mode=rng_mode, seed=KEY, inv_view=_camera(vp, where))
        if est == oracle.EST_DECOMP:
            osc.precompute_opacity()
        oP = oracle.default_param(W, H)
        acc, cnt = None, None
        for f in range(FIRST, FIRST + NFRAMES):
            acc, c = osc.render_frame(oP, f, acc)
            d = c.as_dict()
            cnt = d if cnt is None else {q: cnt[q] + d[q] for q in d}
        assert np.isfinite(acc).all()
        acc.setflags(write=False)
        _ORACLE[k] = (acc, cnt)
    return _ORACLE[k]


def _setup(vp, oracle, sun, where, est, rng_mode):
    direction = _suns()[sun]
    vp.set_subpixel(1)
    vp.init_volume(oracle.julia(N), box=OFF_CENTRE if where == "off_centre" else None, brick=1, linear=True)
    vp.init_envmap(scenes.synthetic_env())
    vp.set_sun(direction, scenes.DEFAULT_SUN_POWER)
    vp.set_camera(_camera(vp, where))
    vp.set_estimator(est)
    vp.set_rng(rng_mode, KEY)
    vp.set_tracking(0)
    vp.set_envmap_sampling(vp.ENV_PASSIVE)
    vp.set_shard(0, 1)
    vp.enable_counters(False)
    if est == vp.EST_DECOMP:
        vp.precompute_opacity(direction)
    return vp.make_param(W, H)


@pytest.mark.parametrize("sun,where", SCENES, ids=[f"{s}-{w}" for s, w in SCENES])
@pytest.mark.parametrize("rng_mode", [2, 0], ids=["philox7", "samplerh"])
@pytest.mark.parametrize("est", [0, 1], ids=["global", "decomp"])
def test_images_and_work_equal_the_oracle(vp, oracle, est, rng_mode, sun, where):
    ref, cnt = _oracle(vp, oracle, sun, where, est, rng_mode)
    assert cnt["scatters"] > 1000, ("the scene starts too few shadow rays", cnt)
    P = _setup(vp, oracle, sun, where, est, rng_mode)
    buf = vp.DeviceBuffer(W, H)
    try:
        vp.render_frames(buf.ptr, FIRST, NFRAMES, P)
        got = buf.download()
        assert got.tobytes() == ref.tobytes(), (est, rng_mode, sun, where, int((got != ref).any(-1).sum()), float(np.abs(got - ref).max()))
        try:
            vp.enable_counters(True)
            vp.read_counters(reset=True)
            buf.reset()
            vp.render_frames(buf.ptr, FIRST, NFRAMES, P)
            k = vp.read_counters()
            got = buf.download()
        finally:
            vp.enable_counters(False)
        assert got.tobytes() == ref.tobytes(), (est, rng_mode, sun, where, "counting launch")
        for q in COUNTERS:
            print(q, k[q], cnt[q])
            assert k[q] == cnt[q], (est, rng_mode, sun, where, q, k[q], cnt[q])
    finally:
        buf.free()


@pytest.mark.parametrize("sun,where", SCENES, ids=[f"{s}-{w}" for s, w in SCENES])
@pytest.mark.parametrize("est", [0, 1], ids=["global", "decomp"])
def test_fast_mode_staged_equals_frame_by_frame_and_repeats(vp, oracle, est, sun, where):
    with _arith(vp, vp.ARITH_FAST):
        P = _setup(vp, oracle, sun, where, est, vp.RNG_PHILOX7)
        buf = vp.DeviceBuffer(W, H)
        try:
            vp.render_frames(buf.ptr, FIRST, NFRAMES, P)
            one = buf.download()
            assert vp.last_arithmetic() == vp.ARITH_FAST
            buf.reset()
            vp.render_frames(buf.ptr, FIRST, NFRAMES, P)
            assert buf.download().tobytes() == one.tobytes(), "two runs differ"
            buf.reset()
            for f in range(FIRST, FIRST + NFRAMES):
                vp.render_frames(buf.ptr, f, 1, P)
            assert buf.download().tobytes() == one.tobytes(), "staged and frame-by-frame launches differ"
            assert np.isfinite(one).all() and (one[..., 3] > 0).any()
        finally:
            buf.free()
