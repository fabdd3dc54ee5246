"""GPU suite: the NL-means filter of the output stage (include/volpath.h vp_denoise).

The filter is DEFINED to the bit; tests/denoise_lib.py restates the definition in numpy, and every comparison here is tobytes()
equality of all four channels against it: on uploaded synthetic buffers (no render), with a separate guide pair, in both forms of the
kernel, and behind renders queued on the same stream, fed with the CPU oracle's frames."""
import numpy as np
import pytest

import adaptive_lib as A
import denoise_lib as D
import scenes

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (5, 3), (16, 16), (17, 9), (70, 37)]     # 70 x 37: no multiple of the tile either way; halos larger than the small images
PARAMS = [(0, 0), (1, 0), (2, 1), (5, 2)]
KS = (0.45, 2.0)
NAN_PATTERN = np.uint32(0x7FC12345)


@pytest.fixture(autouse=True)
def _restore(vp):
    yield
    vp.set_denoise_form(0)
    vp.set_arithmetic(vp.ARITH_EXACT)
    vp.set_subpixel(1)
    vp.set_shard(0, 1)
    vp.set_camera()


class Pair:
    """an accumulator and its records on the device"""

    def __init__(self, vp, acc, rec):
        H, W = rec.shape
        self.acc, self.rec = np.ascontiguousarray(acc, np.float32), np.ascontiguousarray(rec, vp.PIXEL_STATS_DTYPE)
        self.buf, self.stats = vp.DeviceBuffer(W, H), vp.StatsBuffer(W, H)
        self.buf.upload(self.acc)
        self.stats.upload(self.rec)

    def untouched(self):
        return self.buf.download().tobytes() == self.acc.tobytes() and self.stats.download().tobytes() == self.rec.tobytes()

    def free(self):
        self.buf.free(); self.stats.free()


def _run(vp, dst, src, W, H, R, F, k, guide=None):
    """one call into a NaN-filled dst; returns the downloaded image"""
    nan = np.full((H, W, 4), NAN_PATTERN, np.uint32).view(np.float32)
    dst.upload(nan)
    if guide is None:
        vp.denoise(dst.ptr, src.buf.ptr, src.stats.ptr, W, H, R, F, k)
    else:
        vp.denoise(dst.ptr, src.buf.ptr, src.stats.ptr, W, H, R, F, k, guide_ptr=guide.buf.ptr, guide_stats_ptr=guide.stats.ptr)
    return dst.download()


_memo = {}


def _synthetic(W, H, seed):
    key = ("in", W, H, seed)
    if key not in _memo:
        _memo[key] = D.synthetic(W, H, seed)
    return _memo[key]


def _want(W, H, seed, R, F, k, gseed=None):
    """the restatement's answer for the synthetic pair `seed` (guided by the pair `gseed`), computed once"""
    key = ("out", W, H, seed, R, F, k, gseed)
    if key not in _memo:
        acc, rec = _synthetic(W, H, seed)
        g = _synthetic(W, H, gseed) if gseed is not None else (None, None)
        _memo[key] = D.denoise(acc, rec, R, F, k, guide=g[0], guide_rec=g[1])
    return _memo[key]


def _params(W, H):
    return [(R, F, k) for R, F in PARAMS + ([(10, 3)] if (W, H) == (70, 37) else []) for k in KS]


# ---- 1. uploaded synthetic buffers, no render (and no scene: the call works before init_cuda)
@pytest.mark.parametrize("W,H", SIZES)
def test_synthetic_buffers_equal_the_restatement(vp, W, H):
    acc, rec = _synthetic(W, H, 100 + W)
    if W * H > 64:
        v = D.variance(rec)
        assert (rec["n"] == 0).any() and (rec["n"] == 1).any() and (rec["n"] >= 2).any()
        assert (v == 0).any() and (v > 0).any() and (rec["flags"] & 1).any() and not (rec["flags"] & 1).all()
        y = A.luminance(D.mean_image(acc, rec["n"])[0])[rec["n"] > 0]
        assert y.min() < 1e-3 and y.max() > 1e4
    src = Pair(vp, acc, rec)
    dst = vp.DeviceBuffer(W, H)
    try:
        for R, F, k in _params(W, H):
            got = _run(vp, dst, src, W, H, R, F, k)
            assert vp.last_denoise_form() == 0
            assert not np.isnan(got).any(), (R, F, k)             # dst is fully overwritten
            assert got.tobytes() == _want(W, H, 100 + W, R, F, k).tobytes(), (W, H, R, F, k)
        assert src.untouched()
    finally:
        src.free(); dst.free()


# ---- 2. the guide pair
@pytest.mark.parametrize("W,H", [(17, 9), (70, 37)])
def test_guide_pair_swapped_and_explicit_self_guide(vp, W, H):
    a, b = Pair(vp, *_synthetic(W, H, 7)), Pair(vp, *_synthetic(W, H, 8))
    dst = vp.DeviceBuffer(W, H)
    try:
        for R, F, k in ((2, 1, 0.45), (5, 2, 2.0)):
            ab = _run(vp, dst, a, W, H, R, F, k, guide=b)
            ba = _run(vp, dst, b, W, H, R, F, k, guide=a)
            assert ab.tobytes() == _want(W, H, 7, R, F, k, gseed=8).tobytes(), ("a guided by b", R, F, k)
            assert ba.tobytes() == _want(W, H, 8, R, F, k, gseed=7).tobytes(), ("b guided by a", R, F, k)
            own = _run(vp, dst, a, W, H, R, F, k)
            assert own.tobytes() == _want(W, H, 7, R, F, k).tobytes()
            assert ab.tobytes() != own.tobytes()                  # the guide matters
            assert _run(vp, dst, a, W, H, R, F, k, guide=a).tobytes() == own.tobytes()   # guide == src given explicitly
        assert a.untouched() and b.untouched()                    # src, records and guide: byte-identical after the calls
    finally:
        a.free(); b.free(); dst.free()


# ---- 3. both forms
def test_plain_form_equals_tiled_form_equals_the_restatement(vp):
    W, H = 70, 37
    src, gd = Pair(vp, *_synthetic(W, H, 100 + W)), Pair(vp, *_synthetic(W, H, 8))
    dst = vp.DeviceBuffer(W, H)
    try:
        for R, F, k in _params(W, H):
            out = {}
            for form in (1, 0):
                vp.set_denoise_form(form)
                out[form] = _run(vp, dst, src, W, H, R, F, k)
                assert vp.last_denoise_form() == form
            assert out[1].tobytes() == out[0].tobytes() == _want(W, H, 100 + W, R, F, k).tobytes(), (R, F, k)
        vp.set_denoise_form(1)
        assert _run(vp, dst, src, W, H, 5, 2, 2.0, guide=gd).tobytes() == _want(W, H, 100 + W, 5, 2, 2.0, gseed=8).tobytes()
        assert vp.last_denoise_form() == 1
        assert src.untouched() and gd.untouched()
    finally:
        src.free(); gd.free(); dst.free()


# ---- 4. behind renders on the same stream
def _scene(vp, est, rng_mode, key):
    vp.set_subpixel(1)
    vp.init_volume(vp.julia_volume(32), brick=1, linear=True)
    vp.init_envmap(scenes.synthetic_env())
    vp.set_sun(scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER)
    vp.set_camera()
    vp.set_estimator(est)
    vp.set_tracking(0)
    vp.set_envmap_sampling(vp.ENV_PASSIVE)
    vp.set_shard(0, 1)
    vp.set_rng(rng_mode, key)
    if est == vp.EST_DECOMP:
        vp.precompute_opacity(scenes.DEFAULT_SUN_DIR)


def _oracle_scene(oracle, est, rng_mode, key):
    osc = oracle.OracleScene(oracle.julia(32), scenes.synthetic_env(), scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER, estimator=est, rng_mode=rng_mode,
                             seed=key)
    if est == oracle.EST_DECOMP:
        osc.precompute_opacity()
    return osc


@pytest.mark.parametrize("est,rng_mode", [(0, 2), (1, 0)], ids=["global-philox7", "decomp-samplerh"])
def test_rendered_frames_then_denoise_without_a_synchronise(vp, oracle, est, rng_mode):
    W, H = A.ANCHOR_W, A.ANCHOR_H
    osc = _oracle_scene(oracle, est, rng_mode, (1, 2))
    st = A.render_uniform(A.Stats(W, H), A.oracle_frames(osc, oracle.default_param(W, H)), 0, 16)
    rec = st.records()
    assert (D.variance(rec) > 0).sum() > 200
    _scene(vp, est, rng_mode, (1, 2))
    P = vp.make_param(W, H)
    buf, stats, dst = vp.DeviceBuffer(W, H), vp.StatsBuffer(W, H), vp.DeviceBuffer(W, H)
    try:
        for R, F, k in ((5, 1, 0.45), (3, 2, 0.7)):
            buf.reset(); stats.reset()
            vp.render_frames_stats(buf.ptr, stats.ptr, 0, 16, P)
            vp.denoise(dst.ptr, buf.ptr, stats.ptr, W, H, R, F, k)       # queued behind the render: nothing waits in between
            got = dst.download()
            want = D.denoise(st.acc, rec, R, F, k)
            assert got.tobytes() == want.tobytes(), (R, F, k)
            assert buf.download().tobytes() == st.acc.tobytes()
        # the filter's bits do not depend on the arithmetic mode of the renders: the same buffers, the same answer
        vp.set_arithmetic(vp.ARITH_FAST)
        vp.denoise(dst.ptr, buf.ptr, stats.ptr, W, H, 3, 2, 0.7)
        assert dst.download().tobytes() == want.tobytes()
    finally:
        buf.free(); stats.free(); dst.free()


def test_adaptive_render_then_denoise(vp, oracle):
    """varying n per pixel and FROZEN bits: the second anchor of the adaptive-sampling tests"""
    W, H, a = A.ANCHOR_W, A.ANCHOR_H, A.ANCHOR2
    osc, oP = A.anchor_oracle(oracle, scenes, a)
    st = A.Stats(W, H)
    A.render_adaptive(st, A.oracle_frames(osc, oP), 0, a["max_frames"], **A.anchor_args(a))
    assert np.unique(st.n).size > 3 and (st.flags & 1).any()
    _scene(vp, vp.EST_DECOMP, vp.RNG_PHILOX7, a["key"])
    P = vp.make_param(W, H)
    buf, stats, dst = vp.DeviceBuffer(W, H), vp.StatsBuffer(W, H), vp.DeviceBuffer(W, H)
    try:
        vp.render_adaptive(buf.ptr, stats.ptr, 0, a["max_frames"], P, **A.anchor_args(a))
        vp.denoise(dst.ptr, buf.ptr, stats.ptr, W, H, 5, 1, 0.45)
        got = dst.download()
        assert A.same_state(st, buf.download(), stats.download()) is None
        assert got.tobytes() == D.denoise(st.acc, st.records(), 5, 1, 0.45).tobytes()
    finally:
        buf.free(); stats.free(); dst.free()
