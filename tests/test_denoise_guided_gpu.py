"""GPU suite: the feature-guided NL-means filter (include/volpath.h vp_denoise_guided).

The filter is DEFINED to the bit; tests/denoise_guided_lib.py restates the definition in numpy, and every comparison here is tobytes()
equality of all four channels against it: on uploaded synthetic buffers and synthetic feature planes (a ramp with a step edge, a
depth-like plane with a +inf region, a 0/1 cover plane), with every number of features, in both forms of the kernel, with a separate
guide pair, and behind a render and a feature pass queued on the same stream.  tests/test_denoise_guided_cpu.py checks, on the
restatement, that these inputs exercise the feature term (most filtered pixels change; pairs inf/inf and inf/finite occur)."""
import numpy as np
import pytest

import adaptive_lib as A
import denoise_guided_lib as G
import denoise_lib as D
import features_lib as FL
import scenes

pytestmark = pytest.mark.gpu

NAN_PATTERN = np.uint32(0x7FC12345)
K = 0.45
CLI_SIGMA_ALPHA, CLI_SIGMA_DEPTH = 0.2, 0.2
# feature lists by name: (plane, channel, sigma) with plane "a" (alpha-like) or "d" (depth-like)
RAMP, ZT, COVER, SLOPE = ("a", 1, 0.1), ("d", 1, 0.2), ("d", 3, 0.1), ("d", 0, 0.3)
NF_LISTS = {1: [RAMP], 2: [RAMP, ZT], 3: [RAMP, ZT, COVER], 4: [RAMP, ZT, COVER, SLOPE]}


@pytest.fixture(autouse=True)
def _restore(vp):
    yield
    vp.set_denoise_form(0)
    vp.set_arithmetic(vp.ARITH_EXACT)
    vp.set_subpixel(1)
    vp.set_shard(0, 1)
    vp.set_camera()


_memo = {}


def _inputs(W, H, seed):
    """(acc, rec, {"a": alpha, "d": depth}) of a size, made once"""
    key = ("in", W, H, seed)
    if key not in _memo:
        acc, rec = D.synthetic(W, H, seed)
        alpha, depth = G.synthetic_features(W, H, seed)
        _memo[key] = (acc, rec, {"a": alpha, "d": depth})
    return _memo[key]


def _want(W, H, seed, feats, R, F, gseed=None):
    """the restatement's answer, computed once and never changed"""
    key = ("out", W, H, seed, tuple(feats), R, F, gseed)
    if key not in _memo:
        acc, rec, planes = _inputs(W, H, seed)
        g = _inputs(W, H, gseed)[:2] if gseed is not None else (None, None)
        out = G.denoise_guided(acc, rec, [(planes[p], c, s) for p, c, s in feats], R, F, K, guide=g[0], guide_rec=g[1])
        out.setflags(write=False)
        _memo[key] = out
    return _memo[key]


class Scene:
    """a synthetic pair and its two feature planes on the device, and a NaN-filled dst"""

    def __init__(self, vp, W, H, seed):
        self.vp, self.W, self.H = vp, W, H
        self.acc, self.rec, self.planes = _inputs(W, H, seed)
        self.rec = np.ascontiguousarray(self.rec, vp.PIXEL_STATS_DTYPE)
        self.buf, self.stats, self.dst = vp.DeviceBuffer(W, H), vp.StatsBuffer(W, H), vp.DeviceBuffer(W, H)
        self.dev = {n: vp.DeviceBuffer(W, H) for n in self.planes}
        self.buf.upload(self.acc)
        self.stats.upload(self.rec)
        for n, p in self.planes.items():
            self.dev[n].upload(p)

    def run(self, feats, R, F, guide=None, plain=False):
        nan = np.full((self.H, self.W, 4), NAN_PATTERN, np.uint32).view(np.float32)
        self.dst.upload(nan)
        kw = dict(guide_ptr=guide.buf.ptr, guide_stats_ptr=guide.stats.ptr) if guide is not None else {}
        if plain:
            self.vp.denoise(self.dst.ptr, self.buf.ptr, self.stats.ptr, self.W, self.H, R, F, K, **kw)
        else:
            self.vp.denoise_guided(self.dst.ptr, self.buf.ptr, self.stats.ptr, self.W, self.H, [(self.dev[p].ptr, c, s) for p, c, s in feats], R, F, K, **kw)
        return self.dst.download()

    def untouched(self):
        return (self.buf.download().tobytes() == self.acc.tobytes() and self.stats.download().tobytes() == self.rec.tobytes()
                and all(self.dev[n].download().tobytes() == self.planes[n].tobytes() for n in self.planes))

    def free(self):
        for b in [self.buf, self.stats, self.dst] + list(self.dev.values()):
            b.free()


# ---- 1. sizes: one pixel; one pixel more than a tile each way (four workgroups, clamped halos on every side); no multiple of the tile
@pytest.mark.parametrize("W,H", [(1, 1), (33, 9), (70, 37)])
def test_sizes_equal_the_restatement(vp, W, H):
    s = Scene(vp, W, H, 100 + W)
    try:
        for feats, R, F in ((NF_LISTS[3], 5, 1), (NF_LISTS[2], 2, 2)):
            got = s.run(feats, R, F)
            assert vp.last_denoise_form() == 0
            assert not np.isnan(got).any()                        # a NaN-filled dst is fully overwritten
            assert got.tobytes() == _want(W, H, 100 + W, feats, R, F).tobytes(), (W, H, len(feats), R, F)
        assert s.untouched()
    finally:
        s.free()


# ---- 2. parameters: every instance family, the LDS limit, features that share a plane or a channel
PARAM_CASES = [(NF_LISTS[1], 5, 1), (NF_LISTS[2], 5, 1), (NF_LISTS[3], 5, 1), (NF_LISTS[4], 5, 1),
               (NF_LISTS[2], 0, 0),
               (NF_LISTS[4], 10, 3),                              # 64064 bytes of LDS: the limit
               ([ZT, COVER], 5, 1),                               # two features from one plane
               ([RAMP, ("a", 1, 0.25)], 3, 0),                    # the same channel named twice
               (NF_LISTS[3], 4, 2), (NF_LISTS[1], 3, 3)]


@pytest.mark.parametrize("case", range(len(PARAM_CASES)), ids=["R%d-F%d-%s" % (R, F, "+".join("%s%d" % (p, c) for p, c, _ in f)) for f, R, F in PARAM_CASES])
def test_parameters_equal_the_restatement_in_both_forms(vp, case):
    W, H = 70, 37
    feats, R, F = PARAM_CASES[case]
    want = _want(W, H, 100 + W, feats, R, F)
    s = Scene(vp, W, H, 100 + W)
    try:
        out = {}
        for form in (1, 0):
            vp.set_denoise_form(form)
            out[form] = s.run(feats, R, F)
            assert vp.last_denoise_form() == form
            assert not np.isnan(out[form]).any()
        assert out[0].tobytes() == want.tobytes(), "tiled form"
        assert out[1].tobytes() == want.tobytes(), "plain form"
        if R > 0:
            assert out[0].tobytes() != s.run([], R, F, plain=True).tobytes()       # the features matter
        assert s.untouched()
    finally:
        s.free()


# ---- 4. cross-checks
def test_no_feature_equals_vp_denoise_and_a_guide_pair_works(vp):
    W, H = 70, 37
    s, g = Scene(vp, W, H, 100 + W), Scene(vp, W, H, 8)
    try:
        for form in (0, 1):
            vp.set_denoise_form(form)
            plain = s.run([], 5, 1, plain=True)
            assert s.run([], 5, 1).tobytes() == plain.tobytes() == D.denoise(s.acc, s.rec, 5, 1, K).tobytes()
            assert vp.last_denoise_form() == form
            assert s.run([], 3, 2, guide=g).tobytes() == s.run([], 3, 2, guide=g, plain=True).tobytes()
            # a separate guide pair: weights' patch distances from g, colours from s, features from s's planes
            got = s.run(NF_LISTS[3], 5, 1, guide=g)
            assert got.tobytes() == _want(W, H, 100 + W, NF_LISTS[3], 5, 1, gseed=8).tobytes(), form
            assert got.tobytes() != _want(W, H, 100 + W, NF_LISTS[3], 5, 1).tobytes()
        # feature planes may be src or the guide: any float4 image serves (finite channels here)
        vp.set_denoise_form(0)
        nan = np.full((H, W, 4), NAN_PATTERN, np.uint32).view(np.float32)
        s.dst.upload(nan)
        vp.denoise_guided(s.dst.ptr, s.buf.ptr, s.stats.ptr, W, H, [(s.buf.ptr, 3, 40.0), (g.buf.ptr, 0, 1e3)], 2, 1, K, guide_ptr=g.buf.ptr,
                          guide_stats_ptr=g.stats.ptr)
        want = G.denoise_guided(s.acc, s.rec, [(s.acc, 3, 40.0), (g.acc, 0, 1e3)], 2, 1, K, guide=g.acc, guide_rec=g.rec)
        assert s.dst.download().tobytes() == want.tobytes()
        assert s.untouched() and g.untouched()
    finally:
        s.free(); g.free()


# ---- 5. end to end on one stream, and 6. under the fast arithmetic
def _scene(vp):
    vp.set_subpixel(1)
    vp.init_volume(vp.julia_volume(32), brick=1, linear=True)
    vp.init_envmap(scenes.synthetic_env())
    vp.set_sun(scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER)
    vp.set_camera()
    vp.set_estimator(vp.EST_GLOBAL)
    vp.set_tracking(0)
    vp.set_envmap_sampling(vp.ENV_PASSIVE)
    vp.set_shard(0, 1)
    vp.set_rng(vp.RNG_PHILOX7, (1, 2))


def test_render_features_and_guided_denoise_without_a_synchronise(vp, oracle):
    W, H, step = A.ANCHOR_W, A.ANCHOR_H, 0.01
    osc, oP = A.anchor_oracle(oracle, scenes, dict(est="global", rng="philox7", key=(1, 2)))
    st = A.render_uniform(A.Stats(W, H), A.oracle_frames(osc, oP), 0, 16)
    rec = st.records()
    alpha, depth, _ = FL.features(oracle, osc, W, H, step, oP.density, tuple(oP.sigma_t))
    feats = lambda a, d: [(a, 1, CLI_SIGMA_ALPHA), (d, 1, CLI_SIGMA_DEPTH), (d, 3, CLI_SIGMA_ALPHA)]      # the CLI's three
    want = G.denoise_guided(st.acc, rec, feats(alpha, depth), 5, 1, K)
    want_plain = D.denoise(st.acc, rec, 5, 1, K)
    assert want.tobytes() != want_plain.tobytes()
    _scene(vp)
    P = vp.make_param(W, H)
    buf, stats, dst, dst2, da, dd = (vp.DeviceBuffer(W, H), vp.StatsBuffer(W, H), vp.DeviceBuffer(W, H), vp.DeviceBuffer(W, H), vp.DeviceBuffer(W, H),
                                     vp.DeviceBuffer(W, H))
    try:
        # what the two older calls give before the new one has run
        vp.render_frames(dst2.ptr, 0, 2, P)
        frames_before = dst2.download()
        # queued back to back: nothing waits in between
        vp.render_frames_stats(buf.ptr, stats.ptr, 0, 16, P)
        vp.render_features(P, step, alpha_ptr=da.ptr, depth_ptr=dd.ptr)
        vp.denoise_guided(dst.ptr, buf.ptr, stats.ptr, W, H, feats(da.ptr, dd.ptr), 5, 1, K)
        got = dst.download()
        assert da.download().tobytes() == alpha.tobytes() and dd.download().tobytes() == depth.tobytes()
        assert buf.download().tobytes() == st.acc.tobytes()
        assert got.tobytes() == want.tobytes()
        # under VP_ARITH_FAST the call gives the same bytes
        vp.set_arithmetic(vp.ARITH_FAST)
        dst.reset()
        vp.denoise_guided(dst.ptr, buf.ptr, stats.ptr, W, H, feats(da.ptr, dd.ptr), 5, 1, K)
        assert dst.download().tobytes() == want.tobytes()
        vp.set_arithmetic(vp.ARITH_EXACT)
        # vp_denoise and vp_render_frames afterwards: the bits they gave before
        vp.denoise(dst.ptr, buf.ptr, stats.ptr, W, H, 5, 1, K)
        assert dst.download().tobytes() == want_plain.tobytes()
        dst2.reset()
        vp.render_frames(dst2.ptr, 0, 2, P)
        assert dst2.download().tobytes() == frames_before.tobytes()
    finally:
        for b in (buf, stats, dst, dst2, da, dd):
            b.free()
