"""GPU suite: per-pixel statistics and adaptive sampling (include/volpath.h vp_pixel_stats, vp_render_frames_stats,
vp_render_adaptive, vp_scale_by_count, vp_stats_rel_error).

A sample is a pure function of (pixel, frame, keys, scene), so an adaptive render is DEFINED: tests/adaptive_lib.py restates the
definition in numpy and every comparison here is bit equality against it -- accumulator, n, flags, both float64 sums by their bit
patterns, and the result fields -- fed with the CPU oracle's frames, or with the library's own one-frame renders where the oracle has
no say (the fast arithmetic) or is too slow."""
import ctypes as C
import os

import numpy as np
import pytest

import adaptive_lib as A
import scenes
import subpixel_lib as sub

pytestmark = pytest.mark.gpu

W, H = A.ANCHOR_W, A.ANCHOR_H
EST = {"global": 0, "decomp": 1, "bounded": 2}
RNG = {"samplerh": 0, "philox": 1, "philox7": 2}


@pytest.fixture(autouse=True)
def _restore(vp):
    yield
    vp.set_subpixel(1)
    vp.set_arithmetic(vp.ARITH_EXACT)
    vp.set_lookahead(vp.LOOKAHEAD_DEFAULT)
    vp.set_pipeline(True)
    vp.set_shard(0, 1)
    vp.enable_counters(False)
    vp.set_camera()


def _scene(vp, est, rng_mode, key, n=32, brick=1):
    vp.set_subpixel(1)
    vp.init_volume(vp.julia_volume(n), brick=brick, linear=True)
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


class Target:
    """an accumulator and a statistics buffer of one image"""

    def __init__(self, vp, P):
        self.vp, self.P = vp, P
        self.buf = vp.DeviceBuffer(P.width, P.height)
        self.stats = vp.StatsBuffer(P.width, P.height)

    def adaptive(self, first, max_frames, **args):
        return self.vp.render_adaptive(self.buf.ptr, self.stats.ptr, first, max_frames, self.P, **args)

    def uniform(self, first, n):
        self.vp.render_frames_stats(self.buf.ptr, self.stats.ptr, first, n, self.P)

    def state(self):
        return self.buf.download(), self.stats.download()

    def free(self):
        self.buf.free(); self.stats.free()


def _adaptive(vp, P, calls, **args):
    """the calls (first, max_frames) on fresh buffers: (accumulator, records, [result, ...])"""
    t = Target(vp, P)
    try:
        res = [t.adaptive(first, n, **args) for first, n in calls]
        return t.state() + (res,)
    finally:
        t.free()


def _check(st, acc, rec, what=""):
    diff = A.same_state(st, acc, rec)
    assert diff is None, (what, diff)


# ---- 1. the uniform render with statistics
@pytest.mark.parametrize("est_name,rng_name", [("global", "philox"), ("decomp", "samplerh"), ("bounded", "philox7")])
def test_uniform_stats_leave_render_frames_bits_and_the_oracle_records(vp, oracle, est_name, rng_name):
    est, rng_mode, key = EST[est_name], RNG[rng_name], (1, 2)
    osc = oracle.OracleScene(oracle.julia(32), scenes.synthetic_env(), scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER, estimator=est, rng_mode=rng_mode, seed=key)
    if est == 1:
        osc.precompute_opacity()
    frame = A.oracle_frames(osc, oracle.default_param(W, H))
    calls = [(2, 7), (9, 1), (10, 12)]        # a one-frame call goes through staging too; frames 2 .. 21 cross the frame-11 switch
    want = A.Stats(W, H)
    for first, n in calls:
        A.render_uniform(want, frame, first, n)
    _scene(vp, est, rng_mode, key)
    P = vp.make_param(W, H)
    plain = vp.DeviceBuffer(W, H)
    t = Target(vp, P)
    try:
        for first, n in calls:
            vp.render_frames(plain.ptr, first, n, P)
            t.uniform(first, n)
            assert vp.last_pipelined() == 0
        acc, rec = t.state()
        assert acc.tobytes() == plain.download().tobytes()
        _check(want, acc, rec, (est_name, rng_name))
        assert (rec["n"] == 20).all() and not rec["flags"].any() and (rec["sum_y"] > 0).any()
        # flags are neither read nor set: a buffer whose records are all frozen is sampled like any other, and stays frozen
        t.buf.reset()
        frozen = np.zeros((H, W), vp.PIXEL_STATS_DTYPE)
        frozen["flags"] = vp.STATS_FROZEN
        frozen["flags"][::2] |= 0x80        # (the other bits are the caller's too)
        t.stats.upload(frozen)
        t.uniform(2, 7)
        acc, rec = t.state()
        want7 = A.render_uniform(A.Stats(W, H), frame, 2, 7)
        want7.flags[:] = frozen["flags"]
        _check(want7, acc, rec, "frozen records")
    finally:
        plain.free(); t.free()


def test_uniform_stats_touch_only_the_shard(vp):
    _scene(vp, vp.EST_GLOBAL, vp.RNG_PHILOX, (1, 2))
    P = vp.make_param(W, H)
    frame, fbuf = A.library_frames(vp, P)
    t = Target(vp, P)
    try:
        vp.set_shard(0, 1)
        want = A.Stats(W, H)
        for r in (2, 0):
            A.render_uniform(want, frame, 0, 5, owned=A.owned_pixels(vp, W, H, r, 3))
        for r in (2, 0):
            vp.set_shard(r, 3)
            t.uniform(0, 5)
        vp.set_shard(0, 1)
        acc, rec = t.state()
        _check(want, acc, rec)
        mine = A.owned_pixels(vp, W, H, 1, 3)
        assert not rec["n"][mine].any() and (rec["n"][~mine] == 5).all()
    finally:
        vp.set_shard(0, 1)
        fbuf.free(); t.free()


# ---- 2. adaptive against the oracle
@pytest.mark.parametrize("anchor,floor_between,floor_active", [(A.ANCHOR1, 150, 40), (A.ANCHOR2, 100, 8)], ids=["global-philox10", "decomp-philox7"])
def test_anchor_equals_the_oracle_restatement(vp, oracle, anchor, floor_between, floor_active):
    osc, oP = A.anchor_oracle(oracle, scenes, anchor)
    want = A.Stats(W, H)
    wres = A.render_adaptive(want, A.oracle_frames(osc, oP), 0, anchor["max_frames"], **A.anchor_args(anchor))
    c = A.census(want, anchor["min_frames"], anchor["max_frames"])
    print("the oracle's expectation:", wres, c)
    # what keeps the comparison from passing trivially, on the ORACLE's expectation
    assert c["at_min"] >= 2000 and c["between"] >= floor_between and c["active"] >= floor_active
    _scene(vp, EST[anchor["est"]], RNG[anchor["rng"]], anchor["key"])
    acc, rec, res = _adaptive(vp, vp.make_param(W, H), [(0, anchor["max_frames"])], **A.anchor_args(anchor))
    print("the library:", res[0])
    _check(want, acc, rec)
    assert res[0] == wres


@pytest.mark.parametrize("rng_name", ["samplerh", "philox", "philox7"])
@pytest.mark.parametrize("est_name", ["global", "decomp", "bounded"])
def test_estimators_and_streams_equal_the_oracle_restatement(vp, oracle, est_name, rng_name):
    """frames 5 .. 24: across the frame-11 switch of the decomposition estimator"""
    est, rng_mode, key = EST[est_name], RNG[rng_name], (3, 4)
    args = dict(rel_tol=0.2, floor_y=1e-3, min_frames=8, round_frames=4)
    osc = oracle.OracleScene(oracle.julia(32), scenes.synthetic_env(), scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER, estimator=est, rng_mode=rng_mode, seed=key)
    if est == 1:
        osc.precompute_opacity()
    want = A.Stats(W, H)
    wres = A.render_adaptive(want, A.oracle_frames(osc, oracle.default_param(W, H)), 5, 20, **args)
    c = A.census(want, 8, 20)
    assert c["at_min"] >= 2000 and c["between"] >= 50 and c["active"] >= 20, c
    _scene(vp, est, rng_mode, key)
    acc, rec, res = _adaptive(vp, vp.make_param(W, H), [(5, 20)], **args)
    _check(want, acc, rec, (est_name, rng_name))
    assert res[0] == wres


# ---- 3. invariance: each against the same call done plainly
def _anchor_plain(vp, P, first=0, max_frames=48, **over):
    args = dict(A.anchor_args(A.ANCHOR1), **over)
    return _adaptive(vp, P, [(first, max_frames)], **args), args


@pytest.mark.parametrize("world", [2, 3])
def test_shards_sum_to_the_whole_image(vp, world):
    _scene(vp, vp.EST_DECOMP, vp.RNG_PHILOX7, (1, 2))
    P = vp.make_param(W, H)
    (acc, rec, res), args = _anchor_plain(vp, P)
    total = vp.DeviceBuffer(W, H)
    recs, results = [], []
    try:
        for r in range(world):
            vp.set_shard(r, world)
            t = Target(vp, P)     # separate buffers per shard
            try:
                results.append(t.adaptive(0, 48, **args))
                vp.accumulate(total.ptr, t.buf.ptr, W * H)
                recs.append(t.stats.download())
                mine = A.owned_pixels(vp, W, H, r, world)
                assert not recs[-1]["n"][~mine].any() and not recs[-1]["flags"][~mine].any() and (recs[-1]["n"][mine] >= 16).all()
            finally:
                t.free()
        vp.set_shard(0, 1)
        assert total.download().tobytes() == acc.tobytes()
        for k in ("sum_y", "sum_y2", "n", "flags"):
            assert A.equal_bits(sum(r[k].astype(np.float64) for r in recs), rec[k].astype(np.float64)), k   # (every pixel has one owner: the rest is zero)
        assert sum(r["samples"] for r in results) == res[0]["samples"]
        assert sum(r["active_left"] for r in results) == res[0]["active_left"]
        assert max(r["frames_used"] for r in results) == res[0]["frames_used"]
    finally:
        vp.set_shard(0, 1)
        total.free()


def test_a_staging_cap_that_splits_every_round_into_launches(vp):
    """VP_STAGE_MB=1 in a context of its own (the knob is read when a context first touches its device): 160x120 pixels are 300 KiB of
    staging per frame, so a round of eight frames needs three launches while all pixels are active -- and the criterion must be
    evaluated after the round, not after each launch"""
    P = vp.make_param(160, 120)
    args = dict(rel_tol=0.1, floor_y=1e-3, min_frames=2, round_frames=8)   # (min_frames below a launch's three frames)
    _scene(vp, vp.EST_GLOBAL, vp.RNG_PHILOX, (1, 2))
    vp.render_time_ms(reset=True)
    acc, rec, res = _adaptive(vp, P, [(0, 32)], **args)
    launches_plain = vp.render_time_ms(reset=True)[1]
    assert res[0]["rounds"] == launches_plain == 4
    old = os.environ.get("VP_STAGE_MB")
    os.environ["VP_STAGE_MB"] = "1"
    try:
        ctx = vp.Context(0)
    finally:
        if old is None:
            del os.environ["VP_STAGE_MB"]
        else:
            os.environ["VP_STAGE_MB"] = old
    try:
        with ctx:
            _scene(vp, vp.EST_GLOBAL, vp.RNG_PHILOX, (1, 2))
            vp.render_time_ms(reset=True)
            acc2, rec2, res2 = _adaptive(vp, P, [(0, 32)], **args)
            launches = vp.render_time_ms(reset=True)[1]
    finally:
        ctx.destroy()
    assert launches >= launches_plain + 2, (launches, launches_plain)   # (the first round alone: three launches)
    assert acc2.tobytes() == acc.tobytes() and rec2.tobytes() == rec.tobytes() and res2 == res
    frozen = (rec["flags"] & 1) != 0
    assert frozen.any() and (~frozen).any() and (rec["n"][frozen] % 8 == 0).all()


def test_pipeline_round_of_one_and_resumed_calls(vp, oracle):
    osc, oP = A.anchor_oracle(oracle, scenes, A.ANCHOR1)
    frame = A.oracle_frames(osc, oP)
    _scene(vp, vp.EST_GLOBAL, vp.RNG_PHILOX, (1, 2))
    P = vp.make_param(W, H)
    (acc, rec, res), args = _anchor_plain(vp, P)
    want = A.Stats(W, H)
    assert A.render_adaptive(want, frame, 0, 48, **args) == res[0]
    _check(want, acc, rec)
    # the pipeline on and off around the call, with pipelined plain calls in flight before and after it
    other = vp.DeviceBuffer(W, H)
    try:
        for on in (True, False):
            vp.set_pipeline(on)
            other.reset()
            vp.render_frames(other.ptr, 0, 8, P)
            vp.render_frames(other.ptr, 8, 8, P)
            assert vp.last_pipelined() == int(on)
            a2, r2, res2 = _adaptive(vp, P, [(0, 48)], **args)
            assert vp.last_pipelined() == 0
            vp.render_frames(other.ptr, 16, 8, P)
            assert vp.last_pipelined() == int(on)
            assert a2.tobytes() == acc.tobytes() and r2.tobytes() == rec.tobytes() and res2 == res, on
            plain = A.render_uniform(A.Stats(W, H), frame, 0, 24)
            assert other.download().tobytes() == plain.acc.tobytes()
    finally:
        vp.set_pipeline(True)
        other.free()
    # rounds of one frame: every frame through staging, a decision after each
    args1 = dict(args, round_frames=1, min_frames=5)
    want1 = A.Stats(W, H)
    wres1 = A.render_adaptive(want1, frame, 3, 20, **args1)
    a1, r1, res1 = _adaptive(vp, P, [(3, 20)], **args1)
    _check(want1, a1, r1, "round of one")
    assert res1[0] == wres1 and wres1["rounds"] == 20 and len(np.unique(r1["n"])) > 8
    # a last round of one frame
    want2 = A.Stats(W, H)
    wres2 = A.render_adaptive(want2, frame, 0, 17, **args)
    a2, r2, res2 = _adaptive(vp, P, [(0, 17)], **args)
    _check(want2, a2, r2, "last round of one frame")
    assert res2[0] == wres2 and wres2["rounds"] == 3
    # a resumed call: the frozen set is what the buffer says -- equal to one call when the round divides the first call's frames
    a3, r3, res3 = _adaptive(vp, P, [(0, 24), (24, 24)], **args)
    assert a3.tobytes() == acc.tobytes() and r3.tobytes() == rec.tobytes()
    assert res3[0]["samples"] + res3[1]["samples"] == res[0]["samples"] and res3[1]["active_left"] == res[0]["active_left"]
    assert res3[0]["rounds"] + res3[1]["rounds"] == res[0]["rounds"]
    # ... and equal to the restatement of the two calls when it does not
    want4 = A.Stats(W, H)
    wres4 = [A.render_adaptive(want4, frame, 0, 20, **args), A.render_adaptive(want4, frame, 20, 28, **args)]
    a4, r4, res4 = _adaptive(vp, P, [(0, 20), (20, 28)], **args)
    _check(want4, a4, r4, "resumed, odd split")
    assert res4 == wres4 and a4.tobytes() != acc.tobytes()


@pytest.mark.parametrize("est_name", ["global", "decomp"])
def test_fast_arithmetic_and_a_subpixel_factor_equal_the_library_restatement(vp, est_name):
    """the restatement fed with the library's own one-frame renders (fast arithmetic: no oracle; factor 2: the gather of
    tests/subpixel_lib.py from S = 1 renders of the fine image)"""
    est = EST[est_name]
    args = dict(rel_tol=0.15, floor_y=1e-3, min_frames=8, round_frames=4)
    first, max_frames = 4, 24
    _scene(vp, est, vp.RNG_PHILOX7, (5, 9), brick=4 if est == 1 else 1)
    P = vp.make_param(W, H)
    for arith in (vp.ARITH_FAST, vp.ARITH_EXACT):
        vp.set_arithmetic(arith)
        for s in (1, 2):
            vp.set_subpixel(1)
            fine, fbuf = A.library_frames(vp, sub.fine_of(P, s))
            try:
                frame = A.cached(lambda f: sub.gather(vp, fine(f), W, H, f, s))
                want = A.Stats(W, H)
                wres = A.render_adaptive(want, frame, first, max_frames, **args)
                c = A.census(want, 8, max_frames)
                assert c["at_min"] > 1000 and c["between"] > 20 and c["active"] > 5, c
                uni = A.render_uniform(A.Stats(W, H), frame, first, 9)
            finally:
                fbuf.free()
            vp.set_subpixel(s)
            acc, rec, res = _adaptive(vp, P, [(first, max_frames)], **args)
            _check(want, acc, rec, (est_name, arith, s))
            assert res[0] == wres
            assert vp.last_arithmetic() == arith
            t = Target(vp, P)
            try:
                t.uniform(first, 9)
                _check(uni, *t.state(), what=("uniform", est_name, arith, s))
            finally:
                t.free()


# ---- 4. the state machine
def test_plain_calls_lists_and_lookahead_are_the_same_before_and_after(vp):
    _scene(vp, vp.EST_DECOMP, vp.RNG_PHILOX7, (1, 2), n=64, brick=4)
    P = vp.make_param(160, 120)
    args = dict(rel_tol=0.1, floor_y=1e-3, min_frames=8, round_frames=8)

    def plain():
        buf = vp.DeviceBuffer(160, 120)
        try:
            vp.render_frames(buf.ptr, 0, 64, P)       # (64 frames: the walk reads the per-view segment table)
            table = vp.last_approach_table()
            a = buf.download()
            buf.reset()
            for f in range(40):
                vp.render_kernel(buf.ptr, f, P)       # the look-ahead serves most of these from staged batches
            return a, buf.download(), table, [l.copy() for l in vp.pixel_lists(P)]
        finally:
            buf.free()

    a0, k0, table0, lists0 = plain()
    l0 = vp.lookahead_stats()[0]
    # an adaptive call in the middle of a look-ahead run
    buf = vp.DeviceBuffer(160, 120)
    try:
        for f in range(5):
            vp.render_kernel(buf.ptr, f, P)
        acc, rec, res = _adaptive(vp, P, [(0, 40)], **args)
        assert vp.last_approach_table() == 0          # the segment table is indexed by the slots of the FULL list: off on a compacted one
        for f in range(5, 9):
            vp.render_kernel(buf.ptr, f, P)
        nine = buf.download()
    finally:
        buf.free()
    assert 0 < res[0]["active_left"] < 160 * 120 and res[0]["samples"] < 40 * 160 * 120
    a1, k1, table1, lists1 = plain()
    assert vp.lookahead_stats()[0] > l0
    assert a1.tobytes() == a0.tobytes() and k1.tobytes() == k0.tobytes() and table1 == table0
    assert all(np.array_equal(x, y) for x, y in zip(lists0, lists1))
    buf = vp.DeviceBuffer(160, 120)
    try:
        vp.render_frames(buf.ptr, 0, 9, P)
        assert buf.download().tobytes() == nine.tobytes()
    finally:
        buf.free()
    # the adaptive call itself is reproducible after all of that
    acc2, rec2, res2 = _adaptive(vp, P, [(0, 40)], **args)
    assert acc2.tobytes() == acc.tobytes() and rec2.tobytes() == rec.tobytes() and res2 == res


def test_setters_counters_and_frozen_buffers(vp, oracle):
    _scene(vp, vp.EST_GLOBAL, vp.RNG_PHILOX, (1, 2))
    P = vp.make_param(W, H)
    args = A.anchor_args(A.ANCHOR1)
    # a setter between two resumed calls takes effect: the second call's frames come from the other stream
    osc, oP = A.anchor_oracle(oracle, scenes, A.ANCHOR1)
    osc2 = oracle.OracleScene(oracle.julia(32), scenes.synthetic_env(), scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER, estimator=0, rng_mode=2, seed=(8, 9))
    want = A.Stats(W, H)
    wres = [A.render_adaptive(want, A.oracle_frames(osc, oP), 0, 24, **args), A.render_adaptive(want, A.oracle_frames(osc2, oP), 24, 24, **args)]
    t = Target(vp, P)
    try:
        res = [t.adaptive(0, 24, **args)]
        vp.set_rng(vp.RNG_PHILOX7, (8, 9))
        res.append(t.adaptive(24, 24, **args))
        _check(want, *t.state(), what="setter between resumed calls")
        assert res == wres
        # counters enabled: VP_E_STATE, nothing rendered, the context stays usable
        before = t.state()
        vp.enable_counters(True)
        a = vp.Adaptive(0.1, 1e-3, 16, 8)
        assert vp.lib().vp_render_adaptive(t.buf.ptr, t.stats.ptr, 48, 8, C.byref(P), C.byref(a), None) == -2
        assert "counters" in vp.lib().vp_last_error().decode()
        vp.enable_counters(False)
        after = t.state()
        assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
        res.append(t.adaptive(48, 8, **args))
        assert res[-1] == A.render_adaptive(want, A.oracle_frames(osc2, oP), 48, 8, **args)
        _check(want, *t.state(), what="after the refusal")
        # every pixel already frozen: nothing is rendered, zero samples are reported
        rec = t.stats.download()
        rec["flags"] |= vp.STATS_FROZEN
        t.stats.upload(rec)
        acc = t.buf.download()
        vp.render_time_ms(reset=True)
        assert t.adaptive(56, 40, **args) == {"samples": 0, "rounds": 0, "active_left": 0, "frames_used": 0}
        assert vp.render_time_ms(reset=True)[1] == 0
        assert t.buf.download().tobytes() == acc.tobytes() and t.stats.download().tobytes() == rec.tobytes()
    finally:
        vp.enable_counters(False)
        t.free()
    # the decomposition estimator beyond frame 10 without the optical-depth table: refused as vp_render_frames refuses it
    vp.init_volume(vp.julia_volume(32), brick=1, linear=True)
    vp.set_estimator(vp.EST_DECOMP)
    t = Target(vp, P)
    try:
        a = vp.Adaptive(0.1, 1e-3, 4, 4)
        assert vp.lib().vp_render_adaptive(t.buf.ptr, t.stats.ptr, 0, 12, C.byref(P), C.byref(a), None) == -4    # VP_E_NOOPACITY
        assert vp.lib().vp_render_frames(t.buf.ptr, 0, 12, C.byref(P)) == -4
        assert not t.buf.download().any() and not t.stats.download()["n"].any()
        assert t.adaptive(0, 11, rel_tol=0.1, min_frames=4, round_frames=4)["rounds"] == 3
    finally:
        t.free()


# ---- 5. the output stage
def test_scale_by_count_and_the_noise_map(vp, oracle):
    osc, oP = A.anchor_oracle(oracle, scenes, A.ANCHOR1)
    _scene(vp, vp.EST_GLOBAL, vp.RNG_PHILOX, (1, 2))
    P = vp.make_param(W, H)
    t = Target(vp, P)
    out = vp.DeviceBuffer(W, H)
    try:
        t.adaptive(0, 48, **A.anchor_args(A.ANCHOR1))
        rec = t.stats.download()
        rec["n"][:3] = 0                    # n = 0 included; and counts with no exact reciprocal
        rec["n"][3:5] = 1
        t.stats.upload(rec)
        acc = t.buf.download()
        assert len(np.unique(rec["n"])) >= 6
        for s in (1.0, 0.37):
            vp.scale_by_count(out.ptr, t.buf.ptr, t.stats.ptr, W * H, s)
            got = out.download()
            assert got.tobytes() == A.scale_by_count(acc, rec["n"], s).tobytes(), s
            assert not got[:3].any() and (got[5:, :, :3] > 0).any()
        vp.scale_by_count(t.buf.ptr, t.buf.ptr, t.stats.ptr, W * H, 1.0)        # in place
        assert t.buf.download().tobytes() == A.scale_by_count(acc, rec["n"], 1.0).tobytes()
        # the noise map: within 2 binary32 ulps of the float64 restatement (rounded once; the binary64 intermediates are far below that)
        got = vp.stats_rel_error(t.stats.ptr, W, H, 1e-3)
        want = A.rel_error(rec["sum_y"], rec["sum_y2"], rec["n"], 1e-3)
        assert not got[rec["n"] < 2].any() and (got > 0).sum() > 100
        w32 = want.astype(np.float32)
        ulp = np.abs(got.view(np.int32).astype(np.int64) - w32.view(np.int32).astype(np.int64))
        print("noise map: largest distance to the float64 restatement %d ulp, largest value %.3f" % (int(ulp.max()), float(got.max())))
        assert ulp.max() <= 2
    finally:
        t.free(); out.free()


# ---- 6. a pin without the oracle: the estimate means what it says
def test_estimated_standard_error_matches_the_spread_of_independent_renders(vp):
    """Sixteen uniform 64-frame renders of the anchor scene under keys that differ in key1 (the key of a frame is (frame ^ key0) + key1:
    key0 below the frame count would only permute the same samples).  Over the 382 pixels whose means differ at all, the root mean
    square estimated standard error over the root mean square spread of the sixteen means.  Measured on the CPU oracle for three
    disjoint groups of keys: 0.995, 0.998, 1.022; the bound is four times the largest deviation.  In the exact mode the GPU computes
    the oracle's bits, so group 0 gives the oracle's 0.995 here."""
    _scene(vp, vp.EST_GLOBAL, vp.RNG_PHILOX, (7, 0x10000))
    P = vp.make_param(W, H)
    t = Target(vp, P)
    records = []
    try:
        for k in range(16):
            vp.set_rng(vp.RNG_PHILOX, (7, 0x10000 * (k + 1)))
            t.buf.reset(); t.stats.reset()
            t.uniform(0, 64)
            records.append(t.stats.download())
    finally:
        t.free()
    ratio, pixels = A.estimate_ratio(records)
    print("estimated / observed standard error of the mean: %.4f over %d pixels with spread" % (ratio, pixels))
    assert 0.9 <= ratio <= 1.1
    assert pixels == 382 and round(ratio, 3) == 0.995
