"""Adaptive sampling on group layers on the GPU (include/volpath.h vp_render_adaptive_group_layers).

Every comparison is at tolerance 0: accumulators, sum_y and sum_y2 by their bits, n and flags by value, the result struct field by
field -- against the restatement of tests/adaptive_group_layers_lib.py fed by the CPU oracle's plane samples (the anchors) or by the
library's own one-frame vp_render_frames_group_layers calls, and against vp_render_frames_group_layers_stats where the adaptive call
degenerates into it.  Each test runs in a context of its own."""
import ctypes as C

import numpy as np
import pytest

import adaptive_group_layers_lib as AG
import adaptive_lib as AL
import group_layers_lib as GLL
import layers_lib as LL
import plane_stats_lib as PS
import scenes

pytestmark = pytest.mark.gpu

W, H = PS.W, PS.H
E_STATE, E_ARG, E_NOOPACITY = -2, -3, -4
F32 = np.float32
SOFT = AG.ANCHORS[0]                # scene, estimator, stream, first frame: the first anchor's, whose oracle frames 0..47 are shared
SOFT_TOL = AG.ANCHOR_TOL[SOFT]
FLOORS = AG.ANCHOR_ARGS["floor_y"]
IDS = ["%s-est%d-rng%d-from%d" % a for a in AG.ANCHORS]


@pytest.fixture
def ctx(vp):
    c = vp.Context(0)
    try:
        with c:
            yield c
    finally:
        c.destroy()


def _scene(vp, oracle, name, est, rng_mode, size=(W, H), density=None):
    vp.init_volume(LL.grid_of(name, oracle), brick=1, linear=True)
    vp.init_envmap(LL.ENV)
    vp.set_sun(scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER)
    vp.set_camera()
    vp.set_estimator(est)
    vp.set_rng(rng_mode, LL.KEY)
    vp.set_tracking(vp.TRACK_SPECTRAL)
    vp.set_envmap_sampling(vp.ENV_PASSIVE)
    vp.set_shard(0, 1)
    if est == 1:
        vp.precompute_opacity(scenes.DEFAULT_SUN_DIR)
    return vp.make_param(size[0], size[1], **dict(LL.param_kw(name), **({} if density is None else {"density": density})))


class Planes:
    """the three accumulators and the three record buffers of a group-layers call"""

    def __init__(self, vp, w=W, h=H):
        self.vp, self.w, self.h = vp, w, h
        self.acc = tuple(vp.DeviceBuffer(w, h) for _ in range(3))
        self.rec = tuple(vp.StatsBuffer(w, h) for _ in range(3))

    def ptrs(self):
        return tuple(b.ptr for b in self.acc + self.rec)

    def adaptive(self, first, max_frames, P, rel_tol, floor_y, min_frames, round_frames):
        """the adaptive call; returns (its result dict, (acc0, acc1, acc2, rec0, rec1, rec2) downloaded)"""
        res = self.vp.render_adaptive_group_layers(*self.ptrs(), first, max_frames, P, rel_tol, floor_y, min_frames, round_frames)
        return res, self.download()

    def stats(self, first, n, P):
        self.vp.render_frames_group_layers_stats(*self.ptrs(), first, n, P)
        return self.download()

    def plain(self, first, n, P):
        self.vp.render_frames_group_layers(*(b.ptr for b in self.acc), first, n, P)
        return tuple(b.download() for b in self.acc)

    def download(self):
        return tuple(b.download() for b in self.acc + self.rec)

    def upload(self, st3):
        """the state of a restatement into the six buffers"""
        for k in (0, 1, 2):
            self.acc[k].upload(st3[k].acc)
            self.rec[k].upload(st3[k].records())

    def reset(self):
        for b in self.acc + self.rec:
            b.reset()

    def free(self):
        for b in self.acc + self.rec:
            b.free()


def _check(want, res_want, res, got, what):
    bad = AG.same_triple(want, got)
    assert bad is None, (what, bad)
    assert res == res_want, (what, res, res_want)


def _library_triple(vp, P, w=W, h=H):
    """(frame_triple(f) through one-frame plain group-layers calls of the library, the Planes that serve it)"""
    q = Planes(vp, w, h)
    return PS.library_frames(lambda f: vp.render_frames_group_layers(*(b.ptr for b in q.acc), f, 1, P), q.acc), q


# ------------------------------------------------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("name,est,rng,first", AG.ANCHORS, ids=IDS)
def test_anchors_equal_the_oracle_restatement(vp, oracle, ctx, name, est, rng, first):
    want, res_want, tally = AG.anchor_expected(oracle, name, est, rng, first)
    assert min(tally["held%d" % k] for k in (0, 1, 2)) > 0 and 0 < res_want["active_left"] < W * H     # (tests/test_adaptive_group_layers_cpu.py: the census)
    P = _scene(vp, oracle, name, est, rng)
    p = Planes(vp)
    try:
        res, got = p.adaptive(first, AG.ANCHOR_FRAMES, P, AG.ANCHOR_TOL[(name, est, rng, first)], **AG.ANCHOR_ARGS)
        _check(want, res_want, res, got, (name, est, rng, first))
    finally:
        p.free()


# ------------------------------------------------------------------------------------------- degenerate forms, the library itself
def test_min_frames_above_max_frames_and_one_round_is_the_stats_call(vp, oracle, ctx):
    """nothing can freeze and the round is the whole call: the bytes of the _stats call, flags as they were (a pattern in bits 1..31)"""
    name, est, rng, first = SOFT
    P = _scene(vp, oracle, name, est, rng)
    board = np.zeros((H, W), vp.PIXEL_STATS_DTYPE)
    yy, xx = np.mgrid[0:H, 0:W]
    board["flags"] = (((xx + 2 * yy) % 5) * 0x10203040 & 0xfffffffe).astype(np.uint32)
    p, q = Planes(vp), Planes(vp)
    try:
        for b in p.rec + q.rec:
            b.upload(board)
        res, got = p.adaptive(first, 12, P, (0.5, 0.5, 0.5), FLOORS, 13, 12)
        ref = q.stats(first, 12, P)
        assert [a.tobytes() for a in got] == [a.tobytes() for a in ref]
        assert all(np.array_equal(got[3 + k]["flags"], board["flags"]) for k in (0, 1, 2)) and board["flags"].any()
        assert res == {"samples": 12 * W * H, "rounds": 1, "active_left": W * H, "frames_used": 12}
        assert (got[3]["n"] == 12).all() and all((got[3 + k]["sum_y"] > 0).any() for k in (0, 1, 2))
    finally:
        p.free()
        q.free()


@pytest.mark.parametrize("round_frames,max_frames", ((1, 14), (50, 48), (5, 48)))
def test_round_lengths(vp, oracle, ctx, round_frames, max_frames):
    """a round of one frame (a decision after every frame); a round longer than the call (one decision, at the end); a round that does
    not divide the call (a short last round)"""
    name, est, rng, first = SOFT
    frames = AG.anchor_frames(oracle, name, est, rng, first)
    want = AG.new_triple(W, H)
    res_want = AG.render_adaptive_group_layers(want, frames, first, max_frames, SOFT_TOL, FLOORS, 4, round_frames)
    P = _scene(vp, oracle, name, est, rng)
    p = Planes(vp)
    try:
        res, got = p.adaptive(first, max_frames, P, SOFT_TOL, FLOORS, 4, round_frames)
        _check(want, res_want, res, got, (round_frames, max_frames))
        assert (want[0].flags & 1).any() and res_want["rounds"] == -(-max_frames // round_frames)
    finally:
        p.free()


@pytest.mark.parametrize("plane", (0, 1, 2), ids=AG.PLANES)
def test_flags_on_entry(vp, oracle, ctx, plane):
    """a checkerboard of FROZEN in one record only: such a pixel receives nothing and none of its records changes -- the preset bit is
    not copied to the other two; a pattern in the flag bits 1..31 of all three records is kept, also where the call freezes"""
    name, est, rng, first = SOFT
    frames = AG.anchor_frames(oracle, name, est, rng, first)
    yy, xx = np.mgrid[0:H, 0:W]
    board = ((xx + yy) % 2).astype(np.uint32)
    want = AG.new_triple(W, H)
    for k in (0, 1, 2):
        want[k].flags[:] = ((xx * 7 + yy * 13 + k) * 0x01010102 & 0xfffffffe).astype(np.uint32)
        want[k].acc[:] = F32(0.5 + k)                                   # what a frozen pixel keeps is what the caller left
        want[k].sum_y[:], want[k].sum_y2[:], want[k].n[:] = 0.25 * (k + 1), 0.125, 1 + k
    want[plane].flags |= board
    before = AG.copy_triple(want)
    P = _scene(vp, oracle, name, est, rng)
    p = Planes(vp)
    try:
        p.upload(want)
        res_want = AG.render_adaptive_group_layers(want, frames, first, 24, SOFT_TOL, FLOORS, 8, 4)
        res, got = p.adaptive(first, 24, P, SOFT_TOL, FLOORS, 8, 4)
        _check(want, res_want, res, got, plane)
        held = board == 1
        for k in (0, 1, 2):
            assert got[k][held].tobytes() == before[k].acc[held].tobytes() and got[3 + k][held].tobytes() == before[k].records()[held].tobytes(), k
            assert np.array_equal(got[3 + k]["flags"] & 0xfffffffe, before[k].flags & 0xfffffffe)
            if k != plane:
                assert not (got[3 + k]["flags"][held] & 1).any(), k
        newly = ((want[(plane + 1) % 3].flags & 1) != 0) & ~held
        assert newly.any() and res_want["samples"] <= 24 * int((~held).sum())
    finally:
        p.free()


def test_a_second_call_continues_the_first(vp, oracle, ctx):
    """48 frames in one call equal 20 + 28 in two: the frozen set is what the three buffers say, nothing else is kept"""
    name, est, rng, first = SOFT
    want, res_want, _ = AG.anchor_expected(oracle, name, est, rng, first)
    P = _scene(vp, oracle, name, est, rng)
    p = Planes(vp)
    try:
        r1, _ = p.adaptive(first, 20, P, SOFT_TOL, **AG.ANCHOR_ARGS)
        r2, got = p.adaptive(first + 20, 28, P, SOFT_TOL, **AG.ANCHOR_ARGS)
        assert AG.same_triple(want, got) is None, AG.same_triple(want, got)
        assert r1["samples"] + r2["samples"] == res_want["samples"] and r1["rounds"] + r2["rounds"] == res_want["rounds"] == 12
        assert r2["active_left"] == res_want["active_left"] and (r1["frames_used"], r2["frames_used"]) == (20, 28)
        # everything that is left is active: a third call on buffers whose pixels are all frozen in ONE record (the third) renders nothing
        rec = got[5].copy()
        rec["flags"] |= 1
        p.rec[2].upload(rec)
        r3, after = p.adaptive(first + 48, 8, P, SOFT_TOL, **AG.ANCHOR_ARGS)
        assert r3 == {"samples": 0, "rounds": 0, "active_left": 0, "frames_used": 0}
        assert all(after[k].tobytes() == got[k].tobytes() for k in (0, 1, 2, 3, 4)) and after[5].tobytes() == rec.tobytes()
    finally:
        p.free()


@pytest.mark.parametrize("out", ((0,), (1,), (2,), (0, 1), (0, 2), (1, 2)), ids=lambda o: "without-" + "-".join(AG.PLANES[k] for k in o))
def test_large_floors_take_planes_out_of_the_decision(vp, oracle, ctx, out):
    """floor_y[k] = 1e30f for one plane, and for each pair: the call's frozen set is the other planes' own (tests/
    test_adaptive_group_layers_cpu.py pins the restatement to the two-plane one; two planes out leaves adaptive_lib.render_adaptive on the
    third plane alone)"""
    name, est, rng, first = SOFT
    frames = AG.anchor_frames(oracle, name, est, rng, first)
    floors = tuple(AG.BIG_FLOOR if k in out else FLOORS[k] for k in (0, 1, 2))
    want = AG.new_triple(W, H)
    res_want = AG.render_adaptive_group_layers(want, frames, first, AG.ANCHOR_FRAMES, AG.FLOOR_TOL, floors, 8, 4)
    assert 0 < int((want[0].flags & 1).sum()) < W * H
    if len(out) == 2:
        keep = 3 - sum(out)
        alone = AL.Stats(W, H)
        res_alone = AL.render_adaptive(alone, lambda f: frames(f)[keep], first, AG.ANCHOR_FRAMES, AG.FLOOR_TOL[keep], FLOORS[keep], 8, 4)
        assert np.array_equal(alone.flags, want[keep].flags) and res_alone == res_want
    P = _scene(vp, oracle, name, est, rng)
    p = Planes(vp)
    try:
        res, got = p.adaptive(first, AG.ANCHOR_FRAMES, P, AG.FLOOR_TOL, floors, 8, 4)
        _check(want, res_want, res, got, out)
    finally:
        p.free()


# ------------------------------------------------------------------------------------------------------------------- shards
def test_three_shards_touch_their_own_tiles_and_make_up_the_whole(vp, oracle, ctx):
    name, est, rng, first = SOFT
    want, res_want, _ = AG.anchor_expected(oracle, name, est, rng, first)
    P = _scene(vp, oracle, name, est, rng)
    sentinel = np.zeros((H, W), vp.PIXEL_STATS_DTYPE)
    sentinel["sum_y"], sentinel["sum_y2"], sentinel["n"], sentinel["flags"] = -7.25, 1e300, 0xabcd0123, 0xfffffff0      # (FROZEN clear: it would be sampled)
    p, shared = Planes(vp), Planes(vp)
    try:
        seen, samples, left = np.zeros((H, W), int), 0, 0
        for r in range(3):
            vp.set_shard(r, 3)
            owned = AL.owned_pixels(vp, W, H, r, 3)
            start = sentinel.copy()
            start[owned] = 0
            p.reset()
            for b in p.rec:
                b.upload(start)
            res, got = p.adaptive(first, AG.ANCHOR_FRAMES, P, SOFT_TOL, **AG.ANCHOR_ARGS)
            for k in (0, 1, 2):
                assert got[3 + k][~owned].tobytes() == sentinel[~owned].tobytes(), (r, AG.PLANES[k])            # unowned records: untouched
                assert not got[k][~owned].any()
                assert AL.equal_bits(got[k][owned], want[k].acc[owned]) and got[3 + k][owned].tobytes() == want[k].records()[owned].tobytes(), (r, k)
            assert res["samples"] == int(want[0].n[owned].sum()) and res["active_left"] == int(((want[0].flags[owned] & 1) == 0).sum())
            res, _ = shared.adaptive(first, AG.ANCHOR_FRAMES, P, SOFT_TOL, **AG.ANCHOR_ARGS)             # ... and all ranks into one set of buffers
            samples, left = samples + res["samples"], left + res["active_left"]
            seen += owned
        assert (seen == 1).all()
        assert AG.same_triple(want, shared.download()) is None
        assert (samples, left) == (res_want["samples"], res_want["active_left"])
    finally:
        vp.set_shard(0, 1)
        p.free()
        shared.free()


# -------------------------------------------------------------------------------------------------------------- the staging cap
STAGE_TOL, STAGE_ARGS, STAGE_SIZE, STAGE_FRAMES = (0.15, 0.15, 0.15), dict(floor_y=(1e-3, 1e-3, 1e-3), min_frames=17, round_frames=8), (160, 120), 24


def test_a_staging_cap_that_splits_every_round_into_launches(vp, oracle, monkeypatch):
    """VP_STAGE_MB=1 in a context of its own, 160 x 120, as tests/test_adaptive_planes_gpu.py does it: a frame of all pixels is 300 KiB
    of staging per plane and the call stages two planes, so the rounds of 8 frames are split into launches -- and give the bits of one
    launch each.  min_frames is 17, so that every pixel is active in all three rounds and the decisions fall at the end of the third:
    a reduce that judged a record after a part of that round (n = 17 .. 23) would freeze pixels whose criterion holds there and not at
    24.  The restatement is fed by one-frame group-layers calls of the library.  The launches of a round follow from its active
    pixels: ceil(frames / floor(1 MiB / (pixels x 16 x 2)))."""
    monkeypatch.setenv("VP_STAGE_MB", "1")
    c = vp.Context(0)
    monkeypatch.delenv("VP_STAGE_MB", raising=False)
    try:
        with c:
            P = _scene(vp, oracle, "soft", 1, 1, size=STAGE_SIZE)
            frames, q = _library_triple(vp, P, *STAGE_SIZE)
            p = Planes(vp, *STAGE_SIZE)
            try:
                want = AG.new_triple(*STAGE_SIZE)
                active = []

                def counting(f):
                    if (f - 3) % 8 == 0:
                        active.append(int(AG.active_mask(want, AL.all_pixels(*STAGE_SIZE)).sum()))
                    return frames(f)
                res_want = AG.render_adaptive_group_layers(want, counting, 3, STAGE_FRAMES, STAGE_TOL, **STAGE_ARGS)
                vp.synchronize()
                vp.render_time_ms(reset=True)
                res, got = p.adaptive(3, STAGE_FRAMES, P, STAGE_TOL, **STAGE_ARGS)
                launches = vp.render_time_ms(reset=True)[1]
                _check(want, res_want, res, got, "capped")
                per_round = [-(-8 // max(1, (1 << 20) // (a * 16 * 2))) for a in active]
                print("active per round", active, "launches per round", per_round, "measured", launches)
                assert len(active) == res_want["rounds"] == 3 and launches == sum(per_round)
                assert min(per_round) >= 2, (active, per_round)                                  # every round was split
                frozen = (want[0].flags & 1) != 0
                noisy = np.zeros(frozen.shape, bool)
                for st in want:
                    nd = st.n.astype(np.float64)
                    noisy |= nd * st.sum_y2 - st.sum_y * st.sum_y > 0
                print("frozen", int(frozen.sum()), "noisy", int(noisy.sum()), "noisy and frozen", int((noisy & frozen).sum()))
                assert (noisy & frozen).any() and (noisy & ~frozen).any()                        # decisions of both kinds on pixels with variance
            finally:
                p.free()
                q.free()
    finally:
        c.destroy()


# -------------------------------------------------------------------------------------------------------------------- variants
VARIANTS = [("julia", 0, 61.0, 1, 1, "kernel"), ("julia", 0, 64.0, 1, 1, "constants"), ("julia", 1, 61.0, 1, 1, "kernel"), ("soft", 2, None, 2, 1, None),
            ("soft16", 1, None, 1, 1, None), ("soft", 0, None, 1, 0, None)]


@pytest.mark.parametrize("name,est,density,sub,rng,light", VARIANTS, ids=["%s-est%d-d%s-S%d-rng%d" % v[:5] for v in VARIANTS])
def test_variants_equal_the_restatement_on_the_librarys_own_frames(vp, oracle, ctx, name, est, density, sub, rng, light):
    """the light class as a kernel (a majorant of 61) and as constants (64: tests/test_layers_gpu.py has the reasons), the bounded
    estimator under vp_set_subpixel(2), a binary16 volume, the sampler.h stream: the adaptive call against the restatement fed by
    one-frame plain group-layers calls in the same state.  Frames 6..29 cross the decomposition estimator's switch."""
    first, n = 6, 24
    tol = (0.3, 0.1, 0.3)
    P = _scene(vp, oracle, name, est, rng, density=density)
    vp.set_subpixel(sub)
    frames, q = _library_triple(vp, P)
    p = Planes(vp)
    try:
        if light:
            general, lightpx, miss = vp.pixel_lists(P)
            assert len(lightpx) > 0 and len(miss) > 0 and len(general) > 0
        want = AG.new_triple(W, H)
        res_want = AG.render_adaptive_group_layers(want, frames, first, n, tol, FLOORS, 4, 4)
        if light:               # (of the plain one-frame calls just made, on the whole lists: a later round's list may hold no light pixel)
            assert vp.last_light_const() == (light == "constants")
        res, got = p.adaptive(first, n, P, tol, FLOORS, 4, 4)
        _check(want, res_want, res, got, (name, est, density, sub, rng))
        frozen = (want[0].flags & 1) != 0
        assert frozen.any() and not frozen.all()
    finally:
        vp.set_subpixel(1)
        p.free()
        q.free()


# --------------------------------------------------------------------------------------------------------- nothing left behind
@pytest.mark.parametrize("name,est", (("julia", 1), ("soft", 0)))
def test_the_call_leaves_nothing_behind(vp, oracle, ctx, name, est):
    """vp_render_frames, the groups, layers and group-layers calls, vp_render_adaptive and vp_render_adaptive_groups render the bits
    they rendered before the call, and the cached pixel lists are the same"""
    P = _scene(vp, oracle, name, est, 1)
    p, t = Planes(vp), Planes(vp)
    a0, a1, a2 = t.acc
    r0, r1, _ = t.rec
    try:
        def others():
            out = []
            for call in (lambda: vp.render_frames(a0.ptr, 6, 12, P), lambda: vp.render_frames_groups(a0.ptr, a1.ptr, 6, 12, P),
                         lambda: vp.render_frames_layers(a0.ptr, a1.ptr, 6, 12, P), lambda: vp.render_frames_group_layers(a0.ptr, a1.ptr, a2.ptr, 6, 12, P),
                         lambda: vp.render_adaptive(a0.ptr, r0.ptr, 6, 12, P, 0.2, 1e-3, 4, 4),
                         lambda: vp.render_adaptive_groups(a0.ptr, a1.ptr, r0.ptr, r1.ptr, 6, 12, P, (0.3, 0.3), (1e-3, 1e-3), 4, 4)):
                t.reset()
                res = call()
                out += [x.tobytes() for x in t.download()] + [repr(sorted(res.items())) if res else ""]
            out += [x.tobytes() for x in vp.pixel_lists(P)]
            return out

        before = others()
        res, got = p.adaptive(6, 12, P, (0.3, 0.3, 0.3), FLOORS, 4, 4)
        assert others() == before
        assert 0 < res["active_left"] < W * H and np.frombuffer(before[0], F32).max() > 0
    finally:
        p.free()
        t.free()


# --------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_touch_no_buffer_and_leave_the_context_usable(vp, oracle, ctx):
    name, est, rng, first = SOFT
    want, res_want, _ = AG.anchor_expected(oracle, name, est, rng, first)
    P = _scene(vp, oracle, name, est, rng)
    p = Planes(vp)
    fname = "vp_render_adaptive_group_layers"
    f = getattr(vp.lib(), fname)
    try:
        mark = np.full((H, W, 4), 7.25, F32)
        rmark = np.zeros((H, W), vp.PIXEL_STATS_DTYPE)
        rmark["sum_y"], rmark["sum_y2"], rmark["n"], rmark["flags"] = 3.5, 12.25, 5, 0x10
        for b in p.acc:
            b.upload(mark)
        for b in p.rec:
            b.upload(rmark)

        def refused(code, word, ptrs=None, first=first, maxf=12, tol=(0.1, 0.1, 0.1), fl=FLOORS, min_frames=4, round_frames=4):
            a = vp.AdaptivePlanes3((C.c_float * 3)(*tol), (C.c_float * 3)(*fl), min_frames, round_frames)
            res = vp.AdaptiveResult(7, 7, 7, 7)
            rc = f(*(ptrs or p.ptrs()), first, maxf, C.byref(P), C.byref(a), C.byref(res))
            vp.synchronize()
            msg = vp.lib().vp_last_error().decode()
            assert rc == code and word in msg and (fname in msg or code == E_NOOPACITY), (rc, msg)
            assert res.as_dict() == {"samples": 0, "rounds": 0, "active_left": 0, "frames_used": 0}
            got = p.download()
            assert all(got[k].tobytes() == mark.tobytes() and got[3 + k].tobytes() == rmark.tobytes() for k in (0, 1, 2)), word

        a0, a1, a2, r0, r1, r2 = p.ptrs()
        refused(E_ARG, "null", ptrs=(a0, a1, None, r0, r1, r2))
        refused(E_ARG, "null", ptrs=(a0, a1, a2, r0, r1, None))
        refused(E_ARG, "different", ptrs=(a0, a1, a0, r0, r1, r2))
        refused(E_ARG, "different", ptrs=(a0, a1, a2, r0, r2, r2))
        refused(E_ARG, "out of range", maxf=0)
        refused(E_ARG, "min_frames", min_frames=1)
        refused(E_ARG, "round_frames", round_frames=0)
        refused(E_ARG, "rel_tol", tol=(0.1, 0.1, float("nan")))
        refused(E_ARG, "floor_y", fl=(0.0, 0.0, -1.0))
        vp.set_envmap_sampling(vp.ENV_MIS)
        refused(E_STATE, "passive")
        vp.set_envmap_sampling(vp.ENV_PASSIVE)
        vp.set_arithmetic(vp.ARITH_FAST)                # the plane instances are the exact unit's
        refused(E_STATE, "exact")
        vp.set_arithmetic(vp.ARITH_EXACT)
        vp.set_tracking(vp.TRACK_SCALAR)
        refused(E_STATE, "spectral")
        vp.set_tracking(vp.TRACK_SPECTRAL)
        vp.enable_counters(True)
        refused(E_STATE, "counters")
        vp.enable_counters(False)
        vp.set_estimator(vp.EST_DECOMP)                 # no optical-depth table: frames beyond 10 are refused as vp_render_frames refuses them
        refused(E_NOOPACITY, "precompute_opacity", first=0, maxf=12)
        vp.set_estimator(est)
        p.reset()
        res, got = p.adaptive(first, AG.ANCHOR_FRAMES, P, SOFT_TOL, **AG.ANCHOR_ARGS)      # the context stays usable
        _check(want, res_want, res, got, "after the refusals")
    finally:
        vp.set_envmap_sampling(vp.ENV_PASSIVE)
        vp.set_arithmetic(vp.ARITH_EXACT)
        vp.set_tracking(vp.TRACK_SPECTRAL)
        vp.enable_counters(False)
        p.free()


# ------------------------------------------------------------------------------------------------------------- the output stage
def test_scale_by_count_per_plane_then_the_output_stage(vp, oracle, ctx):
    """each plane by ITS records' counts (vp_scale_by_count), then vp_relight_composite of the three means with scale 1, against the
    numpy restatements"""
    name, est, rng, first = SOFT
    rgb = (0.7, 0.1, 9.0)
    gains = ((2.0, 0.5, 0.25), (0.1, 1.0, 3.0))
    P = _scene(vp, oracle, name, est, rng)
    p, mean, dst = Planes(vp), tuple(vp.DeviceBuffer(W, H) for _ in range(3)), vp.DeviceBuffer(W, H)
    try:
        res, got = p.adaptive(first, AG.ANCHOR_FRAMES, P, SOFT_TOL, **AG.ANCHOR_ARGS)
        assert len(set(got[3]["n"].ravel().tolist())) > 2                          # the counts differ from pixel to pixel
        want_mean = [AL.scale_by_count(got[k], got[3 + k]["n"], 1.0) for k in (0, 1, 2)]
        for k in (0, 1, 2):
            vp.scale_by_count(mean[k].ptr, p.acc[k].ptr, p.rec[k].ptr, W * H, 1.0)
            assert mean[k].download().tobytes() == want_mean[k].tobytes(), AG.PLANES[k]
        vp.relight_composite(dst.ptr, mean[0].ptr, mean[1].ptr, mean[2].ptr, W * H, 1.0, *gains, plate_rgb=rgb)
        want = GLL.relight_composite(*want_mean, 1.0, *gains, rgb=rgb)
        assert dst.download().tobytes() == want.tobytes() and want[..., :3].max() > 0
    finally:
        for b in mean + (dst,):
            b.free()
        p.free()
