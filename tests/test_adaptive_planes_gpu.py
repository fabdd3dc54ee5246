"""Adaptive sampling on planes on the GPU (include/volpath.h vp_render_adaptive_groups / vp_render_adaptive_layers).

Every comparison is at tolerance 0: accumulators, sum_y and sum_y2 by their bits, n and flags by value, the result struct field by
field -- against the restatement of tests/adaptive_planes_lib.py fed by the CPU oracle's plane samples (the anchors) or by the library's
own one-frame plane calls, and against the library's _stats calls where the adaptive call degenerates into one.  Each test runs in a
context of its own."""
import ctypes as C

import numpy as np
import pytest

import adaptive_lib as AL
import adaptive_planes_lib as AP
import groups_lib as GL
import layers_lib as LL
import plane_stats_lib as PS
import scenes

pytestmark = pytest.mark.gpu

W, H = PS.W, PS.H
E_STATE, E_ARG, E_NOOPACITY = -2, -3, -4
F32 = np.float32
KINDS = ("groups", "layers")
NAMES = {"groups": ("sun", "sky"), "layers": ("fg", "trans")}
SOFT = ("soft", 0, 1, 0)            # scene, estimator, stream, first frame: the first anchor's, whose oracle frames 0..47 are shared


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
    """the two accumulators and the two record buffers of a plane call of `kind`"""

    def __init__(self, vp, kind, w=W, h=H):
        self.vp, self.kind, self.w, self.h = vp, kind, w, h
        self.acc = (vp.DeviceBuffer(w, h), vp.DeviceBuffer(w, h))
        self.rec = (vp.StatsBuffer(w, h), vp.StatsBuffer(w, h))
        self._adaptive = {"groups": vp.render_adaptive_groups, "layers": vp.render_adaptive_layers}[kind]
        self._stats = {"groups": vp.render_frames_groups_stats, "layers": vp.render_frames_layers_stats}[kind]
        self._plain = {"groups": vp.render_frames_groups, "layers": vp.render_frames_layers}[kind]

    def ptrs(self):
        return self.acc[0].ptr, self.acc[1].ptr, self.rec[0].ptr, self.rec[1].ptr

    def adaptive(self, first, max_frames, P, rel_tol, floor_y, min_frames, round_frames):
        """the adaptive call; returns (its result dict, (acc0, acc1, rec0, rec1) downloaded)"""
        res = self._adaptive(*self.ptrs(), first, max_frames, P, rel_tol, floor_y, min_frames, round_frames)
        return res, self.download()

    def stats(self, first, n, P):
        self._stats(*self.ptrs(), first, n, P)
        return self.download()

    def plain(self, first, n, P):
        self._plain(self.acc[0].ptr, self.acc[1].ptr, first, n, P)
        return self.acc[0].download(), self.acc[1].download()

    def download(self):
        return self.acc[0].download(), self.acc[1].download(), self.rec[0].download(), self.rec[1].download()

    def upload(self, st_pair):
        """the state of a restatement into the four buffers"""
        for k in (0, 1):
            self.acc[k].upload(st_pair[k].acc)
            self.rec[k].upload(st_pair[k].records())

    def reset(self):
        for b in self.acc + self.rec:
            b.reset()

    def free(self):
        for b in self.acc + self.rec:
            b.free()


def _check(kind, want, res_want, res, got, what):
    bad = AP.same_pair(want, got)
    assert bad is None, (what, kind, bad)
    assert res == res_want, (what, kind, res, res_want)


def _library_pair(vp, kind, P, w=W, h=H):
    """(frame_pair(f) through one-frame plain plane calls of the library, the Planes that serve it)"""
    q = Planes(vp, kind, w, h)
    return PS.library_frames(lambda f: q._plain(q.acc[0].ptr, q.acc[1].ptr, f, 1, P), q.acc), q


# ------------------------------------------------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("kind,name,est,rng,first", AP.ANCHORS, ids=["%s-%s-est%d-rng%d-from%d" % a for a in AP.ANCHORS])
def test_anchors_equal_the_oracle_restatement(vp, oracle, ctx, kind, name, est, rng, first):
    want, res_want, tally = AP.anchor_expected(oracle, kind, name, est, rng, first)
    assert tally["only0"] > 0 and tally["only1"] > 0 and 0 < res_want["active_left"] < W * H          # (tests/test_adaptive_planes_cpu.py: the census)
    P = _scene(vp, oracle, name, est, rng)
    p = Planes(vp, kind)
    try:
        res, got = p.adaptive(first, AP.ANCHOR_FRAMES, P, AP.ANCHOR_TOL[kind], **AP.ANCHOR_ARGS)
        _check(kind, want, res_want, res, got, (name, est, rng, first))
    finally:
        p.free()


# ------------------------------------------------------------------------------------------- degenerate forms, the library itself
@pytest.mark.parametrize("kind", KINDS)
def test_min_frames_above_max_frames_and_one_round_is_the_stats_call(vp, oracle, ctx, kind):
    """nothing can freeze and the round is the whole call: the bytes of the _stats call, flags as they were (a pattern in bits 1..31)"""
    name, est, rng, first = SOFT
    P = _scene(vp, oracle, name, est, rng)
    board = np.zeros((H, W), vp.PIXEL_STATS_DTYPE)
    yy, xx = np.mgrid[0:H, 0:W]
    board["flags"] = (((xx + 2 * yy) % 5) * 0x10203040 & 0xfffffffe).astype(np.uint32)
    p, q = Planes(vp, kind), Planes(vp, kind)
    try:
        for b in p.rec + q.rec:
            b.upload(board)
        res, got = p.adaptive(first, 12, P, (0.5, 0.5), (1e-3, 1e-3), 13, 12)
        ref = q.stats(first, 12, P)
        assert [a.tobytes() for a in got] == [a.tobytes() for a in ref]
        assert np.array_equal(got[2]["flags"], board["flags"]) and np.array_equal(got[3]["flags"], board["flags"]) and board["flags"].any()
        assert res == {"samples": 12 * W * H, "rounds": 1, "active_left": W * H, "frames_used": 12}
        assert (got[2]["n"] == 12).all() and (got[2]["sum_y"] > 0).any() and (got[3]["sum_y"] > 0).any()
    finally:
        p.free()
        q.free()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("round_frames,max_frames", ((1, 14), (50, 48), (5, 48)))
def test_round_lengths(vp, oracle, ctx, kind, round_frames, max_frames):
    """a round of one frame (a decision after every frame); a round longer than the call (one decision, at the end); a round that does
    not divide the call (a short last round)"""
    name, est, rng, first = SOFT
    frames = AP.anchor_frames(oracle, kind, name, est, rng, first)
    want = AP.new_pair(W, H)
    res_want = AP.render_adaptive_planes(want, frames, first, max_frames, AP.ANCHOR_TOL[kind], (1e-3, 1e-3), 4, round_frames)
    P = _scene(vp, oracle, name, est, rng)
    p = Planes(vp, kind)
    try:
        res, got = p.adaptive(first, max_frames, P, AP.ANCHOR_TOL[kind], (1e-3, 1e-3), 4, round_frames)
        _check(kind, want, res_want, res, got, (round_frames, max_frames))
        assert (want[0].flags & 1).any() and res_want["rounds"] == -(-max_frames // round_frames)
    finally:
        p.free()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("plane", (0, 1))
def test_flags_on_entry(vp, oracle, ctx, kind, plane):
    """a checkerboard of FROZEN in one record only: such a pixel receives nothing and neither of its records changes; a pattern in the
    flag bits 1..31 of both records is kept, also where the call freezes"""
    name, est, rng, first = SOFT
    frames = AP.anchor_frames(oracle, kind, name, est, rng, first)
    yy, xx = np.mgrid[0:H, 0:W]
    board = ((xx + yy) % 2).astype(np.uint32)
    want = AP.new_pair(W, H)
    for k in (0, 1):
        want[k].flags[:] = ((xx * 7 + yy * 13 + k) * 0x01010102 & 0xfffffffe).astype(np.uint32)
        want[k].acc[:] = F32(0.5 + k)                                   # what a frozen pixel keeps is what the caller left
        want[k].sum_y[:], want[k].sum_y2[:], want[k].n[:] = 0.25 * (k + 1), 0.125, 1 + k
    want[plane].flags |= board
    before = AP.copy_pair(want)
    P = _scene(vp, oracle, name, est, rng)
    p = Planes(vp, kind)
    try:
        p.upload(want)
        res_want = AP.render_adaptive_planes(want, frames, first, 24, AP.ANCHOR_TOL[kind], (1e-3, 1e-3), 8, 4)
        res, got = p.adaptive(first, 24, P, AP.ANCHOR_TOL[kind], (1e-3, 1e-3), 8, 4)
        _check(kind, want, res_want, res, got, plane)
        held = board == 1
        for k in (0, 1):
            assert got[k][held].tobytes() == before[k].acc[held].tobytes() and got[2 + k][held].tobytes() == before[k].records()[held].tobytes(), k
            assert np.array_equal(got[2 + k]["flags"] & 0xfffffffe, before[k].flags & 0xfffffffe)
        newly = ((want[1 - plane].flags & 1) != 0) & ~held
        assert newly.any() and res_want["samples"] <= 24 * int((~held).sum())
    finally:
        p.free()


@pytest.mark.parametrize("kind", KINDS)
def test_a_second_call_continues_the_first(vp, oracle, ctx, kind):
    """48 frames in one call equal 20 + 28 in two: the frozen set is what the two buffers say, nothing else is kept"""
    name, est, rng, first = SOFT
    want, res_want, _ = AP.anchor_expected(oracle, kind, name, est, rng, first)
    P = _scene(vp, oracle, name, est, rng)
    p = Planes(vp, kind)
    try:
        r1, _ = p.adaptive(first, 20, P, AP.ANCHOR_TOL[kind], **AP.ANCHOR_ARGS)
        r2, got = p.adaptive(first + 20, 28, P, AP.ANCHOR_TOL[kind], **AP.ANCHOR_ARGS)
        assert AP.same_pair(want, got) is None, AP.same_pair(want, got)
        assert r1["samples"] + r2["samples"] == res_want["samples"] and r1["rounds"] + r2["rounds"] == res_want["rounds"] == 12
        assert r2["active_left"] == res_want["active_left"] and (r1["frames_used"], r2["frames_used"]) == (20, 28)
        # everything that is left is active: a third call on a buffer pair whose pixels are all frozen renders nothing
        for k in (0, 1):
            rec = got[2 + k].copy()
            rec["flags"] |= 1 if k == 0 else 0
            p.rec[k].upload(rec)
        r3, after = p.adaptive(first + 48, 8, P, AP.ANCHOR_TOL[kind], **AP.ANCHOR_ARGS)
        assert r3 == {"samples": 0, "rounds": 0, "active_left": 0, "frames_used": 0}
        assert after[0].tobytes() == got[0].tobytes() and after[1].tobytes() == got[1].tobytes() and after[3].tobytes() == got[3].tobytes()
    finally:
        p.free()


@pytest.mark.parametrize("out", (0, 1))
def test_a_large_floor_takes_a_plane_out_of_the_decision(vp, oracle, ctx, out):
    """floor_y[out] = 1e30f: the call's frozen set is the other plane's own criterion (tests/test_adaptive_planes_cpu.py pins the
    restatement to adaptive_lib.render_adaptive on that plane alone)"""
    kind, name, est, rng, first = AP.FLOOR_CASE
    frames = AP.anchor_frames(oracle, kind, name, est, rng, first)
    floors = tuple(AP.BIG_FLOOR if k == out else 1e-3 for k in (0, 1))
    want = AP.new_pair(W, H)
    res_want = AP.render_adaptive_planes(want, frames, first, AP.ANCHOR_FRAMES, AP.FLOOR_TOL, floors, 8, 4)
    alone = AL.Stats(W, H)
    AL.render_adaptive(alone, lambda f: frames(f)[1 - out], first, AP.ANCHOR_FRAMES, AP.FLOOR_TOL[1 - out], 1e-3, 8, 4)
    assert np.array_equal(alone.flags, want[0].flags) and 0 < int(alone.flags.sum()) < W * H
    P = _scene(vp, oracle, name, est, rng)
    p = Planes(vp, kind)
    try:
        res, got = p.adaptive(first, AP.ANCHOR_FRAMES, P, AP.FLOOR_TOL, floors, 8, 4)
        _check(kind, want, res_want, res, got, out)
    finally:
        p.free()


# ------------------------------------------------------------------------------------------------------------------- shards
@pytest.mark.parametrize("kind", KINDS)
def test_three_shards_touch_their_own_tiles_and_make_up_the_whole(vp, oracle, ctx, kind):
    name, est, rng, first = SOFT
    want, res_want, _ = AP.anchor_expected(oracle, kind, name, est, rng, first)
    P = _scene(vp, oracle, name, est, rng)
    sentinel = np.zeros((H, W), vp.PIXEL_STATS_DTYPE)
    sentinel["sum_y"], sentinel["sum_y2"], sentinel["n"], sentinel["flags"] = -7.25, 1e300, 0xabcd0123, 0xfffffff0      # (FROZEN clear: it would be sampled)
    p, shared = Planes(vp, kind), Planes(vp, kind)
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
            res, got = p.adaptive(first, AP.ANCHOR_FRAMES, P, AP.ANCHOR_TOL[kind], **AP.ANCHOR_ARGS)
            for k in (0, 1):
                assert got[2 + k][~owned].tobytes() == sentinel[~owned].tobytes(), (r, NAMES[kind][k])            # unowned records: untouched
                assert not got[k][~owned].any()
                assert AL.equal_bits(got[k][owned], want[k].acc[owned]) and got[2 + k][owned].tobytes() == want[k].records()[owned].tobytes(), (r, k)
            assert res["samples"] == int(want[0].n[owned].sum()) and res["active_left"] == int(((want[0].flags[owned] & 1) == 0).sum())
            res, _ = shared.adaptive(first, AP.ANCHOR_FRAMES, P, AP.ANCHOR_TOL[kind], **AP.ANCHOR_ARGS)             # ... and all ranks into one set of buffers
            samples, left = samples + res["samples"], left + res["active_left"]
            seen += owned
        assert (seen == 1).all()
        assert AP.same_pair(want, shared.download()) is None
        assert (samples, left) == (res_want["samples"], res_want["active_left"])
    finally:
        vp.set_shard(0, 1)
        p.free()
        shared.free()


# -------------------------------------------------------------------------------------------------------------- the staging cap
STAGE_TOL, STAGE_ARGS, STAGE_SIZE, STAGE_FRAMES = (0.15, 0.15), dict(floor_y=(1e-3, 1e-3), min_frames=17, round_frames=8), (160, 120), 24


@pytest.mark.parametrize("kind", KINDS)
def test_a_staging_cap_that_splits_every_round_into_launches(vp, oracle, monkeypatch, kind):
    """VP_STAGE_MB=1 in a context of its own, 160 x 120: a frame of all pixels is 300 KiB of staging per plane, so the rounds of 8 frames
    are split into launches -- and give the bits of one launch each.  Four fifths of the pixels of this view are per-pixel constants,
    which freeze at the first decision whatever the tolerance, and what is left of a later round would fit one launch: min_frames is
    17, so that every pixel is active in all three rounds, each of which is then three launches (layers) or eight (groups, two
    planes), and the decisions fall at the end of the third.  A reduce that judged a record after a part of that round (n = 17 .. 23)
    would freeze pixels whose criterion holds there and not at 24.  The restatement is fed by one-frame plane calls of the library.
    The launches of a round follow from its active pixels: ceil(frames / floor(1 MiB / (pixels x 16 x planes)))."""
    monkeypatch.setenv("VP_STAGE_MB", "1")
    c = vp.Context(0)
    monkeypatch.delenv("VP_STAGE_MB", raising=False)
    try:
        with c:
            P = _scene(vp, oracle, "soft", 1, 1, size=STAGE_SIZE)
            frames, q = _library_pair(vp, kind, P, *STAGE_SIZE)
            p = Planes(vp, kind, *STAGE_SIZE)
            try:
                want = AP.new_pair(*STAGE_SIZE)
                active = []

                def counting(f):
                    if (f - 3) % 8 == 0:
                        active.append(int(AP.active_mask(want, AL.all_pixels(*STAGE_SIZE)).sum()))
                    return frames(f)
                res_want = AP.render_adaptive_planes(want, counting, 3, STAGE_FRAMES, STAGE_TOL, **STAGE_ARGS)
                vp.synchronize()
                vp.render_time_ms(reset=True)
                res, got = p.adaptive(3, STAGE_FRAMES, P, STAGE_TOL, **STAGE_ARGS)
                launches = vp.render_time_ms(reset=True)[1]
                _check(kind, want, res_want, res, got, "capped")
                planes = 2 if kind == "groups" else 1
                per_round = [-(-8 // max(1, (1 << 20) // (a * 16 * planes))) for a in active]
                print(kind, "active per round", active, "launches per round", per_round, "measured", launches)
                assert len(active) == res_want["rounds"] == 3 and launches == sum(per_round)
                assert min(per_round) >= 2, (active, per_round)                                  # every round was split
                frozen = (want[0].flags & 1) != 0
                nd = want[1].n.astype(np.float64)
                noisy = (nd * want[1].sum_y2 - want[1].sum_y * want[1].sum_y > 0) | (nd * want[0].sum_y2 - want[0].sum_y * want[0].sum_y > 0)
                print(kind, "frozen", int(frozen.sum()), "noisy", int(noisy.sum()), "noisy and frozen", int((noisy & frozen).sum()))
                assert (noisy & frozen).any() and (noisy & ~frozen).any()                        # decisions of both kinds on pixels with variance
            finally:
                p.free()
                q.free()
    finally:
        c.destroy()


# -------------------------------------------------------------------------------------------------------------------- variants
VARIANTS = [("julia", 0, 61.0, 1, "kernel"), ("julia", 0, 64.0, 1, "constants"), ("julia", 1, 61.0, 1, "kernel"), ("soft", 2, None, 2, None), ("soft16", 1, None, 1, None)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,est,density,sub,light", VARIANTS, ids=["%s-est%d-d%s-S%d" % v[:4] for v in VARIANTS])
def test_variants_equal_the_restatement_on_the_librarys_own_frames(vp, oracle, ctx, kind, name, est, density, sub, light):
    """the light class as a kernel (a majorant of 61) and as constants (64: tests/test_layers_gpu.py has the reasons), the bounded
    estimator under vp_set_subpixel(2), a binary16 volume: the adaptive call against the restatement fed by one-frame plain plane calls
    in the same state.  Frames 6..29 cross the decomposition estimator's switch."""
    first, n = 6, 24
    tol = {"groups": (0.3, 0.1), "layers": (0.2, 0.3)}[kind]
    P = _scene(vp, oracle, name, est, 1, density=density)
    vp.set_subpixel(sub)
    frames, q = _library_pair(vp, kind, P)
    p = Planes(vp, kind)
    try:
        if light:
            general, lightpx, miss = vp.pixel_lists(P)
            assert len(lightpx) > 0 and len(miss) > 0 and len(general) > 0
        want = AP.new_pair(W, H)
        res_want = AP.render_adaptive_planes(want, frames, first, n, tol, (1e-3, 1e-3), 4, 4)
        if light:               # (of the plain one-frame calls just made, on the whole lists: a later round's list may hold no light pixel)
            assert vp.last_light_const() == (light == "constants")
        res, got = p.adaptive(first, n, P, tol, (1e-3, 1e-3), 4, 4)
        _check(kind, want, res_want, res, got, (name, est, density, sub))
        frozen = (want[0].flags & 1) != 0
        assert frozen.any() and not frozen.all()
    finally:
        vp.set_subpixel(1)
        p.free()
        q.free()


# --------------------------------------------------------------------------------------------------------- nothing left behind
@pytest.mark.parametrize("kind,name,est", (("groups", "julia", 1), ("layers", "soft", 0)))
def test_the_call_leaves_nothing_behind(vp, oracle, ctx, kind, name, est):
    P = _scene(vp, oracle, name, est, 1)
    p, g, b, r = Planes(vp, kind), Planes(vp, "groups"), vp.DeviceBuffer(W, H), vp.StatsBuffer(W, H)
    try:
        def others():
            out = []
            b.reset()
            vp.render_frames(b.ptr, 6, 12, P)
            out.append(b.download().tobytes())
            g.reset()
            out += [a.tobytes() for a in g.plain(6, 12, P)]
            b.reset()
            r.reset()
            res = vp.render_adaptive(b.ptr, r.ptr, 6, 12, P, 0.2, 1e-3, 4, 4)
            out += [b.download().tobytes(), r.download().tobytes(), repr(sorted(res.items()))]
            out += [a.tobytes() for a in vp.pixel_lists(P)]
            return out

        before = others()
        res, got = p.adaptive(6, 12, P, (0.3, 0.3), (1e-3, 1e-3), 4, 4)
        assert others() == before
        assert 0 < res["active_left"] < W * H and np.frombuffer(before[0], F32).max() > 0
    finally:
        p.free()
        g.free()
        b.free()
        r.free()


# --------------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("kind", KINDS)
def test_refusals_touch_no_buffer_and_leave_the_context_usable(vp, oracle, ctx, kind):
    name, est, rng, first = SOFT
    want, res_want, _ = AP.anchor_expected(oracle, kind, name, est, rng, first)
    P = _scene(vp, oracle, name, est, rng)
    p = Planes(vp, kind)
    fname = "vp_render_adaptive_%s" % kind
    f = getattr(vp.lib(), fname)
    try:
        mark = np.full((H, W, 4), 7.25, F32)
        rmark = np.zeros((H, W), vp.PIXEL_STATS_DTYPE)
        rmark["sum_y"], rmark["sum_y2"], rmark["n"], rmark["flags"] = 3.5, 12.25, 5, 0x10
        for b in p.acc:
            b.upload(mark)
        for b in p.rec:
            b.upload(rmark)

        def refused(code, word, ptrs=None, first=first, maxf=12, tol=(0.1, 0.1), fl=(1e-3, 1e-3), min_frames=4, round_frames=4):
            a = vp.AdaptivePlanes((C.c_float * 2)(*tol), (C.c_float * 2)(*fl), min_frames, round_frames)
            res = vp.AdaptiveResult(7, 7, 7, 7)
            rc = f(*(ptrs or p.ptrs()), first, maxf, C.byref(P), C.byref(a), C.byref(res))
            vp.synchronize()
            msg = vp.lib().vp_last_error().decode()
            assert rc == code and word in msg and (fname in msg or code == E_NOOPACITY), (rc, msg)
            assert res.as_dict() == {"samples": 0, "rounds": 0, "active_left": 0, "frames_used": 0}
            got = p.download()
            assert got[0].tobytes() == mark.tobytes() == got[1].tobytes() and got[2].tobytes() == rmark.tobytes() == got[3].tobytes(), word

        a0, a1, r0, r1 = p.ptrs()
        refused(E_ARG, "null", ptrs=(a0, None, r0, r1))
        refused(E_ARG, "different", ptrs=(a0, a0, r0, r1))
        refused(E_ARG, "different", ptrs=(a0, a1, r1, r1))
        refused(E_ARG, "out of range", maxf=0)
        refused(E_ARG, "min_frames", min_frames=1)
        refused(E_ARG, "round_frames", round_frames=0)
        refused(E_ARG, "rel_tol", tol=(0.1, float("nan")))
        refused(E_ARG, "floor_y", fl=(-1.0, 0.0))
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
        res, got = p.adaptive(first, AP.ANCHOR_FRAMES, P, AP.ANCHOR_TOL[kind], **AP.ANCHOR_ARGS)      # the context stays usable
        _check(kind, want, res_want, res, got, "after the refusals")
    finally:
        vp.set_envmap_sampling(vp.ENV_PASSIVE)
        vp.set_arithmetic(vp.ARITH_EXACT)
        vp.set_tracking(vp.TRACK_SPECTRAL)
        vp.enable_counters(False)
        p.free()


# ------------------------------------------------------------------------------------------------------------- the output stage
@pytest.mark.parametrize("kind", KINDS)
def test_scale_by_count_per_plane_then_the_output_stage(vp, oracle, ctx, kind):
    """each plane by ITS records' counts (vp_scale_by_count), then vp_relight / vp_composite of the two means with scale 1, against the
    numpy restatements"""
    name, est, rng, first = SOFT
    rgb = (0.7, 0.1, 9.0)
    P = _scene(vp, oracle, name, est, rng)
    p, mean, dst = Planes(vp, kind), (vp.DeviceBuffer(W, H), vp.DeviceBuffer(W, H)), vp.DeviceBuffer(W, H)
    try:
        res, got = p.adaptive(first, AP.ANCHOR_FRAMES, P, AP.ANCHOR_TOL[kind], **AP.ANCHOR_ARGS)
        assert len(set(got[2]["n"].ravel().tolist())) > 2                          # the counts differ from pixel to pixel
        want_mean = [AL.scale_by_count(got[k], got[2 + k]["n"], 1.0) for k in (0, 1)]
        for k in (0, 1):
            vp.scale_by_count(mean[k].ptr, p.acc[k].ptr, p.rec[k].ptr, W * H, 1.0)
            assert mean[k].download().tobytes() == want_mean[k].tobytes(), NAMES[kind][k]
        if kind == "groups":
            gains = ((2.0, 0.5, 0.25), (0.1, 1.0, 3.0))
            vp.relight(dst.ptr, mean[0].ptr, mean[1].ptr, W * H, 1.0, *gains)
            want = GL.relight(want_mean[0], want_mean[1], 1.0, *gains)
        else:
            vp.composite(dst.ptr, mean[0].ptr, mean[1].ptr, W * H, 1.0, plate_rgb=rgb)
            want = LL.composite(want_mean[0], want_mean[1], 1.0, rgb=rgb)
        assert dst.download().tobytes() == want.tobytes() and want[..., :3].max() > 0
    finally:
        for b in mean + (dst,):
            b.free()
        p.free()
