"""Adaptive sampling on half-buffers on the GPU (include/volpath.h vp_render_adaptive_halves, vp_render_adaptive_planes_halves; DESIGN.md
section 2.20).

Every comparison is at tolerance 0: accumulators, sum_y and sum_y2 by their bits, n and flags by value, the result struct field by
field -- against the restatement of tests/adaptive_halves_lib.py fed by the CPU oracle's frames (the anchors) or by the library's own
one-frame calls in the same context state.  The scene is Julia-32 at 64 x 48 unless a case says otherwise.  Each test runs in a context
of its own."""
import ctypes as C

import numpy as np
import pytest

import adaptive_halves_lib as AH
import adaptive_lib as AL
import halves_lib as HL
import large_image_cases as LI
import layers_lib as LL
import plane_stats_lib as PS
import scenes

pytestmark = pytest.mark.gpu

W, H = AL.ANCHOR_W, AL.ANCHOR_H
E_STATE, E_ARG, E_NOOPACITY = -2, -3, -4
F32 = np.float32
NAN = float("nan")
BEAUTY, LAYERS, GROUPS, GROUP_LAYERS = 0, AH.LAYERS, AH.GROUPS, AH.GROUP_LAYERS
PLANE_MODES = [LAYERS, GROUPS, GROUP_LAYERS]
MODE_IDS = ["layers", "groups", "group_layers"]
EST = {"global": 0, "decomp": 1}
RNG = {"philox": 1, "philox7": 2}
FLOORS = {BEAUTY: (1e-3,), LAYERS: (1e-3, 1e-2), GROUPS: (1e-3, 1e-3), GROUP_LAYERS: (1e-3, 1e-3, 1e-2)}


@pytest.fixture
def ctx(vp):
    c = vp.Context(0)
    try:
        with c:
            yield c
    finally:
        c.destroy()


def _scene(vp, est, rng_mode, key=(1, 2), size=(W, H), camera=None, **param):
    """Julia-32 under the suite's environment and sun: the anchors' scene (default medium) or, with `param`, layers_lib's thin one"""
    vp.init_volume(vp.julia_volume(32), brick=1, linear=True)
    vp.init_envmap(scenes.synthetic_env())
    vp.set_sun(scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER)
    if camera is None:
        vp.set_camera()
    else:
        vp.set_camera(camera)
    vp.set_estimator(est)
    vp.set_rng(rng_mode, key)
    vp.set_tracking(vp.TRACK_SPECTRAL)
    vp.set_envmap_sampling(vp.ENV_PASSIVE)
    vp.set_shard(0, 1)
    if est == 1:
        vp.precompute_opacity(scenes.DEFAULT_SUN_DIR)
    return vp.make_param(size[0], size[1], **param)


class Halves:
    """the 2 N accumulators and 2 N record buffers of a call on halves (mode 0: the beauty image, N = 1); downloads come in the order
    adaptive_halves_lib.same_halves takes: h0's accumulators, h1's accumulators, h0's records, h1's records"""

    def __init__(self, vp, mode, w=W, h=H):
        self.vp, self.mode, self.N = vp, mode, len(AH.PLANES[mode])
        self.acc = [[vp.DeviceBuffer(w, h) for _ in range(self.N)] for _ in (0, 1)]
        self.rec = [[vp.StatsBuffer(w, h) for _ in range(self.N)] for _ in (0, 1)]

    def all(self):
        return self.acc[0] + self.acc[1] + self.rec[0] + self.rec[1]

    def half(self, h):
        return [(a.ptr, r.ptr) for a, r in zip(self.acc[h], self.rec[h])]

    def upload(self, halves):
        for h in (0, 1):
            for k in range(self.N):
                self.acc[h][k].upload(halves[h][k].acc)
                self.rec[h][k].upload(halves[h][k].records().astype(self.vp.PIXEL_STATS_DTYPE))

    def adaptive(self, first, max_frames, P, rel_tol, floor_y, min_frames, round_frames, pad=()):
        """the adaptive call; `pad`: what the entries of rel_tol and floor_y beyond the mode's planes hold (ignored, garbage included)"""
        if self.mode == BEAUTY:
            res = self.vp.render_adaptive_halves(self.acc[0][0].ptr, self.acc[1][0].ptr, self.rec[0][0].ptr, self.rec[1][0].ptr, first, max_frames, P,
                                                 np.ravel(rel_tol)[0], np.ravel(floor_y)[0], min_frames, round_frames)
        else:
            pad = tuple(pad)[:3 - self.N]
            res = self.vp.render_adaptive_planes_halves(self.mode, self.half(0), self.half(1), first, max_frames, P, tuple(rel_tol) + pad, tuple(floor_y) + pad,
                                                        min_frames, round_frames)
        return res, self.download()

    def uniform(self, first, n, P):
        if self.mode == BEAUTY:
            self.vp.render_frames_halves_stats(self.acc[0][0].ptr, self.acc[1][0].ptr, self.rec[0][0].ptr, self.rec[1][0].ptr, first, n, P)
        else:
            self.vp.render_frames_planes_halves_stats(self.mode, self.half(0), self.half(1), first, n, P)
        return self.download()

    def download(self):
        return tuple(b.download() for b in self.all())

    def reset(self):
        for b in self.all():
            b.reset()

    def free(self):
        for b in self.all():
            b.free()


def _check(want, res_want, res, got, what):
    bad = AH.same_halves(want, got)
    assert bad is None, (what, bad)
    assert res == res_want, (what, res, res_want)


def _library_frames(vp, mode, P, w=W, h=H):
    """(frame_planes(f) through one-frame plain calls of the library in the current state, the buffers to free)"""
    if mode == BEAUTY:
        frame, buf = AL.library_frames(vp, P)
        return AH.beauty(frame), [buf]
    bufs = [vp.DeviceBuffer(w, h) for _ in AH.PLANES[mode]]
    call = {LAYERS: vp.render_frames_layers, GROUPS: vp.render_frames_groups, GROUP_LAYERS: vp.render_frames_group_layers}[mode]
    return PS.library_frames(lambda f: call(*[b.ptr for b in bufs], f, 1, P), bufs), bufs


# ------------------------------------------------------------------------------------------------------- 1. the anchors, 2. odd start
@pytest.mark.parametrize("anchor,first", [(AL.ANCHOR1, 0), (AL.ANCHOR2, 0)], ids=["anchor1", "anchor2"])
def test_anchors_equal_the_oracle_restatement(vp, oracle, ctx, anchor, first):
    frames = AH.beauty(AH.anchor_frames(oracle, scenes, anchor))
    args = AL.anchor_args(anchor)
    want = AH.new_halves(W, H)
    res_want = AH.render_adaptive_halves(want, frames, first, anchor["max_frames"], **args)
    c = AH.census(want, anchor["min_frames"], anchor["max_frames"])
    print("the oracle's expectation:", res_want, c)
    assert c["at_min"] >= 1 and c["between"] >= 1 and c["all_frames"] >= 1 and c["active"] >= 1        # (tests/test_adaptive_halves_cpu.py)
    P = _scene(vp, EST[anchor["est"]], RNG[anchor["rng"]], anchor["key"])
    t = Halves(vp, BEAUTY)
    try:
        res, got = t.adaptive(first, anchor["max_frames"], P, **args)
        print("the library:", res)
        _check(want, res_want, res, got, anchor["est"])
    finally:
        t.free()


def test_an_odd_start_on_prefilled_buffers(vp, oracle, ctx):
    """ANCHOR1 from frame 1: the parity of the halves flips, the first frame of every round goes to half 1, and the last round is cut to
    one frame, which half 1 alone receives.  The buffers hold something already (halves_lib.prefill): flag bits other than FROZEN, which
    must be kept, and pixels frozen in ONE half's record only, which must receive nothing.  The -0.0f among the accumulators must
    survive in a half that gets no frame of a launch: every round of two frames or more feeds both halves, so that is shown by a call
    of one frame on the same buffers"""
    a = AL.ANCHOR1
    first, n = 1, 41
    frames = AH.beauty(AH.anchor_frames(oracle, scenes, a))
    args = AL.anchor_args(a)
    want = AH.prefilled(W, H, 1, 70)
    yy, xx = np.mgrid[0:H, 0:W]
    for h in (0, 1):
        want[h][0].flags[:] = (((xx * 5 + yy * 3 + h) % 7) << 1).astype(np.uint32)      # bits 1..3, FROZEN clear
    held0, held1 = (xx + yy) % 5 == 0, (xx + yy) % 5 == 2                  # frozen in half 0's record only / in half 1's only
    want[0][0].flags[held0] |= 1
    want[1][0].flags[held1] |= 1
    held = held0 | held1
    before = AH.copy_halves(want)
    res_want = AH.render_adaptive_halves(want, frames, first, n, **args)
    assert res_want["rounds"] == 6 and res_want["frames_used"] == n and HL.half_of_frame(first) == 1
    newly = ((want[0][0].flags & 1) != 0) & ~held
    assert newly.any() and ((want[1][0].flags & 1) != 0)[newly].all() and 0 < res_want["active_left"] < int((~held).sum())
    P = _scene(vp, EST[a["est"]], RNG[a["rng"]], a["key"])
    t = Halves(vp, BEAUTY)
    try:
        t.upload(before)
        res, got = t.adaptive(first, n, P, **args)
        _check(want, res_want, res, got, "odd start")
        for h in (0, 1):
            assert got[h][held].tobytes() == before[h][0].acc[held].tobytes() and got[2 + h][held].tobytes() == before[h][0].records()[held].tobytes(), h
            assert np.array_equal(got[2 + h]["flags"] & 0xfffffffe, before[h][0].flags & 0xfffffffe) and (before[h][0].flags & 0xfffffffe).any()
        # one frame: the other half keeps every byte, its -0.0f included
        t.upload(before)
        one = AH.copy_halves(before)
        one_want = AH.render_adaptive_halves(one, frames, first + 1, 1, **args)
        res, got = t.adaptive(first + 1, 1, P, **args)
        _check(one, one_want, res, got, "one frame")
        other = 1 - HL.half_of_frame(first + 1)
        zero = before[other][0].acc == 0
        assert np.signbit(before[other][0].acc[zero]).any() and (~np.signbit(before[other][0].acc[zero])).any()
        assert got[other].tobytes() == before[other][0].acc.tobytes() and np.array_equal(got[2 + other]["n"], before[other][0].n)
        assert res["samples"] == int((~held).sum())
    finally:
        t.free()


# ------------------------------------------------------------------------------------------------------- 3. continuation
def test_a_second_call_continues_the_first(vp, oracle, ctx):
    """40 frames, then 56 on the same buffers: each against the restatement run on the same state; and the two equal the one call of 96,
    because the round divides 40"""
    a = AL.ANCHOR1
    frames = AH.beauty(AH.anchor_frames(oracle, scenes, a))
    args = AL.anchor_args(a)
    want = AH.new_halves(W, H)
    w1 = AH.render_adaptive_halves(want, frames, 0, 40, **args)
    mid = AH.copy_halves(want)
    w2 = AH.render_adaptive_halves(want, frames, 40, 56, **args)
    whole = AH.new_halves(W, H)
    AH.render_adaptive_halves(whole, frames, 0, 96, **args)
    P = _scene(vp, EST[a["est"]], RNG[a["rng"]], a["key"])
    t = Halves(vp, BEAUTY)
    try:
        r1, got = t.adaptive(0, 40, P, **args)
        _check(mid, w1, r1, got, "first call")
        r2, got = t.adaptive(40, 56, P, **args)
        _check(want, w2, r2, got, "second call")
        assert AH.same_halves(whole, got) is None and 0 < r2["active_left"] < r1["active_left"]
        # everything that is left is active: frozen in one record, it is left alone
        rec = got[2].copy()
        rec["flags"] |= 1
        t.rec[0][0].upload(rec)
        r3, after = t.adaptive(96, 8, P, **args)
        assert r3 == {"samples": 0, "rounds": 0, "active_left": 0, "frames_used": 0}
        assert [x.tobytes() for x in after[:2] + after[3:]] == [x.tobytes() for x in got[:2] + got[3:]]
    finally:
        t.free()


# ------------------------------------------------------------------------------------------------------- 4. a sub-pixel factor
@pytest.mark.parametrize("first", [0, 2])
def test_subpixel_rounds_that_lie_in_one_half_or_straddle(vp, oracle, ctx, first):
    """S = 2, rounds of 4: from frame 0 every round lies in one half (blocks of S^2 = 4 frames alternate), so a pixel has two samples in
    both halves after the second round at the earliest and nothing may freeze before it; from frame 2 every round straddles"""
    P = _scene(vp, 0, 2)
    vp.set_subpixel(2)
    frames, bufs = _library_frames(vp, BEAUTY, P)
    t = Halves(vp, BEAUTY)
    try:
        args = dict(rel_tol=0.2, floor_y=1e-3, min_frames=4, round_frames=4)
        want = AH.new_halves(W, H)
        one = AH.copy_halves(want)
        r_one = AH.render_adaptive_halves(one, frames, first, 4, S=2, **args)
        frozen_one = AH.frozen_mask(one)
        if first == 0:
            assert not frozen_one.any() and (one[1][0].n == 0).all() and (one[0][0].n == 4).all()      # min_frames is met, half 1 is empty
        else:
            assert frozen_one.any() and (one[0][0].n == 2).all() and (one[1][0].n == 2).all()
        res_want = AH.render_adaptive_halves(want, frames, first, 24, S=2, **args)
        frozen = AH.frozen_mask(want)
        assert frozen.any() and not frozen.all()
        res, got = t.adaptive(first, 24, P, **args)
        _check(want, res_want, res, got, ("S = 2", first))
        t.reset()
        res, got = t.adaptive(first, 4, P, **args)
        _check(one, r_one, res, got, ("S = 2, one round", first))
    finally:
        vp.set_subpixel(1)
        t.free()
        for b in bufs:
            b.free()


# ------------------------------------------------------------------------------------------------------- 5. a shard
def test_rank_1_of_3_touches_only_its_pixels(vp, oracle, ctx):
    a = AL.ANCHOR2
    frames = AH.beauty(AH.anchor_frames(oracle, scenes, a))
    args = AL.anchor_args(a)
    owned = AL.owned_pixels(vp, W, H, 1, 3)
    assert owned.any() and (~owned).any()
    want = AH.prefilled(W, H, 1, 80)
    for h in (0, 1):
        want[h][0].flags[:] &= 0xfffffffe                                   # (FROZEN clear everywhere: an unowned pixel would be sampled)
        for name in ("acc", "sum_y", "sum_y2", "n"):
            getattr(want[h][0], name)[owned] = 0
    before = AH.copy_halves(want)
    res_want = AH.render_adaptive_halves(want, frames, 0, a["max_frames"], owned=owned, **args)
    P = _scene(vp, EST[a["est"]], RNG[a["rng"]], a["key"])
    t = Halves(vp, BEAUTY)
    try:
        t.upload(before)
        vp.set_shard(1, 3)
        res, got = t.adaptive(0, a["max_frames"], P, **args)
        _check(want, res_want, res, got, "rank 1 of 3")
        for h in (0, 1):
            assert got[h][~owned].tobytes() == before[h][0].acc[~owned].tobytes() and got[2 + h][~owned].tobytes() == before[h][0].records()[~owned].tobytes(), h
        assert 0 < res["active_left"] < int(owned.sum())
    finally:
        vp.set_shard(0, 1)
        t.free()


# ------------------------------------------------------------------------------------------------------- 6. the staging cap
@pytest.mark.parametrize("mode", [BEAUTY, GROUP_LAYERS], ids=["beauty", "group_layers"])
def test_a_staging_cap_that_splits_the_rounds_into_launches(vp, oracle, monkeypatch, mode):
    """VP_STAGE_MB=1 in a context of its own, 160 x 120, rounds of 8: a frame of all pixels is 300 KiB of staging per staging plane, so
    the first round goes in several launches (three for the beauty image, eight for group layers' two staging planes) -- and the call
    gives the bits of the same call under the default cap, where every round is one launch"""
    size, first, n = (160, 120), 3, 24
    tol, fl = (0.15,) * len(AH.PLANES[mode]), FLOORS[mode]
    args = dict(min_frames=10, round_frames=8)
    kw = dict(LL.param_kw("julia")) if mode != BEAUTY else {}
    out = []
    for capped in (True, False):
        if capped:
            monkeypatch.setenv("VP_STAGE_MB", "1")
        c = vp.Context(0)
        monkeypatch.delenv("VP_STAGE_MB", raising=False)
        try:
            with c:
                P = _scene(vp, 0, 1, size=size, **kw)
                t = Halves(vp, mode, *size)
                try:
                    vp.synchronize()
                    vp.render_time_ms(reset=True)
                    res, got = t.adaptive(first, n, P, tol, fl, **args)
                    out.append((res, got, vp.render_time_ms(reset=True)[1]))
                finally:
                    t.free()
        finally:
            c.destroy()
    (res_c, got_c, launches_c), (res_u, got_u, launches_u) = out
    print("launches capped", launches_c, "uncapped", launches_u, res_c)
    assert res_c == res_u and res_c["rounds"] == 3
    assert [x.tobytes() for x in got_c] == [x.tobytes() for x in got_u]
    planes = 2 if mode == GROUP_LAYERS else 1
    # (the first round holds every pixel: ceil(8 / floor(1 MiB / (pixels x 16 x staging planes))) launches under the cap)
    assert launches_c >= -(-8 // ((1 << 20) // (size[0] * size[1] * 16 * planes))) >= 3 and launches_c > launches_u >= 1
    N = len(AH.PLANES[mode])
    frozen = (got_c[2 * N]["flags"] & 1) != 0
    nd = got_c[2 * N]["n"].astype(np.float64)
    noisy = nd * got_c[2 * N]["sum_y2"] - got_c[2 * N]["sum_y"] ** 2 > 0
    assert (noisy & frozen).any() and (noisy & ~frozen).any() and 0 < res_c["active_left"] < size[0] * size[1]


# ------------------------------------------------------------------------------------------------------- 7. plane modes
PLANE_TOL = {LAYERS: (0.2, 0.3), GROUPS: (0.3, 0.1), GROUP_LAYERS: (0.3, 0.1, 0.3)}


@pytest.mark.parametrize("alone", [None, 0], ids=["all-planes", "plane0-alone"])
@pytest.mark.parametrize("est", [0, 1], ids=["global", "decomp"])
@pytest.mark.parametrize("mode", PLANE_MODES, ids=MODE_IDS)
def test_plane_modes_equal_the_restatement_on_the_librarys_own_frames(vp, oracle, ctx, mode, est, alone):
    """32 frames in rounds of 4 from frame 3 (odd: rounds begin on half 1; the decomposition estimator crosses its switch at frame 11),
    layers_lib's thin Julia medium, all three pixel classes in the view.  `alone`: floor_y = 1e30f on every plane but that one -- the
    frozen set is then that plane's own pooled rule.  The entries of rel_tol and floor_y beyond the mode's planes hold NaN."""
    first, n, N = 3, 32, len(AH.PLANES[mode])
    P = _scene(vp, est, 2, key=LL.KEY, **LL.param_kw("julia"))
    general, light, miss = vp.pixel_lists(P)
    assert len(general) > 0 and len(light) > 0 and len(miss) > 0
    frames, bufs = _library_frames(vp, mode, P)
    t = Halves(vp, mode)
    try:
        tol = PLANE_TOL[mode]
        fl = FLOORS[mode] if alone is None else tuple(FLOORS[mode][k] if k == alone else 1e30 for k in range(N))
        want = AH.new_halves(W, H, N)
        res_want = AH.render_adaptive_halves(want, frames, first, n, tol, fl, 4, 4)
        frozen = AH.frozen_mask(want)
        assert frozen.any() and not frozen.all() and 0 < res_want["active_left"] < W * H
        if alone is not None:
            own = AH.new_halves(W, H, 1)
            AH.render_adaptive_halves(own, lambda f: (frames(f)[alone],), first, n, tol[alone], fl[alone], 4, 4)
            assert np.array_equal(AH.frozen_mask(own), frozen)
        res, got = t.adaptive(first, n, P, tol, fl, 4, 4, pad=(NAN, NAN))
        _check(want, res_want, res, got, (mode, est, alone))
    finally:
        t.free()
        for b in bufs:
            b.free()


# ------------------------------------------------------------------------------------------------------- 8. past one scan chunk
AWAY = (0.0, 0.207912, 0.978148, 3.922986, 0.0, 0.978148, -0.207912, 100.0, -1.0, 0.0, 0.0, 0.03)      # the default camera, lifted far off the box


@pytest.mark.parametrize("mode", [GROUPS, GROUP_LAYERS], ids=["groups-4-records", "group_layers-6-records"])
def test_a_list_past_one_scan_chunk(vp, ctx, mode):
    """the compaction's 4- and 6-record instances on a list of more than 1024 x 1024 slots: every camera ray misses the box, so every
    pixel is a constant; 4 frames in rounds of 2 with min_frames 4 -- after round 1 each half holds one sample and nothing freezes,
    after round 2 every pixel does.  Then a third call finds nothing to do"""
    name = next(k for k in sorted(LI.SIZES) if LI.scan_chunks(*LI.SIZES[k][:2]) > 1)
    Wl, Hl, _ = LI.SIZES[name]
    assert Wl * Hl > LI.CHUNK_SLOTS
    P = _scene(vp, 0, 2, size=(Wl, Hl), camera=AWAY, **LL.param_kw("julia"))
    general, light, miss = vp.pixel_lists(P)
    assert len(general) == 0 and len(light) == 0 and len(miss) == Wl * Hl
    N = len(AH.PLANES[mode])
    t = Halves(vp, mode, Wl, Hl)
    try:
        tol, fl = (0.1,) * N, FLOORS[mode]
        res = t.vp.render_adaptive_planes_halves(mode, t.half(0), t.half(1), 0, 2, P, tol, fl, 4, 2)
        assert res == {"samples": 2 * Wl * Hl, "rounds": 1, "active_left": Wl * Hl, "frames_used": 2}
        for h in (0, 1):
            for k in range(N):
                rec = t.rec[h][k].download()
                assert (rec["n"] == 1).all() and not rec["flags"].any(), (h, k)
        for b in t.all():
            b.reset()
        res = t.vp.render_adaptive_planes_halves(mode, t.half(0), t.half(1), 0, 4, P, tol, fl, 4, 2)
        assert res == {"samples": 4 * Wl * Hl, "rounds": 2, "active_left": 0, "frames_used": 4}
        sums = []
        for h in (0, 1):
            for k in range(N):
                rec = t.rec[h][k].download()
                assert (rec["n"] == 2).all() and (rec["flags"] == 1).all(), (h, k)
                sums.append(rec["sum_y"])
        assert any((s > 0).all() for s in sums)
        res = t.vp.render_adaptive_planes_halves(mode, t.half(0), t.half(1), 4, 4, P, tol, fl, 4, 2)
        assert res == {"samples": 0, "rounds": 0, "active_left": 0, "frames_used": 0}
    finally:
        vp.set_camera()
        t.free()


# ------------------------------------------------------------------------------------------------------- 9. nothing left behind
def _census(vp, reset=False):
    return {"render": vp.launch_census(vp.CENSUS_EXACT, vp.CENSUS_RENDER, reset=reset), LAYERS: vp.launch_census(vp.CENSUS_EXACT, vp.CENSUS_LAYERS, reset=reset),
            GROUPS: vp.groups_census(reset=reset), GROUP_LAYERS: vp.group_layers_census(reset=reset),
            "approach": vp.launch_census(vp.CENSUS_EXACT, vp.CENSUS_APPROACH, reset=reset)}


@pytest.mark.parametrize("mode", [BEAUTY] + PLANE_MODES, ids=["beauty"] + MODE_IDS)
def test_the_call_leaves_nothing_behind_and_launches_the_underlying_modes_instances(vp, oracle, ctx, mode):
    P = _scene(vp, 0, 2, key=LL.KEY, **LL.param_kw("julia"))
    N = len(AH.PLANES[mode])
    t, u, b, r = Halves(vp, mode), Halves(vp, mode), vp.DeviceBuffer(W, H), vp.StatsBuffer(W, H)
    try:
        def others():
            out = []
            b.reset()
            vp.render_frames(b.ptr, 6, 12, P)
            out.append(b.download().tobytes())
            assert vp.last_pipelined() == 1
            b.reset()
            r.reset()
            res = vp.render_adaptive(b.ptr, r.ptr, 6, 12, P, 0.2, 1e-3, 4, 4)
            out += [b.download().tobytes(), r.download().tobytes(), repr(sorted(res.items()))]
            out += [a.tobytes() for a in vp.pixel_lists(P)]
            return out

        before = others()
        _census(vp, reset=True)
        u.uniform(6, 12, P)                                                 # the underlying halves call: the kinds and instances it launches
        uniform = _census(vp, reset=True)
        res, got = t.adaptive(6, 12, P, (0.3,) * N, FLOORS[mode], 4, 4)
        mine = _census(vp, reset=True)
        kind = "render" if mode == BEAUTY else mode
        assert sum(mine[kind].values()) >= 1 and sum(uniform[kind].values()) >= 1
        for k in mine:
            if k not in (kind, "approach"):
                assert sum(mine[k].values()) == 0 and sum(uniform[k].values()) == 0, k      # launches under the underlying mode's kind only (and its walks)
            assert set(mine[k]) == set(uniform[k])                          # the `built` tables are what they are without the call
        assert others() == before
        assert 0 < res["active_left"] < W * H and np.frombuffer(before[0], F32).max() > 0
    finally:
        t.free()
        u.free()
        b.free()
        r.free()


# ------------------------------------------------------------------------------------------------------- 10. state refusals
@pytest.mark.parametrize("mode", [BEAUTY] + PLANE_MODES, ids=["beauty"] + MODE_IDS)
def test_state_refusals_touch_no_buffer_and_leave_the_context_usable(vp, oracle, ctx, mode):
    P = _scene(vp, 0, 1, key=LL.KEY, **LL.param_kw("julia"))
    N = len(AH.PLANES[mode])
    fname = "vp_render_adaptive_halves" if mode == BEAUTY else "vp_render_adaptive_planes_halves"
    frames, bufs = _library_frames(vp, mode, P)
    t = Halves(vp, mode)
    try:
        fill = AH.prefilled(W, H, N, 90)
        t.upload(fill)
        t.adaptive(0, 2, P, (0.3,) * N, FLOORS[mode], 4, 2)                 # the device is in use before the refusals
        t.upload(fill)
        mark = t.download()

        def refused(code, word, first=0, maxf=12):
            res = vp.AdaptiveResult(7, 7, 7, 7)
            if mode == BEAUTY:
                a = vp.Adaptive(0.3, 1e-3, 4, 4)
                rc = vp.lib().vp_render_adaptive_halves(t.acc[0][0].ptr, t.acc[1][0].ptr, t.rec[0][0].ptr, t.rec[1][0].ptr, first, maxf, C.byref(P), C.byref(a), C.byref(res))
            else:
                a = vp.AdaptivePlanes3((C.c_float * 3)(0.3, 0.3, 0.3), (C.c_float * 3)(1e-3, 1e-3, 1e-2), 4, 4)
                b0, b1 = vp.plane_bufs(t.half(0)), vp.plane_bufs(t.half(1))
                rc = vp.lib().vp_render_adaptive_planes_halves(mode, C.byref(b0), C.byref(b1), first, maxf, C.byref(P), C.byref(a), C.byref(res))
            vp.synchronize()
            msg = vp.lib().vp_last_error().decode()
            assert rc == code and word in msg and (fname in msg or code == E_NOOPACITY), (rc, msg)
            assert res.as_dict() == {"samples": 0, "rounds": 0, "active_left": 0, "frames_used": 0}
            assert [x.tobytes() for x in t.download()] == [x.tobytes() for x in mark], word

        vp.enable_counters(True)
        refused(E_STATE, "counters")
        vp.enable_counters(False)
        if mode != BEAUTY:
            vp.set_envmap_sampling(vp.ENV_MIS)
            refused(E_STATE, "passive")
            vp.set_envmap_sampling(vp.ENV_PASSIVE)
            vp.set_arithmetic(vp.ARITH_FAST)
            refused(E_STATE, "exact")
            vp.set_arithmetic(vp.ARITH_EXACT)
            vp.set_tracking(vp.TRACK_SCALAR)
            refused(E_STATE, "spectral")
            vp.set_tracking(vp.TRACK_MULTI_CHANNEL)
            refused(E_STATE, "spectral")
            vp.set_tracking(vp.TRACK_SPECTRAL)
        vp.set_estimator(vp.EST_DECOMP)                                     # no optical-depth table: frames beyond 10 are refused as vp_render_frames refuses them
        refused(E_NOOPACITY, "precompute_opacity", first=0, maxf=12)
        vp.set_estimator(vp.EST_GLOBAL)
        # the context stays usable
        t.reset()
        want = AH.new_halves(W, H, N)
        res_want = AH.render_adaptive_halves(want, frames, 2, 12, (0.3,) * N, FLOORS[mode], 4, 4)
        res, got = t.adaptive(2, 12, P, (0.3,) * N, FLOORS[mode], 4, 4)
        _check(want, res_want, res, got, "after the refusals")
        assert AH.frozen_mask(want).any()
    finally:
        vp.set_envmap_sampling(vp.ENV_PASSIVE)
        vp.set_arithmetic(vp.ARITH_EXACT)
        vp.set_tracking(vp.TRACK_SPECTRAL)
        vp.enable_counters(False)
        t.free()
        for b in bufs:
            b.free()
