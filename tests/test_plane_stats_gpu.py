"""Statistics on planes on the GPU (include/volpath.h vp_render_frames_groups_stats / vp_render_frames_layers_stats).

Every comparison is at tolerance 0, accumulators and records by their bits: against the oracle-built expectation of
tests/plane_stats_lib.py, against the plain plane calls and vp_render_frames_stats of the library itself, or against the numpy
restatements of vp_denoise, vp_relight and vp_composite.  Each test runs in a context of its own."""
import ctypes as C

import numpy as np
import pytest

import adaptive_lib as AL
import denoise_lib as D
import groups_lib as GL
import layers_lib as LL
import plane_stats_lib as PS
import scenes
import subpixel_lib

pytestmark = pytest.mark.gpu

W, H, FRAMES, LONG = PS.W, PS.H, PS.FRAMES, PS.LONG
FIRST, N = FRAMES[0], len(FRAMES)
E_STATE = -2
F32 = np.float32
ZERO = (0.0, 0.0, 0.0)
KINDS = ("groups", "layers")
NAMES = {"groups": ("sun", "sky"), "layers": ("fg", "trans")}


@pytest.fixture
def ctx(vp):
    c = vp.Context(0)
    try:
        with c:
            yield c
    finally:
        c.destroy()


def _scene(vp, oracle, name, est, rng_mode, size=(W, H), env=None, sun_power=scenes.DEFAULT_SUN_POWER, density=None):
    g = LL.grid_of(name, oracle)
    vp.init_volume(g, brick=1, linear=True)
    vp.init_envmap(LL.ENV if env is None else env)
    vp.set_sun(scenes.DEFAULT_SUN_DIR, sun_power)
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
    """the two accumulators and the two record buffers of a _stats call of `kind`"""

    def __init__(self, vp, kind, w=W, h=H):
        self.vp, self.kind = vp, kind
        self.acc = (vp.DeviceBuffer(w, h), vp.DeviceBuffer(w, h))
        self.rec = (vp.StatsBuffer(w, h), vp.StatsBuffer(w, h))
        self._stats = {"groups": vp.render_frames_groups_stats, "layers": vp.render_frames_layers_stats}[kind]
        self._plain = {"groups": vp.render_frames_groups, "layers": vp.render_frames_layers}[kind]

    def render(self, first, n, P):
        """the _stats call; returns (acc0, acc1, rec0, rec1) downloaded"""
        self._stats(self.acc[0].ptr, self.acc[1].ptr, self.rec[0].ptr, self.rec[1].ptr, first, n, P)
        return self.download()

    def plain(self, first, n, P):
        """the plain plane call into the same accumulators"""
        self._plain(self.acc[0].ptr, self.acc[1].ptr, first, n, P)
        return self.acc[0].download(), self.acc[1].download()

    def download(self):
        return self.acc[0].download(), self.acc[1].download(), self.rec[0].download(), self.rec[1].download()

    def reset(self):
        for b in self.acc + self.rec:
            b.reset()

    def free(self):
        for b in self.acc + self.rec:
            b.free()


def _same(kind, got, want, what, flags=None):
    """got: (acc0, acc1, rec0, rec1) downloaded; want: the two Stats of plane_stats_lib"""
    for k in (0, 1):
        assert AL.equal_bits(got[k], want[k].acc), (what, NAMES[kind][k], "accumulator", int((got[k] != want[k].acc).any(-1).sum()))
        bad = PS.same_records(want[k], got[2 + k], None if flags is None else flags)
        assert bad is None, (what, NAMES[kind][k], bad)


def _plain_expectation(oracle, kind, *a, **kw):
    E = (GL if kind == "groups" else LL).expected(oracle, *a, **kw)
    return (E.sun, E.sky) if kind == "groups" else (E.fg, E.trans)


# ------------------------------------------------------------------------------------------------------- against the oracle
CASES = [(k, "soft", e, r) for k in KINDS for e in (0, 1, 2) for r in (0, 2)] + [(k, n, e, 1) for k in KINDS for n in ("julia", "soft16") for e in (0, 1)]


@pytest.mark.parametrize("kind,name,est,rng_mode", CASES, ids=["%s-%s-est%d-rng%d" % c for c in CASES])
def test_planes_and_records_equal_the_oracle_expectation(vp, oracle, ctx, kind, name, est, rng_mode):
    want = PS.expected(oracle, kind, name, est, rng_mode)
    plain = _plain_expectation(oracle, kind, name, est, rng_mode)
    assert want[0].acc.tobytes() == plain[0].tobytes() and want[1].acc.tobytes() == plain[1].tobytes()      # the existing Expectations
    P = _scene(vp, oracle, name, est, rng_mode)
    p = Planes(vp, kind)
    try:
        _same(kind, p.render(FIRST, N, P), want, (kind, name, est, rng_mode, "batched"))          # one staged launch
        p.reset()
        for f in FRAMES:                                                                            # frame by frame: staged too
            single = p.render(f, 1, P)
        _same(kind, single, want, (kind, name, est, rng_mode, "frame by frame"))
    finally:
        p.free()
    # the test means something: both planes carry luminance somewhere, and some record of either plane holds none
    for s in want:
        assert (s.sum_y > 0).any() and (s.n == N).all()
    assert (want[0].sum_y == 0).any()


@pytest.mark.parametrize("kind,name,est", [(k, n, e) for k in KINDS for n, e in (("julia", 1), ("soft", 2))])
def test_accumulators_are_the_plain_calls_by_bytes(vp, oracle, ctx, kind, name, est):
    P = _scene(vp, oracle, name, est, 1)
    p, q = Planes(vp, kind), Planes(vp, kind)
    try:
        got = p.render(FIRST, N, P)
        ref = q.plain(FIRST, N, P)
        assert got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes()
        assert not q.rec[0].download()["n"].any()                                  # the plain call writes no record
        for f in FRAMES:                                                           # a second call continues the first: one frame each
            got = p.render(f + N, 1, P)
            ref = q.plain(f + N, 1, P)
        assert got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes()
        assert (got[2]["n"] == 2 * N).all() and (got[3]["n"] == 2 * N).all() and got[0][..., :3].max() > 0
    finally:
        p.free()
        q.free()


# -------------------------------------------------------------------------------- against the library's own renders of the twins
@pytest.mark.parametrize("name,est", (("julia", 0), ("julia", 1), ("soft", 2)))
def test_group_records_equal_the_stats_renders_of_the_twins(vp, oracle, ctx, name, est):
    """no oracle: 64 x 48, one launch of 70 frames; the sun records are vp_render_frames_stats' with init_envmap(zeros), the sky records
    vp_render_frames_stats' after set_sun(dir, 0) -- the header's equivalent form"""
    size, first, n = (64, 48), LONG[0], len(LONG)
    P = _scene(vp, oracle, name, est, 1, size=size)
    p, b, r = Planes(vp, "groups", *size), vp.DeviceBuffer(*size), vp.StatsBuffer(*size)
    try:
        got = p.render(first, n, P)
        for k, twin in enumerate((dict(env=np.zeros_like(GL.ENV)), dict(sun_power=ZERO))):
            _scene(vp, oracle, name, est, 1, size=size, **twin)
            b.reset()
            r.reset()
            vp.render_frames_stats(b.ptr, r.ptr, first, n, P)
            assert got[k].tobytes() == b.download().tobytes(), NAMES["groups"][k]
            rec = r.download()
            assert got[2 + k].tobytes() == rec.tobytes(), (NAMES["groups"][k], int((got[2 + k] != rec).sum()))
            assert (rec["n"] == n).all() and (rec["sum_y"] > 0).any() and (rec["sum_y2"] > 0).any()
    finally:
        p.free()
        b.free()
        r.free()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("est,density,const", ((0, 61.0, False), (0, 64.0, True), (1, 61.0, False), (2, 61.0, False)))
def test_light_class_as_a_kernel_and_as_constants(vp, oracle, ctx, kind, est, density, const):
    """The light pixel class of the Julia set (tests/test_layers_gpu.py has the reasons for the two densities): at a majorant of 61 the
    light kernel runs -- in a layers launch its samples carry no mark, and the reduce is told their slots --, at 64 the class
    is written as constants, staged once and folded into the records frame by frame all the same."""
    want = PS.expected(oracle, kind, "julia", est, 1, density=density)
    P = _scene(vp, oracle, "julia", est, 1, density=density)
    general, light, miss = vp.pixel_lists(P)
    assert len(light) > 0 and len(miss) > 0 and len(general) > 0
    p = Planes(vp, kind)
    try:
        for first, n in ((FIRST, N), (FIRST, 1)):
            p.reset()
            p.render(first, n, P)
            assert vp.last_light_const() == const
        _same(kind, p.render(FIRST + 1, 1, P), want, (kind, density, "one frame, then the next"))
        p.reset()
        _same(kind, p.render(FIRST, N, P), want, (kind, density, "batched"))
    finally:
        p.free()
    ly, lx = light >> 16, light & 0xffff
    assert not want[0].sum_y[ly, lx].any() and (want[1].sum_y[ly, lx] > 0).all()       # the class sees the sky only: sun and fg stay at 0
    assert (want[0].n[ly, lx] == N).all() and (want[1].n[ly, lx] == N).all()


@pytest.mark.parametrize("name,est", (("julia", 0), ("julia", 1), ("soft", 1)))
def test_a_launch_of_70_frames_and_its_split_into_two_calls(vp, oracle, monkeypatch, name, est):
    """one launch of 64 frames or more: the approach walks hand their samples over (VP_DENSE_PERCENT=101: never too dense to walk), the
    constants of the launch are staged once; a call of 2 frames followed by a call of 68 leaves the bits of one call of 70"""
    monkeypatch.setenv("VP_DENSE_PERCENT", "101")
    c = vp.Context(0)
    monkeypatch.delenv("VP_DENSE_PERCENT")
    try:
        with c:
            P = _scene(vp, oracle, name, est, 1)
            for kind in KINDS:
                want = PS.expected(oracle, kind, name, est, 1, frames=LONG)
                p = Planes(vp, kind)
                try:
                    got = p.render(LONG[0], len(LONG), P)
                    if name == "julia":
                        assert vp.last_approach_mode() != 0, "the approach walk did not run"
                    _same(kind, got, want, (kind, name, est, "70 frames"))
                    p.reset()
                    p.render(LONG[0], 2, P)
                    _same(kind, p.render(LONG[0] + 2, len(LONG) - 2, P), want, (kind, name, est, "2 + 68 frames"))
                finally:
                    p.free()
    finally:
        c.destroy()


@pytest.mark.parametrize("kind", KINDS)
def test_a_staging_cap_that_splits_the_call_into_launches(vp, oracle, monkeypatch, kind):
    """VP_STAGE_MB=1 in a context of its own (the knob is read when a context first touches its device): 160 x 120 pixels are 300 KiB of
    staging per frame and plane, so a call of 8 frames is three launches (layers) or eight (groups, two planes) -- and leaves the bits
    of the one launch of an uncapped context, records read and written once per launch"""
    size, n = (160, 120), 8
    out = []
    for cap in (None, "1"):
        if cap:
            monkeypatch.setenv("VP_STAGE_MB", cap)
        c = vp.Context(0)
        monkeypatch.delenv("VP_STAGE_MB", raising=False)
        try:
            with c:
                P = _scene(vp, oracle, "julia", 1, 1, size=size)
                p = Planes(vp, kind, *size)
                try:
                    vp.synchronize()
                    vp.render_time_ms(reset=True)
                    got = p.render(FIRST, n, P)
                    out.append((vp.render_time_ms(reset=True)[1], [a.tobytes() for a in got]))
                    assert (got[2]["n"] == n).all() and (got[3]["n"] == n).all() and (got[3]["sum_y"] > 0).any()
                finally:
                    p.free()
        finally:
            c.destroy()
    assert out[0][0] == 1 and out[1][0] == (8 if kind == "groups" else 3), (out[0][0], out[1][0])
    assert out[0][1] == out[1][1]


@pytest.mark.parametrize("kind", KINDS)
def test_three_shards_touch_their_own_records_and_make_up_the_whole(vp, oracle, ctx, kind):
    want = PS.expected(oracle, kind, "soft", 0, 1)
    P = _scene(vp, oracle, "soft", 0, 1)
    sentinel = np.zeros((H, W), vp.PIXEL_STATS_DTYPE)
    sentinel["sum_y"], sentinel["sum_y2"], sentinel["n"], sentinel["flags"] = -7.25, 1e300, 0xabcd0123, 0xfffffff0
    whole = [np.zeros((H, W), vp.PIXEL_STATS_DTYPE) for _ in (0, 1)]
    seen = np.zeros((H, W), int)
    p = Planes(vp, kind)
    try:
        for r in range(3):
            vp.set_shard(r, 3)
            owned = AL.owned_pixels(vp, W, H, r, 3)
            p.reset()
            for b in p.rec:
                b.upload(sentinel)
            got = p.render(FIRST, N, P)
            for k in (0, 1):
                assert got[2 + k][~owned].tobytes() == sentinel[~owned].tobytes(), (r, NAMES[kind][k])     # unowned records: untouched
                assert not got[k][~owned].any()
                p.rec[k].reset()                                                                          # ... the owned ones from zero
            p.acc[0].reset()
            p.acc[1].reset()
            got = p.render(FIRST, N, P)
            for k in (0, 1):
                assert not np.frombuffer(got[2 + k][~owned].tobytes(), np.uint8).any()
                whole[k][owned] = got[2 + k][owned]
            seen += owned
        assert (seen == 1).all()
        for k in (0, 1):
            assert PS.same_records(want[k], whole[k]) is None, (NAMES[kind][k], PS.same_records(want[k], whole[k]))
    finally:
        vp.set_shard(0, 1)
        p.free()


@pytest.mark.parametrize("kind", KINDS)
def test_flags_are_neither_read_nor_written(vp, oracle, ctx, kind):
    want = PS.expected(oracle, kind, "julia", 1, 1)
    P = _scene(vp, oracle, "julia", 1, 1)
    board = np.zeros((H, W), vp.PIXEL_STATS_DTYPE)
    board["flags"] = (np.add.outer(np.arange(H), np.arange(W)) % 2).astype(np.uint32) * AL.FROZEN
    p = Planes(vp, kind)
    try:
        for b in p.rec:
            b.upload(board)
        _same(kind, p.render(FIRST, N, P), want, (kind, "frozen checkerboard"), flags=board["flags"])     # sampled like the others
        assert board["flags"].sum() == W * H // 2
    finally:
        p.free()


@pytest.mark.parametrize("kind,name,est", (("layers", "julia", 1), ("groups", "soft", 0)))
def test_subpixel_factor_2_folds_the_gathered_fine_samples(vp, oracle, ctx, kind, name, est):
    """vp_set_subpixel(2) at 16 x 12: the records are the fold of the library's own S = 1 plane samples at 32 x 24, one frame at a time,
    gathered by vp_subpixel_offset"""
    P = _scene(vp, oracle, name, est, 1)
    fineP = subpixel_lib.fine_of(P, 2)
    fine, p = Planes(vp, kind, 2 * W, 2 * H), Planes(vp, kind)
    try:
        fine_pair = PS.library_frames(lambda f: fine.plain(f, 1, fineP), fine.acc)
        want = PS.fold(lambda f: tuple(subpixel_lib.gather(vp, img, W, H, f, 2) for img in fine_pair(f)), W, H, FIRST, N)
        vp.set_subpixel(2)
        _same(kind, p.render(FIRST, N, P), want, (kind, name, est, "S = 2"))
        assert (want[0].sum_y > 0).any() and (want[1].sum_y > 0).any() and (want[0].sum_y == 0).any()
    finally:
        vp.set_subpixel(1)
        fine.free()
        p.free()


@pytest.mark.parametrize("kind,name,est", (("groups", "julia", 1), ("layers", "soft", 2)))
def test_the_call_leaves_nothing_behind(vp, oracle, ctx, kind, name, est):
    P = _scene(vp, oracle, name, est, 1)
    p, q, b, r = Planes(vp, kind), Planes(vp, kind), vp.DeviceBuffer(W, H), vp.StatsBuffer(W, H)
    try:
        def others():
            out = []
            b.reset()
            vp.render_frames(b.ptr, FIRST, N, P)
            out.append(b.download().tobytes())
            b.reset()
            r.reset()
            vp.render_frames_stats(b.ptr, r.ptr, FIRST, N, P)
            out += [b.download().tobytes(), r.download().tobytes()]
            q.reset()
            out += [a.tobytes() for a in q.plain(FIRST, N, P)]
            return out

        before = others()
        p.render(FIRST, N, P)
        assert others() == before
        p.render(FIRST + N, 1, P)                       # ... after a one-frame call too
        assert others() == before
        assert before[0] == before[1] and np.frombuffer(before[0], F32).max() > 0
    finally:
        p.free()
        q.free()
        b.free()
        r.free()


@pytest.mark.parametrize("kind", KINDS)
def test_refusals_return_state_errors_and_touch_no_buffer(vp, oracle, ctx, kind):
    want = PS.expected(oracle, kind, "soft", 0, 1)
    P = _scene(vp, oracle, "soft", 0, 1)
    p = Planes(vp, kind)
    f = getattr(vp.lib(), "vp_render_frames_%s_stats" % kind)
    try:
        mark = np.full((H, W, 4), 7.25, F32)
        rmark = np.zeros((H, W), vp.PIXEL_STATS_DTYPE)
        rmark["sum_y"], rmark["sum_y2"], rmark["n"], rmark["flags"] = 3.5, 12.25, 5, 0x10
        for b in p.acc:
            b.upload(mark)
        for b in p.rec:
            b.upload(rmark)

        def refused(word):
            rc = f(p.acc[0].ptr, p.acc[1].ptr, p.rec[0].ptr, p.rec[1].ptr, FIRST, N, C.byref(P))
            vp.synchronize()
            msg = vp.lib().vp_last_error().decode()
            assert rc == E_STATE and word in msg and "vp_render_frames_%s_stats" % kind in msg, (rc, msg)
            got = p.download()
            assert got[0].tobytes() == mark.tobytes() == got[1].tobytes() and got[2].tobytes() == rmark.tobytes() == got[3].tobytes()

        vp.set_envmap_sampling(vp.ENV_MIS)
        refused("passive")
        vp.set_envmap_sampling(vp.ENV_PASSIVE)
        vp.set_arithmetic(vp.ARITH_FAST)                # the plane instances are the exact unit's
        refused("exact")
        vp.set_arithmetic(vp.ARITH_EXACT)
        p.reset()
        _same(kind, p.render(FIRST, N, P), want, (kind, "after the refusals"))      # the context stays usable
    finally:
        vp.set_envmap_sampling(vp.ENV_PASSIVE)
        vp.set_arithmetic(vp.ARITH_EXACT)
        p.free()


# ------------------------------------------------------------------------------------------------------------- the pipeline
@pytest.mark.parametrize("kind", KINDS)
def test_stats_then_denoise_per_plane_then_the_output_stage(vp, oracle, ctx, kind):
    """what the calls exist for: the _stats call, vp_denoise per plane with the plane's own records as guide, then vp_relight /
    vp_composite of the two MEAN images with scale 1 -- against denoise_lib.denoise on the downloaded planes and the numpy restatement
    of the output stage; radius 2, patch 1, both forms of the filter"""
    R, F, k = 2, 1, 0.45
    rgb = (0.7, 0.1, 9.0)
    P = _scene(vp, oracle, "soft", 1, 1)
    p, mean, dst = Planes(vp, kind), (vp.DeviceBuffer(W, H), vp.DeviceBuffer(W, H)), vp.DeviceBuffer(W, H)
    try:
        got = p.render(LONG[0], 8, P)
        want_mean = [D.denoise(got[j], got[2 + j], R, F, k) for j in (0, 1)]
        want = GL.relight(want_mean[0], want_mean[1], 1.0) if kind == "groups" else LL.composite(want_mean[0], want_mean[1], 1.0, rgb=rgb)
        for form in (0, 1):
            vp.set_denoise_form(form)
            for j in (0, 1):
                mean[j].reset()
                vp.denoise(mean[j].ptr, p.acc[j].ptr, p.rec[j].ptr, W, H, R, F, k)
                assert mean[j].download().tobytes() == want_mean[j].tobytes(), (form, NAMES[kind][j])
            if kind == "groups":
                vp.relight(dst.ptr, mean[0].ptr, mean[1].ptr, W * H, 1.0)
            else:
                vp.composite(dst.ptr, mean[0].ptr, mean[1].ptr, W * H, 1.0, plate_rgb=rgb)
            assert dst.download().tobytes() == want.tobytes(), form
            assert vp.last_denoise_form() == form
        # the filter had something to do in either plane, and left w alone: coverage / heat are the unfiltered means
        for j in (0, 1):
            raw = D.mean_image(got[j], got[2 + j]["n"])[0]
            assert not np.array_equal(want_mean[j][..., :3], raw), NAMES[kind][j]
            assert np.array_equal(want_mean[j][..., 3], got[j][..., 3] * (F32(1.0) / F32(8)))
    finally:
        vp.set_denoise_form(0)
        for b in mean + (dst,):
            b.free()
        p.free()
