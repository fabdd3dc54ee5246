"""Half-buffer renders and the cross-filtered output stage on the GPU (include/volpath.h vp_render_frames_halves_stats, vp_merge_halves,
vp_accumulate_stats).

Every comparison is byte for byte.  The render is held to its definition: the sequence of one-frame vp_render_frames_stats calls, each
into the half its frame belongs to, made by the library itself in the same context state.  The output stage is held to the numpy
restatement of tests/halves_lib.py.  Each test runs in a context of its own."""
import ctypes as C
import os

import numpy as np
import pytest

import adaptive_lib as A
import denoise_guided_lib as G
import denoise_lib as D
import halves_lib as HL
import layers_lib as LL
import scenes

pytestmark = pytest.mark.gpu

W, H = LL.W, LL.H
SHORT, LONG = (9, 8), (10, 70)      # odd start across the frame-11 switch; one long launch with approach walks and constant rows
F32 = np.float32


@pytest.fixture
def ctx(vp):
    c = vp.Context(0)
    try:
        with c:
            yield c
    finally:
        c.destroy()


def _scene(vp, oracle, name, est, rng_mode, size=(W, H), key=LL.KEY, **param):
    vp.init_volume(LL.grid_of(name, oracle), brick=1, linear=True)
    vp.init_envmap(LL.ENV)
    vp.set_sun(scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER)
    vp.set_camera()
    vp.set_estimator(est)
    vp.set_rng(rng_mode, key)
    vp.set_shard(0, 1)
    if est == 1:
        vp.precompute_opacity(scenes.DEFAULT_SUN_DIR)
    return vp.make_param(size[0], size[1], **(param or LL.param_kw(name)))


class Halves:
    """the two accumulators and the two record buffers of a halves call"""

    def __init__(self, vp, w=W, h=H, fill=None):
        self.vp = vp
        self.acc = (vp.DeviceBuffer(w, h), vp.DeviceBuffer(w, h))
        self.rec = (vp.StatsBuffer(w, h), vp.StatsBuffer(w, h))
        if fill is not None:
            self.upload(fill)

    def upload(self, fill):
        """fill: (acc0, acc1, rec0, rec1)"""
        for b, a in zip(self.acc + self.rec, fill):
            b.upload(a)

    def render(self, first, n, P):
        self.vp.render_frames_halves_stats(self.acc[0].ptr, self.acc[1].ptr, self.rec[0].ptr, self.rec[1].ptr, first, n, P)
        return self.download()

    def by_definition(self, first, n, P, S=1, runs=False):
        """one vp_render_frames_stats call per frame (runs: per maximal run of frames of one half), ascending, each into its half"""
        calls = [(f, 1) for f in range(first, first + n)] if not runs else sorted(HL.runs_of_half(first, n, 0, S) + HL.runs_of_half(first, n, 1, S))
        for f, k in calls:
            h = HL.half_of_frame(f, S)
            assert all(HL.half_of_frame(g, S) == h for g in range(f, f + k))
            self.vp.render_frames_stats(self.acc[h].ptr, self.rec[h].ptr, f, k, P)
        return self.download()

    def download(self):
        return tuple(b.download() for b in self.acc + self.rec)

    def free(self):
        for b in self.acc + self.rec:
            b.free()


NAMES = ("h0 accumulator", "h1 accumulator", "h0 records", "h1 records")


def _same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.tobytes() == w.tobytes(), (what, name, int((g.view(np.uint8).reshape(g.shape[0], g.shape[1], -1) != w.view(np.uint8).reshape(g.shape[0], g.shape[1], -1)).any(-1).sum()))


def _compare(vp, P, first, n, what, fill=None, S=1, runs=False, w=W, h=H):
    a, b = Halves(vp, w, h, fill), Halves(vp, w, h, fill)
    try:
        got = a.render(first, n, P)
        want = b.by_definition(first, n, P, S, runs)
        _same(got, want, what)
        return got
    finally:
        a.free(); b.free()


def _classes_present(vp, P):
    g, l, m = vp.pixel_lists(P)
    assert len(g) >= 1 and len(l) >= 1 and len(m) >= 1, (len(g), len(l), len(m))


# ------------------------------------------------------------------------------------------------------- 1. the definition
@pytest.mark.parametrize("rng_mode", [0, 2], ids=["samplerh", "philox7"])
@pytest.mark.parametrize("est", [0, 1, 2], ids=["global", "decomp", "bounded"])
def test_halves_are_the_one_frame_calls_of_their_frames(vp, oracle, ctx, est, rng_mode):
    P = _scene(vp, oracle, "julia", est, rng_mode)
    _classes_present(vp, P)
    for first, n in (SHORT, LONG):
        got = _compare(vp, P, first, n, (est, rng_mode, first, n))
        n0, n1 = len(HL.frames_of_half(first, n, 0)), len(HL.frames_of_half(first, n, 1))
        assert (got[2]["n"] == n0).all() and (got[3]["n"] == n1).all() and n0 + n1 == n
        assert (got[0] != got[1]).any()                                  # the two halves differ somewhere
        assert not got[2]["flags"].any() and not got[3]["flags"].any()


# ------------------------------------------------------------------------------------------------------- 2. modes that plane calls refuse
@pytest.mark.parametrize("mode", ["fast", "mis", "scalar", "f16"])
def test_modes_that_plane_calls_refuse(vp, oracle, ctx, mode):
    name = "soft16" if mode == "f16" else "julia"
    rng_mode = {"fast": 1, "mis": 0, "scalar": 1, "f16": 2}[mode]
    P = _scene(vp, oracle, name, 1, rng_mode)
    if mode == "fast":
        vp.set_arithmetic(vp.ARITH_FAST)
    if mode == "mis":
        vp.set_envmap_sampling(vp.ENV_MIS)
    if mode == "scalar":
        vp.set_tracking(vp.TRACK_SCALAR)
    if mode == "f16":
        assert vp.volume_info()["format"] == vp.VOL_F16
    # a plane call refuses this state (the binary16 volume aside, which plane calls take)
    if mode != "f16":
        t = Halves(vp)
        try:
            with pytest.raises(vp.VolpathError):
                vp.render_frames_layers_stats(t.acc[0].ptr, t.acc[1].ptr, t.rec[0].ptr, t.rec[1].ptr, SHORT[0], SHORT[1], P)
        finally:
            t.free()
    got = _compare(vp, P, SHORT[0], SHORT[1], mode)
    assert got[0][..., :3].max() > 0 and got[1][..., :3].max() > 0
    if mode == "fast":
        assert vp.last_arithmetic() == vp.ARITH_FAST


# ------------------------------------------------------------------------------------------------------- 3. untouched and continued buffers
def _fill(seed, w=W, h=H):
    a0, r0 = HL.prefill(w, h, seed)
    a1, r1 = HL.prefill(w, h, seed + 1)
    return a0, a1, r0, r1


def test_one_frame_leaves_the_other_half_alone_and_calls_continue(vp, oracle, ctx):
    P = _scene(vp, oracle, "julia", 0, 1)
    _classes_present(vp, P)
    fill = _fill(40)
    assert any(np.signbit(a[a == 0]).any() for a in fill[:2]) and fill[2]["n"].any() and fill[3]["flags"].any()
    for f, other in ((10, 1), (11, 0)):
        got = _compare(vp, P, f, 1, ("one frame", f), fill=fill)
        assert got[other].tobytes() == fill[other].tobytes() and got[2 + other].tobytes() == fill[2 + other].tobytes()
        mine = 1 - other
        assert got[mine].tobytes() != fill[mine].tobytes() and (got[2 + mine]["n"] == fill[2 + mine]["n"] + 1).all()
        assert np.array_equal(got[2 + mine]["flags"], fill[2 + mine]["flags"])
    a, b = Halves(vp, fill=fill), Halves(vp, fill=fill)
    try:
        a.render(9, 3, P)
        split = a.render(12, 5, P)
        whole = b.render(9, 8, P)
        _same(split, whole, "3 + 5 frames against 8")
    finally:
        a.free(); b.free()


# ------------------------------------------------------------------------------------------------------- 4. a sub-pixel factor
def test_subpixel_halves_alternate_in_blocks_of_s_squared(vp, oracle, ctx):
    P = _scene(vp, oracle, "julia", 0, 2)
    vp.set_subpixel(2)
    first, n = 6, 11
    got = _compare(vp, P, first, n, "S = 2, per run", S=2, runs=True)
    n0, n1 = len(HL.frames_of_half(first, n, 0, 2)), len(HL.frames_of_half(first, n, 1, 2))
    assert (n0, n1) == (5, 6) and (got[2]["n"] == n0).all() and (got[3]["n"] == n1).all()
    _compare(vp, P, first, n, "S = 2, per frame", S=2)


# ------------------------------------------------------------------------------------------------------- 5. a shard
def test_a_shard_touches_only_its_pixels(vp, oracle, ctx):
    P = _scene(vp, oracle, "julia", 1, 2)
    whole = _compare(vp, P, SHORT[0], SHORT[1], "unsharded")
    fill = _fill(50)
    vp.set_shard(1, 3)
    try:
        got = _compare(vp, P, SHORT[0], SHORT[1], "rank 1 of 3", fill=fill)
    finally:
        vp.set_shard(0, 1)
    mine = A.owned_pixels(vp, W, H, 1, 3)
    assert mine.any() and (~mine).any()
    for k in range(4):
        assert got[k][~mine].tobytes() == fill[k][~mine].tobytes(), NAMES[k]
    # the owned pixels gained their own frames' samples: the counts, and the unsharded call's samples on top of the prefill
    for k in (0, 1):
        assert (got[2 + k]["n"][mine] == fill[2 + k]["n"][mine] + whole[2 + k]["n"][mine]).all()
        assert (got[k][mine] != fill[k][mine]).any()
    # ... and from zeroed buffers they are the unsharded call's bytes
    zero = (np.zeros((H, W, 4), F32),) * 2 + (np.zeros((H, W), vp.PIXEL_STATS_DTYPE),) * 2
    vp.set_shard(1, 3)
    try:
        t = Halves(vp, fill=zero)
        try:
            z = t.render(SHORT[0], SHORT[1], P)
        finally:
            t.free()
    finally:
        vp.set_shard(0, 1)
    for k in range(4):
        assert z[k][mine].tobytes() == whole[k][mine].tobytes() and not z[k][~mine].view(np.uint8).any(), NAMES[k]


# ------------------------------------------------------------------------------------------------------- 6. the staging cap
def test_a_staging_cap_that_splits_the_job_into_launches(vp, oracle):
    """VP_STAGE_MB=1 in a context of its own (the knob is read when a context first touches its device): 160 x 120 pixels are 300 KiB
    of staging per frame, so nine frames from frame 3 go in launches of three -- which begin on the absolute frames 3, 6 and 9"""
    old = os.environ.get("VP_STAGE_MB")
    os.environ["VP_STAGE_MB"] = "1"
    try:
        c = vp.Context(0)
    finally:
        if old is None:
            del os.environ["VP_STAGE_MB"]
        else:
            os.environ["VP_STAGE_MB"] = old
    try:
        with c:
            P = _scene(vp, oracle, "julia", 0, 1, size=(160, 120), key=(1, 2), density=800.0)
            t, d = Halves(vp, 160, 120), Halves(vp, 160, 120)
            try:
                vp.render_time_ms(reset=True)
                got = t.render(3, 9, P)
                launches = vp.render_time_ms(reset=True)[1]
                want = d.by_definition(3, 9, P)
            finally:
                t.free(); d.free()
    finally:
        c.destroy()
    assert launches >= 3, launches
    _same(got, want, "capped staging")
    assert (got[2]["n"] == 4).all() and (got[3]["n"] == 5).all()


# ------------------------------------------------------------------------------------------------------- 7. the output stage
class FloatBuffer:
    def __init__(self, vp, n):
        self.vp, self.n = vp, n
        self.ptr = vp.lib().vp_malloc(max(n, 1) * 4)
        assert self.ptr

    def upload(self, arr):
        arr = np.ascontiguousarray(arr, F32)
        assert arr.size == self.n
        assert self.vp.lib().vp_upload(self.ptr, arr.ctypes.data_as(C.c_void_p), arr.nbytes) == 0

    def download(self, shape):
        out = np.empty(shape, F32)
        assert self.vp.lib().vp_download(out.ctypes.data_as(C.c_void_p), self.ptr, out.nbytes) == 0
        return out

    def free(self):
        self.vp.lib().vp_free(self.ptr)


def test_merge_and_accumulate_stats_equal_the_restatement(vp, ctx):
    Wm, Hm = 23, 13
    a, ra = D.synthetic(Wm, Hm, 5)
    b, rb = D.synthetic(Wm, Hm, 6)
    ma, mb = A.scale_by_count(a, ra["n"], 1.0), A.scale_by_count(b, rb["n"], 1.0)
    assert ((ra["n"] == 0) & (rb["n"] > 0)).any() and ((ra["n"] > 0) & (rb["n"] == 0)).any() and ((ra["n"] > 0) & (rb["n"] > 0) & (ra["n"] != rb["n"])).any()
    assert np.isfinite(ma).all() and np.isfinite(mb).all()
    n = Wm * Hm
    da, db, dd = (vp.DeviceBuffer(Wm, Hm) for _ in range(3))
    sa, sb = vp.StatsBuffer(Wm, Hm), vp.StatsBuffer(Wm, Hm)
    res = FloatBuffer(vp, n)
    try:
        da.upload(ma); db.upload(mb); sa.upload(ra); sb.upload(rb)
        for floor_y in (1e-3, 0.5):
            want, want_resid = HL.merge_halves(ma, ra, mb, rb, floor_y)
            poison = np.full((Hm, Wm), 7.0, F32)
            res.upload(poison)
            dd.upload(np.full((Hm, Wm, 4), 7.0, F32))
            vp.merge_halves(dd.ptr, res.ptr, da.ptr, sa.ptr, db.ptr, sb.ptr, n, floor_y)
            assert dd.download().tobytes() == want.tobytes() and res.download((Hm, Wm)).tobytes() == want_resid.tobytes(), floor_y
        want, want_resid = HL.merge_halves(ma, ra, mb, rb, 1e-3)
        # size 0: nothing is written
        vp.merge_halves(dd.ptr, res.ptr, da.ptr, sa.ptr, db.ptr, sb.ptr, 0, 0.5)
        assert dd.download().tobytes() == want.tobytes() and res.download((Hm, Wm)).tobytes() == HL.merge_halves(ma, ra, mb, rb, 0.5)[1].tobytes()
        # no residual map: dst alone (and no floor is asked for)
        dd.upload(np.full((Hm, Wm, 4), 7.0, F32))
        vp.merge_halves(dd.ptr, None, da.ptr, sa.ptr, db.ptr, sb.ptr, n, float("nan"))
        assert dd.download().tobytes() == want.tobytes()
        # in place: dst == a, then dst == b
        vp.merge_halves(da.ptr, res.ptr, da.ptr, sa.ptr, db.ptr, sb.ptr, n, 1e-3)
        assert da.download().tobytes() == want.tobytes() and res.download((Hm, Wm)).tobytes() == want_resid.tobytes()
        da.upload(ma)
        vp.merge_halves(db.ptr, res.ptr, da.ptr, sa.ptr, db.ptr, sb.ptr, n, 1e-3)
        assert db.download().tobytes() == want.tobytes() and res.download((Hm, Wm)).tobytes() == want_resid.tobytes()
        # the records add; with vp_accumulate the pair of all frames
        vp.accumulate_stats(sa.ptr, sb.ptr, n)
        assert sa.download().tobytes() == HL.accumulate_stats(ra, rb).tobytes() and sb.download().tobytes() == rb.tobytes()
        vp.accumulate_stats(sa.ptr, sb.ptr, 0)
        assert sa.download().tobytes() == HL.accumulate_stats(ra, rb).tobytes()
    finally:
        for x in (da, db, dd, sa, sb, res):
            x.free()


# ------------------------------------------------------------------------------------------------------- 8. the pipeline
def test_the_cross_filter_pipeline_equals_the_restatement(vp, oracle, ctx):
    Wp, Hp, R, Fp, k = 32, 24, 3, 1, 0.45
    P = _scene(vp, oracle, "julia", 0, 2, size=(Wp, Hp))
    t = Halves(vp, Wp, Hp)
    ta, tb, dst, fa_buf = (vp.DeviceBuffer(Wp, Hp) for _ in range(4))
    res = FloatBuffer(vp, Wp * Hp)
    alpha, _ = G.synthetic_features(Wp, Hp, 3)
    try:
        h0, h1, r0, r1 = t.render(0, 16, P)
        assert (r0["n"] == 8).all() and (r1["n"] == 8).all()
        want, want_resid, wa, wb = HL.denoise_cross(h0, r0, h1, r1, R, Fp, k)
        assert (D.variance(r0) != 0).sum() > 20 and want_resid.max() > 0
        assert wa.tobytes() != D.denoise(h0, r0, R, Fp, k).tobytes()            # the guide matters on this render
        try:
            for form in (0, 1):
                vp.set_denoise_form(form)
                vp.denoise_guided(ta.ptr, t.acc[0].ptr, t.rec[0].ptr, Wp, Hp, (), R, Fp, k, guide_ptr=t.acc[1].ptr, guide_stats_ptr=t.rec[1].ptr)
                vp.denoise_guided(tb.ptr, t.acc[1].ptr, t.rec[1].ptr, Wp, Hp, (), R, Fp, k, guide_ptr=t.acc[0].ptr, guide_stats_ptr=t.rec[0].ptr)
                vp.merge_halves(dst.ptr, res.ptr, ta.ptr, t.rec[0].ptr, tb.ptr, t.rec[1].ptr, Wp * Hp, 1e-3)
                assert ta.download().tobytes() == wa.tobytes() and tb.download().tobytes() == wb.tobytes(), form
                assert dst.download().tobytes() == want.tobytes() and res.download((Hp, Wp)).tobytes() == want_resid.tobytes(), form
                # the helper: the same three calls
                for b in (ta, tb, dst):
                    b.reset()
                res.upload(np.zeros((Hp, Wp), F32))
                vp.denoise_cross(dst.ptr, res.ptr, t.acc[0].ptr, t.rec[0].ptr, t.acc[1].ptr, t.rec[1].ptr, ta.ptr, tb.ptr, Wp, Hp, R, Fp, k)
                assert dst.download().tobytes() == want.tobytes() and res.download((Hp, Wp)).tobytes() == want_resid.tobytes(), form
            # ... and with a feature plane
            fa_buf.upload(alpha)
            fwant, fresid, _, _ = HL.denoise_cross(h0, r0, h1, r1, R, Fp, k, features=[(alpha, 1, 0.1)])
            assert fwant.tobytes() != want.tobytes()
            vp.denoise_cross(dst.ptr, res.ptr, t.acc[0].ptr, t.rec[0].ptr, t.acc[1].ptr, t.rec[1].ptr, ta.ptr, tb.ptr, Wp, Hp, R, Fp, k, features=[(fa_buf.ptr, 1, 0.1)])
            assert dst.download().tobytes() == fwant.tobytes() and res.download((Hp, Wp)).tobytes() == fresid.tobytes()
        finally:
            vp.set_denoise_form(0)
        # the halves did not change under the filters
        _same(t.download(), (h0, h1, r0, r1), "after the output stage")
    finally:
        t.free(); res.free()
        for b in (ta, tb, dst, fa_buf):
            b.free()


# ------------------------------------------------------------------------------------------------------- 9. nothing left behind
def test_the_call_leaves_nothing_behind(vp, oracle, ctx):
    P = _scene(vp, oracle, "julia", 1, 2)
    buf, t = vp.DeviceBuffer(W, H), Halves(vp)
    try:
        vp.render_frames(buf.ptr, 8, 6, P)
        before = buf.download()
        assert vp.last_pipelined() == 1
        for kind in (vp.CENSUS_RENDER, vp.CENSUS_LAYERS):
            vp.launch_census(vp.CENSUS_EXACT, kind, reset=True)
        vp.groups_census(reset=True); vp.group_layers_census(reset=True)
        t.render(SHORT[0], SHORT[1], P)
        assert vp.last_pipelined() == 0
        assert sum(vp.launch_census(vp.CENSUS_EXACT, vp.CENSUS_RENDER).values()) >= 1
        assert sum(vp.launch_census(vp.CENSUS_EXACT, vp.CENSUS_LAYERS).values()) == 0
        assert sum(vp.groups_census().values()) == 0 and sum(vp.group_layers_census().values()) == 0
        L = vp.lib()
        assert L.vp_test_launch_census(0, 0, None, None, 0, 0) == L.vp_test_launch_census(0, 1, None, None, 0, 0) == 10368
        assert L.vp_test_groups_census(None, None, 0, 0) == L.vp_test_group_layers_census(None, None, 0, 0) == 10368
        buf.reset()
        vp.render_frames(buf.ptr, 8, 6, P)
        assert buf.download().tobytes() == before.tobytes() and vp.last_pipelined() == 1
        buf.reset()
        vp.render_frames(buf.ptr, 8, 1, P)                     # the direct one-frame accumulation too
        one = buf.download()
        t.render(8, 1, P)
        buf.reset()
        vp.render_frames(buf.ptr, 8, 1, P)
        assert buf.download().tobytes() == one.tobytes()
    finally:
        buf.free(); t.free()
