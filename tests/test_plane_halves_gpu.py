"""Half-buffer renders of plane calls and their output stage on the GPU (include/volpath.h vp_render_frames_planes_halves_stats; DESIGN.md
section 2.19).

Every comparison is byte for byte over all 2N accumulators and 2N record buffers.  The render is held to its definition: the sequence
of the mode's one-frame _stats calls, each into the planes of the half its frame belongs to, made by the library itself in the same
context state.  The output stage is held to the explicit sequence of library calls and to the numpy restatements of tests/halves_lib.py,
tests/denoise_lib.py and tests/variance_lib.py.  Each test runs in a context of its own."""
import ctypes as C
import os

import numpy as np
import pytest

import adaptive_lib as A
import denoise_lib as D
import halves_lib as HL
import layers_lib as LL
import scenes
import variance_lib as VL

pytestmark = pytest.mark.gpu

W, H = LL.W, LL.H
SHORT, LONG = (9, 8), (10, 70)      # odd start across the frame-11 switch; one long launch with approach walks and constant rows
F32 = np.float32
E_STATE = -2
LAYERS, GROUPS, GROUP_LAYERS = 1, 2, 3
MODES = [LAYERS, GROUPS, GROUP_LAYERS]
MODE_IDS = ["layers", "groups", "group_layers"]
PLANES = {LAYERS: ("fg", "trans"), GROUPS: ("sun", "sky"), GROUP_LAYERS: ("sun", "sky", "trans")}


@pytest.fixture
def ctx(vp):
    c = vp.Context(0)
    try:
        with c:
            yield c
    finally:
        c.destroy()


def _scene(vp, oracle, est, rng_mode, size=(W, H), key=LL.KEY, **param):
    vp.init_volume(LL.grid_of("julia", oracle), brick=1, linear=True)
    vp.init_envmap(LL.ENV)
    vp.set_sun(scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER)
    vp.set_camera()
    vp.set_estimator(est)
    vp.set_rng(rng_mode, key)
    vp.set_shard(0, 1)
    if est == 1:
        vp.precompute_opacity(scenes.DEFAULT_SUN_DIR)
    return vp.make_param(size[0], size[1], **(param or LL.param_kw("julia")))


def _stats_call(vp, mode):
    return {LAYERS: vp.render_frames_layers_stats, GROUPS: vp.render_frames_groups_stats, GROUP_LAYERS: vp.render_frames_group_layers_stats}[mode]


def _classes_present(vp, P):
    """the view holds all three pixel classes: the light class's slots reach the layers split through `unmarked`"""
    g, l, m = vp.pixel_lists(P)
    assert len(g) >= 1 and len(l) >= 1 and len(m) >= 1, (len(g), len(l), len(m))


class PlaneHalves:
    """the 2N accumulators and 2N record buffers of a planes-halves call; downloads come in the order of names():
    h0's accumulators, h1's accumulators, h0's records, h1's records, each in the mode's plane order"""

    def __init__(self, vp, mode, w=W, h=H, fill=None):
        self.vp, self.mode, self.n = vp, mode, len(PLANES[mode])
        self.acc = [[vp.DeviceBuffer(w, h) for _ in range(self.n)] for _ in (0, 1)]
        self.rec = [[vp.StatsBuffer(w, h) for _ in range(self.n)] for _ in (0, 1)]
        if fill is not None:
            self.upload(fill)

    def all(self):
        return self.acc[0] + self.acc[1] + self.rec[0] + self.rec[1]

    def names(self):
        return ["h%d %s %s" % (h, p, kind) for kind in ("accumulator", "records") for h in (0, 1) for p in PLANES[self.mode]]

    def upload(self, fill):
        for b, a in zip(self.all(), fill):
            b.upload(a)

    def half(self, h):
        return [(a.ptr, r.ptr) for a, r in zip(self.acc[h], self.rec[h])]

    def render(self, first, n, P):
        self.vp.render_frames_planes_halves_stats(self.mode, self.half(0), self.half(1), first, n, P)
        return self.download()

    def by_definition(self, first, n, P, S=1, runs=False):
        """the mode's _stats call once per frame (runs: per maximal run of frames of one half), ascending, each into the planes of its half"""
        calls = [(f, 1) for f in range(first, first + n)] if not runs else sorted(HL.runs_of_half(first, n, 0, S) + HL.runs_of_half(first, n, 1, S))
        call = _stats_call(self.vp, self.mode)
        for f, k in calls:
            h = HL.half_of_frame(f, S)
            assert all(HL.half_of_frame(g, S) == h for g in range(f, f + k))
            call(*[a.ptr for a in self.acc[h]], *[r.ptr for r in self.rec[h]], f, k, P)
        return self.download()

    def download(self):
        return tuple(b.download() for b in self.all())

    def free(self):
        for b in self.all():
            b.free()


def _same(names, got, want, what):
    assert len(got) == len(want) == len(names)
    for name, g, w in zip(names, got, want):
        assert g.tobytes() == w.tobytes(), (what, name, int((g.view(np.uint8).reshape(g.shape[0], g.shape[1], -1) != w.view(np.uint8).reshape(g.shape[0], g.shape[1], -1)).any(-1).sum()))


def _compare(vp, mode, P, first, n, what, fill=None, S=1, runs=False, w=W, h=H):
    a, b = PlaneHalves(vp, mode, w, h, fill), PlaneHalves(vp, mode, w, h, fill)
    try:
        got = a.render(first, n, P)
        want = b.by_definition(first, n, P, S, runs)
        _same(a.names(), got, want, what)
        return got
    finally:
        a.free(); b.free()


# ------------------------------------------------------------------------------------------------------- 1. the definition
@pytest.mark.parametrize("rng_mode", [0, 2], ids=["samplerh", "philox7"])
@pytest.mark.parametrize("est", [0, 1, 2], ids=["global", "decomp", "bounded"])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_halves_are_the_one_frame_plane_calls_of_their_frames(vp, oracle, ctx, mode, est, rng_mode):
    P = _scene(vp, oracle, est, rng_mode)
    _classes_present(vp, P)
    N = len(PLANES[mode])
    for first, n in (SHORT, LONG):
        got = _compare(vp, mode, P, first, n, (mode, est, rng_mode, first, n))
        cnt = [len(HL.frames_of_half(first, n, h)) for h in (0, 1)]
        assert sum(cnt) == n
        for h in (0, 1):
            for k in range(N):
                rec = got[2 * N + h * N + k]
                assert (rec["n"] == cnt[h]).all() and not rec["flags"].any(), (h, k)
        assert any((got[k] != got[N + k]).any() for k in range(N))          # the two halves differ somewhere


# ------------------------------------------------------------------------------------------------------- 2. prefilled buffers
def _minus_zero_fill(vp, N, w=W, h=H):
    """every accumulator -0.0f with one denormal; records non-zero with sum_y = -0.0"""
    acc = np.full((h, w, 4), -0.0, F32)
    acc[0, 0, 0] = F32(1e-40)
    assert np.signbit(acc[acc == 0]).all() and 0 < acc[0, 0, 0] < np.finfo(F32).tiny
    rec = np.zeros((h, w), vp.PIXEL_STATS_DTYPE)
    rec["sum_y"], rec["sum_y2"], rec["n"], rec["flags"] = -0.0, 0.5, 3, 2
    assert np.signbit(rec["sum_y"]).all()
    return (acc,) * (2 * N) + (rec,) * (2 * N)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_one_frame_leaves_the_other_half_alone(vp, oracle, ctx, mode):
    P = _scene(vp, oracle, 0, 2)
    _classes_present(vp, P)
    N = len(PLANES[mode])
    fill = _minus_zero_fill(vp, N)
    for f, mine in ((10, 0), (11, 1)):
        other = 1 - mine
        got = _compare(vp, mode, P, f, 1, ("one frame", mode, f), fill=fill)
        for k in range(N):
            for base in (0, 2 * N):                                          # accumulators, records: every byte of the other half
                assert got[base + other * N + k].tobytes() == fill[base + other * N + k].tobytes(), (f, k, base)
            assert np.signbit(got[other * N + k][1:]).all() and (got[other * N + k][1:] == 0).all()      # its -0.0f is still -0.0f
            rec = got[2 * N + mine * N + k]
            assert (rec["n"] == 4).all() and (rec["flags"] == 2).all()
        if mode == GROUPS:
            continue                                                         # (every sample feeds both planes)
        # within the fed half: where the sample is not an unscattered path's, the transmittance plane is ADDED (0, 0, 0, 0) -- -0.0f
        # turns to +0.0f in all four channels --; where it is, the other planes' colour channels are, and trans.w gains 1
        trans = got[mine * N + N - 1]
        unfed = trans[..., 3] == 0
        assert unfed.any() and (~unfed).any() and (trans[~unfed][:, 3] == 1).all()
        through = ~unfed
        unfed[0, 0] = through[0, 0] = False                                  # (the denormal's pixel)
        assert (trans[unfed] == 0).all() and not np.signbit(trans[unfed]).any()
        first = got[mine * N]
        assert (first[through][:, :3] == 0).all() and not np.signbit(first[through][:, :3]).any()


# ------------------------------------------------------------------------------------------------------- 3. continuation
def _fill(vp, N, seed, w=W, h=H):
    pre = [HL.prefill(w, h, seed + i) for i in range(2 * N)]
    return tuple(a for a, _ in pre) + tuple(r.astype(vp.PIXEL_STATS_DTYPE) for _, r in pre)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_a_second_call_continues_a_first_one(vp, oracle, ctx, mode):
    P = _scene(vp, oracle, 1, 0)
    fill = _fill(vp, len(PLANES[mode]), 40)
    a, b = PlaneHalves(vp, mode, fill=fill), PlaneHalves(vp, mode, fill=fill)
    try:
        a.render(9, 3, P)
        split = a.render(12, 5, P)
        whole = b.render(9, 8, P)
        _same(a.names(), split, whole, "3 + 5 frames against 8")
        assert any(s.tobytes() != f.tobytes() for s, f in zip(split, fill))
    finally:
        a.free(); b.free()


# ------------------------------------------------------------------------------------------------------- 4. a sub-pixel factor
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_subpixel_halves_alternate_in_blocks_of_s_squared(vp, oracle, ctx, mode):
    P = _scene(vp, oracle, 0, 2)
    vp.set_subpixel(2)
    first, n, N = 6, 11, len(PLANES[mode])
    assert first % 4 != 0                                                    # not block-aligned
    got = _compare(vp, mode, P, first, n, "S = 2, per run", S=2, runs=True)
    cnt = [len(HL.frames_of_half(first, n, h, 2)) for h in (0, 1)]
    assert cnt == [5, 6]
    for h in (0, 1):
        for k in range(N):
            assert (got[2 * N + h * N + k]["n"] == cnt[h]).all()


# ------------------------------------------------------------------------------------------------------- 5. a shard
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_a_shard_touches_only_its_pixels(vp, oracle, ctx, mode):
    P = _scene(vp, oracle, 1, 2)
    N = len(PLANES[mode])
    fill = _fill(vp, N, 50)
    vp.set_shard(1, 3)
    try:
        got = _compare(vp, mode, P, SHORT[0], SHORT[1], "rank 1 of 3", fill=fill)
    finally:
        vp.set_shard(0, 1)
    mine = A.owned_pixels(vp, W, H, 1, 3)
    assert mine.any() and (~mine).any()
    cnt = [len(HL.frames_of_half(SHORT[0], SHORT[1], h)) for h in (0, 1)]
    for i in range(4 * N):
        assert got[i][~mine].tobytes() == fill[i][~mine].tobytes(), i
    for h in (0, 1):
        for k in range(N):
            i = 2 * N + h * N + k
            assert (got[i]["n"][mine] == fill[i]["n"][mine] + cnt[h]).all() and np.array_equal(got[i]["flags"], fill[i]["flags"])


# ------------------------------------------------------------------------------------------------------- 6. the staging cap
def test_a_staging_cap_that_splits_the_job_into_launches(vp, oracle, ctx):
    """VP_STAGE_MB=1 in a context of its own (the knob is read when a context first touches its device): a group-layers frame of
    160 x 120 pixels stages two planes of 300 KiB each, so the job goes in launches of vp_groups_frames_per_launch(P, 2) frames"""
    mode, first, n, size = GROUP_LAYERS, 3, 9, (160, 120)
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
            P = _scene(vp, oracle, 0, 1, size=size, key=(1, 2), density=800.0)
            t, d = PlaneHalves(vp, mode, *size), PlaneHalves(vp, mode, *size)
            try:
                per = vp.groups_frames_per_launch(P, 2)
                got = t.render(first, n, P)
                assert vp.groups_frames_per_launch(P, 2) == per
                want = d.by_definition(first, n, P)
                names = t.names()
            finally:
                t.free(); d.free()
    finally:
        c.destroy()
    starts = list(range(first, first + n, per))
    assert per >= 1 and len(starts) >= 3 and any(s % 2 for s in starts), (per, starts)
    _same(names, got, want, "capped staging against the definition")
    # ... and against one unsplit job, in a context with the default cap (`ctx`)
    P = _scene(vp, oracle, 0, 1, size=size, key=(1, 2), density=800.0)
    assert vp.groups_frames_per_launch(P, 2) >= n
    u = PlaneHalves(vp, mode, *size)
    try:
        _same(names, got, u.render(first, n, P), "capped staging against one launch")
    finally:
        u.free()
    for k in range(3):
        assert (got[6 + k]["n"] == 4).all() and (got[9 + k]["n"] == 5).all()


# ------------------------------------------------------------------------------------------------------- 7. exact counts
@pytest.mark.parametrize("mode", [LAYERS, GROUP_LAYERS], ids=["layers", "group_layers"])
def test_the_unscattered_counts_of_the_halves_add_up(vp, oracle, ctx, mode):
    P = _scene(vp, oracle, 0, 2)
    N, (first, n) = len(PLANES[mode]), SHORT
    t = PlaneHalves(vp, mode)
    acc, rec = [vp.DeviceBuffer(W, H) for _ in range(N)], [vp.StatsBuffer(W, H) for _ in range(N)]
    try:
        got = t.render(first, n, P)
        _stats_call(vp, mode)(*[a.ptr for a in acc], *[r.ptr for r in rec], first, n, P)
        whole = acc[N - 1].download()[..., 3]
        w0, w1 = got[N - 1][..., 3], got[2 * N - 1][..., 3]
        assert np.array_equal(w0 + w1, whole) and (whole > 0).any() and (whole < n).any()      # sums of 0 and 1: exact
        assert (w0 != w1).any()
        for k in range(N):
            assert (got[2 * N + k]["n"] + got[3 * N + k]["n"] == n).all()
            assert (rec[k].download()["n"] == n).all()
    finally:
        t.free()
        for b in acc + rec:
            b.free()


# ------------------------------------------------------------------------------------------------------- 8. refusals on the device
@pytest.mark.parametrize("state", ["fast", "mis", "scalar", "counters"])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_states_the_plane_calls_refuse(vp, oracle, ctx, mode, state):
    P = _scene(vp, oracle, 1, 1)
    N = len(PLANES[mode])
    fill = _fill(vp, N, 60)
    t = PlaneHalves(vp, mode, fill=fill)
    try:
        t.render(SHORT[0], 2, P)                                             # the device is in use before the refusal
        t.upload(fill)
        set_, reset = {"fast": (lambda: vp.set_arithmetic(vp.ARITH_FAST), lambda: vp.set_arithmetic(vp.ARITH_EXACT)),
                       "mis": (lambda: vp.set_envmap_sampling(vp.ENV_MIS), lambda: vp.set_envmap_sampling(vp.ENV_PASSIVE)),
                       "scalar": (lambda: vp.set_tracking(vp.TRACK_SCALAR), lambda: vp.set_tracking(vp.TRACK_SPECTRAL)),
                       "counters": (lambda: vp.enable_counters(True), lambda: vp.enable_counters(False))}[state]
        set_()
        try:
            b0, b1 = vp.plane_bufs(t.half(0)), vp.plane_bufs(t.half(1))
            rc = vp.lib().vp_render_frames_planes_halves_stats(mode, C.byref(b0), C.byref(b1), SHORT[0], SHORT[1], C.byref(P))
            assert rc == E_STATE, rc
            assert "vp_render_frames_planes_halves_stats" in vp.lib().vp_last_error().decode()
            vp.synchronize()
            _same(t.names(), t.download(), fill, "refused: every buffer as it was")
        finally:
            reset()
        # the context stays usable
        t.free()
        t = None
        _compare(vp, mode, P, SHORT[0], SHORT[1], ("after the refusal", state))
    finally:
        if t is not None:
            t.free()


# ------------------------------------------------------------------------------------------------------- 9. nothing left behind
def _census(vp, mode, reset=False):
    """(the mode's table, every other render table, the approach walks'): {instance: launches}"""
    tables = {"render": lambda r: vp.launch_census(vp.CENSUS_EXACT, vp.CENSUS_RENDER, reset=r), LAYERS: lambda r: vp.launch_census(vp.CENSUS_EXACT, vp.CENSUS_LAYERS, reset=r),
              GROUPS: lambda r: vp.groups_census(reset=r), GROUP_LAYERS: lambda r: vp.group_layers_census(reset=r)}
    own = tables.pop(mode)(reset)
    others = {k: f(reset) for k, f in tables.items()}
    return own, others, vp.launch_census(vp.CENSUS_EXACT, vp.CENSUS_APPROACH, reset=reset)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_the_call_leaves_nothing_behind_and_launches_the_plane_calls_instances(vp, oracle, ctx, mode):
    P = _scene(vp, oracle, 0, 2)
    N = len(PLANES[mode])
    buf, t = vp.DeviceBuffer(W, H), PlaneHalves(vp, mode)
    acc, rec = [vp.DeviceBuffer(W, H) for _ in range(N)], [vp.StatsBuffer(W, H) for _ in range(N)]
    plain = lambda: _stats_call(vp, mode)(*[a.ptr for a in acc], *[r.ptr for r in rec], LONG[0], LONG[1], P)
    try:
        vp.render_frames(buf.ptr, 8, 6, P)
        beauty = buf.download()
        _census(vp, mode, reset=True)
        plain()
        stats_census = _census(vp, mode, reset=True)
        planes_before = [b.download() for b in acc + rec]
        t.render(LONG[0], LONG[1], P)
        own, others, approach = _census(vp, mode, reset=True)
        assert sum(own.values()) >= 1 and own == stats_census[0], "the mode's census kind, the _stats call's instances"
        assert all(sum(o.values()) == 0 for o in others.values()), "no other kind"
        assert approach == stats_census[2]
        assert vp.last_pipelined() == 0
        buf.reset()
        vp.render_frames(buf.ptr, 8, 6, P)
        assert buf.download().tobytes() == beauty.tobytes() and vp.last_pipelined() == 1
        for b in acc + rec:
            b.reset()
        plain()
        for b, want in zip(acc + rec, planes_before):
            assert b.download().tobytes() == want.tobytes()
    finally:
        buf.free(); t.free()
        for b in acc + rec:
            b.free()


# ------------------------------------------------------------------------------------------------------- 10. the output stage
class FloatBuffer:
    def __init__(self, vp, n):
        self.vp, self.n = vp, n
        self.ptr = vp.lib().vp_malloc(max(n, 1) * 4)
        assert self.ptr

    def download(self, shape):
        out = np.empty(shape, F32)
        assert self.vp.lib().vp_download(out.ctypes.data_as(C.c_void_p), self.ptr, out.nbytes) == 0
        return out

    def free(self):
        self.vp.lib().vp_free(self.ptr)


@pytest.mark.parametrize("variance", [None, (1, 3, 0.45)], ids=["plain", "variance"])
def test_the_cross_filter_per_plane_equals_the_calls_and_the_restatement(vp, oracle, ctx, variance):
    Wp, Hp, R, Fp, k = 32, 24, 3, 1, 0.45
    mode, names = GROUP_LAYERS, PLANES[GROUP_LAYERS]
    floors = (1e-3, 1e-3, 1e-2)
    P = _scene(vp, oracle, 0, 2, size=(Wp, Hp))
    t = PlaneHalves(vp, mode, Wp, Hp)
    ta, tb = vp.DeviceBuffer(Wp, Hp), vp.DeviceBuffer(Wp, Hp)
    dst = [vp.DeviceBuffer(Wp, Hp) for _ in names]
    res = [FloatBuffer(vp, Wp * Hp) for _ in names]
    var = [FloatBuffer(vp, Wp * Hp) for _ in range(3)]
    one, one_res = vp.DeviceBuffer(Wp, Hp), FloatBuffer(vp, Wp * Hp)
    try:
        before = t.render(0, 16, P)
        h = [before[:3], before[3:6]]
        r = [before[6:9], before[9:12]]
        assert all((x["n"] == 8).all() for x in r[0] + r[1])
        assert [vp.PLANE_RESID_FLOOR[n] for n in names] == list(floors)
        try:
            for form in (0, 1):
                vp.set_denoise_form(form)
                for b in dst:
                    b.reset()
                vp.denoise_cross_planes(mode, [b.ptr for b in dst], [b.ptr for b in res], t.half(0), t.half(1), ta.ptr, tb.ptr, Wp, Hp, R, Fp, k,
                                        variance=variance, var_ptrs=[b.ptr for b in var] if variance else None)
                for j, name in enumerate(names):
                    if variance is None:
                        want, want_resid, _, _ = HL.denoise_cross(h[0][j], r[0][j], h[1][j], r[1][j], R, Fp, k, floor_y=floors[j])
                    else:
                        want, want_resid, _, _, _ = VL.denoise_cross_var(h[0][j], r[0][j], h[1][j], r[1][j], R, Fp, k, variance=variance, floor_y=floors[j])
                    got, got_resid = dst[j].download(), res[j].download((Hp, Wp))
                    assert got.tobytes() == want.tobytes() and got_resid.tobytes() == want_resid.tobytes(), (form, name)
                    # the explicit sequence of library calls for this plane
                    a0, s0, a1, s1 = t.acc[0][j].ptr, t.rec[0][j].ptr, t.acc[1][j].ptr, t.rec[1][j].ptr
                    if variance is None:
                        vp.denoise_guided(ta.ptr, a0, s0, Wp, Hp, (), R, Fp, k, guide_ptr=a1, guide_stats_ptr=s1)
                        vp.denoise_guided(tb.ptr, a1, s1, Wp, Hp, (), R, Fp, k, guide_ptr=a0, guide_stats_ptr=s0)
                    else:
                        vp.halves_variance(var[0].ptr, var[1].ptr, s0, s1, Wp * Hp)
                        vp.filter_variance(var[2].ptr, var[0].ptr, var[1].ptr, Wp, Hp, *variance)
                        vp.denoise_var(ta.ptr, a0, s0, Wp, Hp, var[2].ptr, (), R, Fp, k, guide_ptr=a1, guide_stats_ptr=s1)
                        vp.denoise_var(tb.ptr, a1, s1, Wp, Hp, var[2].ptr, (), R, Fp, k, guide_ptr=a0, guide_stats_ptr=s0)
                    vp.merge_halves(one.ptr, one_res.ptr, ta.ptr, s0, tb.ptr, s1, Wp * Hp, floors[j])
                    assert one.download().tobytes() == got.tobytes() and one_res.download((Hp, Wp)).tobytes() == got_resid.tobytes(), (form, name)
                    assert np.isfinite(got).all() and np.isfinite(got_resid).all()
        finally:
            vp.set_denoise_form(0)
        assert any(res[j].download((Hp, Wp)).max() > 0 for j in range(3))
        _same(t.names(), t.download(), before, "the halves did not change under the filters")
    finally:
        t.free()
        for b in [ta, tb, one, one_res] + dst + res + var:
            b.free()
