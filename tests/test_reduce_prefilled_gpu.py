"""The reduces, started from buffers that are not zero.

Every other test hands the library zeroed accumulators and records.  Here every accumulator holds a pattern of -0.0f, a denormal and
ordinary values, varied by pixel, channel and plane, and every record sum_y = -0.0 with sum_y2 and n above zero.  A sample that does not
feed a plane is ADDED to it as +0.0f, which turns a -0.0f accumulator into +0.0f; a reduce that skipped the addition, multiplied a
constant by the frame count or started its sums from zero would show here and nowhere else.

The eight vp_render_frames* forms and the four adaptive forms run on layers_lib's small Julia image (general, light and box-missing
pixels), 3 frames from frame 0 and from frame 3.  The expectation is the existing restatement continued from the same state:
adaptive_lib.Stats folded by plane_stats_lib.fold, and the round loops of adaptive_lib, adaptive_planes_lib and
adaptive_group_layers_lib, on the samples of group_layers_lib.Samples.  Everything is compared by bits.  A few pixels carry FROZEN in
their records: the plain and _stats forms neither read nor write it, the adaptive forms must hand those pixels back byte for byte."""
import numpy as np
import pytest

import adaptive_group_layers_lib as AG
import adaptive_lib as AL
import adaptive_planes_lib as AP
import group_layers_lib as GLL
import layers_lib as LL
import plane_stats_lib as PS

pytestmark = pytest.mark.gpu

W, H, N = LL.W, LL.H, 3
FIRSTS = (0, 3)
EST, RNG = 0, 1                   # the global majorant on Philox: no optical-depth table to precompute
F32 = np.float32
DENORMAL = F32(1e-40)
PATTERN = np.array([-0.0, DENORMAL, 0.75, -0.0, -2.5, 3e-3, -0.0], F32)
# the planes of each mode, by their names in group_layers_lib.Samples (its `trans` is the layers call's too: zero where scattered)
MODES = {"one": ("beauty",), "layers": ("fg", "trans"), "groups": ("gsun", "gsky"), "group_layers": ("sun", "sky", "trans")}
FROZEN_ALL = (5, 40, 77, 100, 150, 191)      # pixels (y * W + x) frozen in every record
FROZEN_ONE = ((20, 0), (60, -1))             # (pixel, plane): frozen in that plane's record alone -- inactive all the same
ADAPT = dict(min_frames=5, round_frames=2)
# per plane, so that a criterion read from the wrong plane shows.  Chosen on the CPU oracle alone (check_oracle_side): with these the
# first round freezes some pixels of every mode and not all, and the second leaves some active
REL_TOL, FLOOR_Y = (0.62, 1.0, 1.2), (1e-3, 2e-3, 3e-3)


def samples(oracle):
    return GLL.expected(oracle, "julia", EST, RNG, frames=range(0, FIRSTS[-1] + N))


def prefilled(mode):
    """the state before a call: one adaptive_lib.Stats per plane of `mode`"""
    out = []
    for k in range(len(MODES[mode])):
        st = AL.Stats(W, H)
        e = np.arange(W * H * 4).reshape(H, W, 4) + 3 * k
        st.acc[...] = PATTERN[e % len(PATTERN)]
        i = np.arange(W * H).reshape(H, W) + k
        st.sum_y[...] = -0.0
        st.sum_y2[...] = 1e-8 * (1 + i % 5)
        st.n[...] = 2 + k + np.arange(W * H).reshape(H, W) % 3      # (below min_frames after the first round in plane 0 of every third pixel)
        st.flags.reshape(-1)[list(FROZEN_ALL)] = AL.FROZEN
        out.append(st)
    for pix, plane in FROZEN_ONE:
        out[plane].flags.reshape(-1)[pix] = AL.FROZEN
    return tuple(out)


def frames_of(E, mode):
    return lambda f: tuple(getattr(E, p)[f - E.first] for p in MODES[mode])


def expected(E, mode, form, first):
    """(the Stats per plane after the call, the adaptive result or None)"""
    st, frame, n_planes = prefilled(mode), frames_of(E, mode), len(MODES[mode])
    if form != "adaptive":
        return PS.fold(frame, W, H, first, N, into=st), None
    tol, fl = REL_TOL[:n_planes], FLOOR_Y[:n_planes]
    if n_planes == 1:
        res = AL.render_adaptive(st[0], lambda f: frame(f)[0], first, N, tol[0], fl[0], ADAPT["min_frames"], ADAPT["round_frames"])
    elif n_planes == 2:
        res = AP.render_adaptive_planes(st, frame, first, N, tol, fl, ADAPT["min_frames"], ADAPT["round_frames"])
    else:
        res = AG.render_adaptive_group_layers(st, frame, first, N, tol, fl, ADAPT["min_frames"], ADAPT["round_frames"])
    return st, res


def check_oracle_side(E, mode, first):
    """the expectation alone must exercise what the test is about, in every plane: a -0.0f that becomes +0.0f, a -0.0f that a sample
    replaces by a non-zero, a denormal that survives an addition of +0.0f -- and a record sum that leaves -0.0"""
    before, (after, _) = prefilled(mode), expected(E, mode, "stats", first)
    for k, plane in enumerate(MODES[mode]):
        b, a = before[k].acc.view(np.uint32), after[k].acc.view(np.uint32)
        neg0 = b == 0x80000000
        assert (neg0 & (a == 0)).any(), (mode, plane, "no -0.0f accumulator becomes +0.0f")
        assert (neg0 & ((a & 0x7fffffff) != 0)).any(), (mode, plane, "no -0.0f accumulator receives a non-zero")
        assert ((b == DENORMAL.view(np.uint32)) & (a == b)).any(), (mode, plane, "no denormal survives")
        # (sum_y = -0.0 leaves by an addition too: +0.0 where the plane's three samples are black, which no pixel of sun-and-sky planes is)
        sy = after[k].sum_y.view(np.uint64)
        black = np.all([AL.luminance(getattr(E, plane)[f - E.first]) == 0 for f in range(first, first + N)], axis=0)
        assert (sy[black] == 0).all() and ((sy[~black] & 0x7fffffffffffffff) != 0).all() and not black.all(), (mode, plane, "sum_y")
        assert black.any() or plane in ("beauty", "gsky"), (mode, plane, "no record whose sum_y becomes +0.0")
    # ... and the adaptive form a second round on a list that the first has shortened, with pixels left over at the end
    res, active0 = expected(E, mode, "adaptive", first)[1], W * H - len(FROZEN_ALL) - len(FROZEN_ONE)
    assert res["rounds"] == 2 and 0 < res["active_left"] and active0 * 2 < res["samples"] < active0 * N, (mode, res)


class Buffers:
    def __init__(self, vp, n_planes):
        self.acc = tuple(vp.DeviceBuffer(W, H) for _ in range(n_planes))
        self.rec = tuple(vp.StatsBuffer(W, H) for _ in range(n_planes))

    def upload(self, st):
        for b, r, s in zip(self.acc, self.rec, st):
            b.upload(s.acc)
            r.upload(s.records())

    def download(self):
        return tuple(b.download() for b in self.acc), tuple(r.download() for r in self.rec)

    def ptrs(self, with_records):
        return [b.ptr for b in self.acc + (self.rec if with_records else ())]

    def free(self):
        for b in self.acc + self.rec:
            b.free()


def call(vp, mode, form, B, first, P):
    """the library's call of (mode, form); returns the adaptive result or None"""
    stem = {"one": "", "layers": "_layers", "groups": "_groups", "group_layers": "_group_layers"}[mode]
    if form == "plain":
        return getattr(vp, "render_frames" + stem)(*B.ptrs(False), first, N, P)
    if form == "stats":
        return getattr(vp, "render_frames" + stem + "_stats")(*B.ptrs(True), first, N, P)
    n = len(MODES[mode])
    tol, fl = (REL_TOL[:n], FLOOR_Y[:n]) if n > 1 else (REL_TOL[0], FLOOR_Y[0])
    return getattr(vp, "render_adaptive" + stem)(*B.ptrs(True), first, N, P, tol, fl, ADAPT["min_frames"], ADAPT["round_frames"])


@pytest.mark.parametrize("first", FIRSTS)
@pytest.mark.parametrize("mode", list(MODES))
def test_reduces_continue_from_prefilled_buffers(vp, oracle, mode, first):
    import test_group_layers_gpu as TG
    E = samples(oracle)
    check_oracle_side(E, mode, first)
    c = vp.Context(0)
    try:
        with c:
            P = TG._scene(vp, oracle, "julia", EST, RNG)
            general, light, miss = vp.pixel_lists(P)
            assert len(general) and len(light) and len(miss)
            B = Buffers(vp, len(MODES[mode]))
            try:
                for form in ("plain", "stats", "adaptive"):
                    before = prefilled(mode)
                    B.upload(before)
                    res = call(vp, mode, form, B, first, P)
                    acc, rec = B.download()
                    want, want_res = expected(E, mode, form, first)
                    for k, plane in enumerate(MODES[mode]):
                        what = (mode, form, first, plane)
                        if form == "plain":      # accumulators only: the records come back as they went
                            assert AL.equal_bits(want[k].acc, acc[k]), what
                            assert rec[k].tobytes() == before[k].records().tobytes(), what
                            continue
                        bad = AL.same_state(want[k], acc[k], rec[k])
                        assert bad is None, what + (bad,)
                        if form == "stats":      # FROZEN is neither read nor written: every pixel received its frames
                            assert np.array_equal(rec[k]["flags"], before[k].flags) and np.array_equal(rec[k]["n"], before[k].n + N), what
                            continue
                        off = ~AG.active_mask(before, AL.all_pixels(W, H))      # frozen in some record of the pixel
                        assert off.sum() == len(FROZEN_ALL) + len(FROZEN_ONE)
                        assert acc[k][off].tobytes() == before[k].acc[off].tobytes(), what + ("an inactive pixel's accumulator changed",)
                        assert rec[k][off].tobytes() == before[k].records()[off].tobytes(), what + ("an inactive pixel's record changed",)
                    if form == "adaptive":
                        assert res == want_res, (mode, first, res, want_res)
            finally:
                B.free()
    finally:
        c.destroy()
