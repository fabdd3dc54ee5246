"""GPU suite: the output-stage filters at the tile's own edges and at the ends of the magnitude range.

Part 1, shapes.  The 32 x 8 tile of csrc/vp_denoise.hip exactly (32 x 8), a whole number of tiles (64 x 16), one pixel short of a
tile (31 x 7), one pixel over on both axes at once (65 x 17), a column one pixel wide and taller than a tile (1 x 40: 31 of 32 lanes
of every workgroup are outside the image and the whole halo clamps to one column) and a row one pixel high and wider than three
tiles (100 x 1: every patch row clamps to the same row).  And the early exit of denoise_tiled_k / denoise_guided_tiled_k for a tile
without a noisy pixel, on records whose flat block covers two whole tiles next to noisy tiles that read it as halo.

Part 2, magnitudes (filter_cases_lib.REGIMES).  dark: luminances times 1e-17 -- variances of the mean that are subnormal or underflow
to 0, so that eps = 1e-20f carries the pair term's denominator; bright: times 1e13 -- d * d and v_a + v_b near the end of binary32;
normal is the control.  vp_filter_variance, whose planes are squared and fourth-power luminances, at 1e-9 and 1e4; vp_select on error
planes whose every value and box sum is subnormal.  This pins on these kernels what the build promises: no denormal flushing,
correctly rounded division, and a (float) of a binary64 quotient that rounds into the subnormal range as numpy's does.

Every comparison is filter_cases_lib.hold: both forms, a NaN-filled destination fully overwritten, tobytes() equality of the whole
output with the numpy restatement; the inputs are downloaded again afterwards.  tests/test_filter_edges_cpu.py asserts on the
restatement that each case reaches the edge it is named for.

Measured on an MI355X: the slowest case takes 0.14 s (vp_filter_variance and vp_select at 65 x 17: the restatement of the (10, 3) window
is most of it), a regime case at most 0.08 s; all 24 cases 1.2 s."""
import numpy as np
import pytest

import adaptive_lib as A
import denoise_guided_lib as G
import denoise_lib as D
import filter_cases_lib as FC
import halves_lib as HL
import select_lib as S
import variance_lib as V
from test_denoise_guided_gpu import NF_LISTS

pytestmark = pytest.mark.gpu

F32 = np.float32
K = 0.45
SIZES = [(32, 8), (31, 7), (64, 16), (65, 17), (1, 40), (100, 1)]


@pytest.fixture(autouse=True)
def _restore(vp):
    yield
    vp.set_denoise_form(0)


_memo = {}


def once(key, make):
    """a restatement's answer, computed once and never changed"""
    if key not in _memo:
        _memo[key] = make()
        for a in (_memo[key] if isinstance(_memo[key], tuple) else (_memo[key],)):
            a.setflags(write=False)
    return _memo[key]


def feature_planes(W, H, seed):
    alpha, depth = once(("feat", W, H, seed), lambda: G.synthetic_features(W, H, seed))
    return {"a": alpha, "d": depth}


def host_features(planes, nf):
    return [(planes[p], c, s) for p, c, s in NF_LISTS[nf]]


# ---- part 1: tile-edge shapes
def shape_inputs(W, H):
    def make():
        acc, rec = D.synthetic(W, H, 600 + W)
        gacc, grec = D.synthetic(W, H, 700 + W)
        plane, _ = V.halves_variance(rec, grec)
        plane[np.random.default_rng(W).random((H, W)) < 0.1] = 0
        return acc, rec, gacc, grec, plane
    return once(("shape", W, H), make)


@pytest.mark.parametrize("W,H", SIZES)
def test_colour_filters_at_tile_edge_shapes(vp, W, H):
    acc, rec, gacc, grec, plane = shape_inputs(W, H)
    planes = feature_planes(W, H, 600 + W)
    dev = FC.Dev(vp)
    try:
        src, stats = dev.pair(acc, rec)
        guide, gstats = dev.pair(gacc, grec)
        dplanes = {n: dev.put(p) for n, p in planes.items()}
        dplane = dev.put(plane)
        dst = dev.out((H, W, 4))
        kw, hkw = dict(guide_ptr=guide, guide_stats_ptr=gstats), dict(guide=gacc, guide_rec=grec)
        for R, F in ((2, 1), (5, 3)):                       # vp_denoise, a separate guide pair
            want = once(("d", W, H, R, F), lambda: D.denoise(acc, rec, R, F, K, **hkw))
            FC.hold(vp, lambda: vp.denoise(dst.ptr, src, stats, W, H, R, F, K, **kw), [dst], [want], ("vp_denoise", W, H, R, F))
        want = once(("g", W, H), lambda: G.denoise_guided(acc, rec, host_features(planes, 2), 5, 1, K))
        FC.hold(vp, lambda: vp.denoise_guided(dst.ptr, src, stats, W, H, host_features(dplanes, 2), 5, 1, K), [dst], [want],
                ("vp_denoise_guided", W, H))          # self-guided
        want = once(("v", W, H), lambda: V.denoise_var(acc, rec, plane, 3, 2, K, host_features(planes, 1), **hkw))
        FC.hold(vp, lambda: vp.denoise_var(dst.ptr, src, stats, W, H, dplane, host_features(dplanes, 1), 3, 2, K, **kw), [dst], [want],
                ("vp_denoise_var", W, H))
        assert dev.untouched()
    finally:
        dev.free()


@pytest.mark.parametrize("W,H", SIZES)
def test_variance_filter_and_selection_at_tile_edge_shapes(vp, W, H):
    dev = FC.Dev(vp)
    try:
        dst = dev.out((H, W))
        for kind in ("block", "isolated"):
            u, q = once(("uq", W, H, kind), lambda: V.planes(W, H, 300 + W, kind))
            du, dq = dev.put(u), dev.put(q)
            for R, F in ((1, 3), (10, 3)):
                want = once(("fv", W, H, kind, R), lambda: V.filter_variance(u, q, R, F, K))
                got, = FC.hold(vp, lambda: vp.filter_variance(dst.ptr, du, dq, W, H, R, F, K), [dst], [want], ("vp_filter_variance", W, H, kind, R, F))
                assert not got[u == 0].any()
        img, idx = dev.out((H, W, 4)), dev.out((H, W), np.uint8)
        for kind in ("noise", "ties", "block"):
            both = once(("sel", W, H, kind), lambda: tuple(S.images_for(W, H, 4, 400 + W) + S.error_planes(W, H, 4, 500 + W, kind)))
            imgs, errs = both[:4], both[4:]
            want = once(("pick", W, H, kind), lambda: S.select(list(imgs), list(errs), 3, 3))
            dimg, derr = [dev.put(a) for a in imgs], [dev.put(a) for a in errs]
            FC.hold(vp, lambda: vp.select(img.ptr, idx.ptr, dimg, derr, W, H, 3, 3), [img, idx], list(want), ("vp_select", W, H, kind))
        assert dev.untouched()
    finally:
        dev.free()


def test_whole_flat_tiles_leave_early_and_serve_their_neighbours(vp):
    """records whose flat block is rows 8..23, columns 32..63 of 70 x 37: tiles (1, 1) and (1, 2) hold no noisy pixel and take the
    early exit, their neighbours stage them as halo"""
    W, H = FC.FLAT_TILE_SIZE
    y0, y1, x0, x1 = FC.FLAT_TILE_RECT
    acc, rec = FC.flat_tile_pair()
    planes = feature_planes(W, H, FC.FLAT_TILE_SEED)
    mean = A.scale_by_count(acc, rec["n"], 1.0)
    noisy = D.variance(rec) != 0
    assert not noisy[y0:y1, x0:x1].any()
    near = np.zeros((H, W), bool)
    near[y0 - 5:y1 + 5, x0 - 5:x1 + 5] = True           # within R = 5 of the block
    near[y0:y1, x0:x1] = False
    near &= noisy
    assert near.sum() > 300
    dev = FC.Dev(vp)
    try:
        src, stats = dev.pair(acc, rec)
        dplanes = {n: dev.put(p) for n, p in planes.items()}
        dst = dev.out((H, W, 4))
        want = once(("flat", "d"), lambda: D.denoise(acc, rec, 5, 2, K))
        got_d, = FC.hold(vp, lambda: vp.denoise(dst.ptr, src, stats, W, H, 5, 2, K), [dst], [want], "vp_denoise on whole flat tiles")
        want = once(("flat", "g"), lambda: G.denoise_guided(acc, rec, host_features(planes, 3), 5, 1, K))
        got_g, = FC.hold(vp, lambda: vp.denoise_guided(dst.ptr, src, stats, W, H, host_features(dplanes, 3), 5, 1, K), [dst], [want],
                         "vp_denoise_guided on whole flat tiles")
        for got in (got_d, got_g):
            assert got[y0:y1, x0:x1].tobytes() == mean[y0:y1, x0:x1].tobytes()                       # the block: the plain mean
            # its noisy neighbours are filtered.  Not every one differs from its mean: where every neighbour's weight is below half an
            # ulp of the centre's 1 the definition's answer is c * 1 / 1 (38 and 7 of the 500 here, tests/test_filter_edges_cpu.py)
            assert (got[..., :3] != mean[..., :3]).any(-1)[near].sum() > 0.75 * near.sum()
        assert dev.untouched()
    finally:
        dev.free()


# ---- part 2: magnitude regimes
@pytest.mark.parametrize("regime", list(FC.REGIMES))
def test_colour_filters_in_a_magnitude_regime(vp, regime):
    W, H = FC.EDGE_W, FC.EDGE_H
    (h0, r0), (h1, r1) = FC.regime_pairs(regime)
    planes = feature_planes(W, H, 140)
    dev = FC.Dev(vp)
    try:
        src, stats = dev.pair(h0, r0)
        guide, gstats = dev.pair(h1, r1)
        dplanes = {n: dev.put(p) for n, p in planes.items()}
        dst = dev.out((H, W, 4))
        for R, F, k in ((2, 1, 0.45), (5, 3, 2.0)):
            for kw, hkw in ((dict(), dict()), (dict(guide_ptr=guide, guide_stats_ptr=gstats), dict(guide=h1, guide_rec=r1))):
                want = once((regime, "d", R, F, bool(kw)), lambda: D.denoise(h0, r0, R, F, k, **hkw))
                FC.hold(vp, lambda: vp.denoise(dst.ptr, src, stats, W, H, R, F, k, **kw), [dst], [want], (regime, "vp_denoise", R, F, k, bool(kw)))
        want = once((regime, "g"), lambda: G.denoise_guided(h0, r0, host_features(planes, 2), 5, 1, K))
        FC.hold(vp, lambda: vp.denoise_guided(dst.ptr, src, stats, W, H, host_features(dplanes, 2), 5, 1, K), [dst], [want], (regime, "vp_denoise_guided"))
        # vp_denoise_var at (3, 1), fed with the restatement's pooled and filtered plane of the two pairs
        uf = once((regime, "uf"), lambda: V.filter_variance(*V.halves_variance(r0, r1), 1, 3, K))
        duf = dev.put(uf)
        want = once((regime, "v"), lambda: V.denoise_var(h0, r0, uf, 3, 1, K, guide=h1, guide_rec=r1))
        FC.hold(vp, lambda: vp.denoise_var(dst.ptr, src, stats, W, H, duf, (), 3, 1, K, guide_ptr=guide, guide_stats_ptr=gstats), [dst], [want],
                (regime, "vp_denoise_var"))
        assert dev.untouched()
    finally:
        dev.free()


@pytest.mark.parametrize("regime", list(FC.REGIMES))
def test_pointwise_kernels_in_a_magnitude_regime(vp, regime):
    """halves_variance_k, merge_halves_k, cross_error_k and accumulate_stats_k of csrc/vp_kernels.hip on the two scaled pairs"""
    W, H = FC.EDGE_W, FC.EDGE_H
    n = W * H
    (h0, r0), (h1, r1) = FC.regime_pairs(regime)
    floor_y = float(F32(1e-3 * FC.REGIMES[regime]))                  # inside the luminance range, so that both sides of the floor occur
    fa = once((regime, "fa"), lambda: D.denoise(h0, r0, 2, 1, K, guide=h1, guide_rec=r1))
    fb = once((regime, "fb"), lambda: D.denoise(h1, r1, 2, 1, K, guide=h0, guide_rec=r0))
    dev = FC.Dev(vp)
    try:
        a, sa = dev.pair(h0, r0)
        b, sb = dev.pair(h1, r1)
        dfa, dfb = dev.put(fa), dev.put(fb)
        u, q, err, resid, dst = dev.out((H, W)), dev.out((H, W)), dev.out((H, W)), dev.out((H, W)), dev.out((H, W, 4))
        FC.hold(vp, lambda: vp.halves_variance(u.ptr, q.ptr, sa, sb, n), [u, q], list(V.halves_variance(r0, r1)), (regime, "vp_halves_variance"), pointwise=True)
        want, want_resid = HL.merge_halves(fa, r0, fb, r1, floor_y)
        assert (A.luminance(want) > F32(floor_y)).any() and (A.luminance(want) < F32(floor_y)).any() and (want_resid > 0).sum() > 300
        FC.hold(vp, lambda: vp.merge_halves(dst.ptr, resid.ptr, dfa, sa, dfb, sb, n, floor_y), [dst, resid], [want, want_resid], (regime, "vp_merge_halves"),
                pointwise=True)
        FC.hold(vp, lambda: vp.cross_error(err.ptr, dfa, dfb, a, sa, b, sb, n), [err], [S.cross_error(fa, fb, h0, r0, h1, r1)], (regime, "vp_cross_error"),
                pointwise=True)
        assert dev.untouched()
        # vp_accumulate_stats adds in place: a copy of the first half's records is the destination
        total = vp.StatsBuffer(W, H)
        try:
            total.upload(np.ascontiguousarray(r0, vp.PIXEL_STATS_DTYPE))
            vp.accumulate_stats(total.ptr, sb, n)
            want = np.ascontiguousarray(HL.accumulate_stats(r0, r1), vp.PIXEL_STATS_DTYPE)
            assert total.download().tobytes() == want.tobytes(), (regime, "vp_accumulate_stats")
        finally:
            total.free()
        assert dev.untouched()
    finally:
        dev.free()


@pytest.mark.parametrize("regime", list(FC.VARIANCE_REGIMES))
def test_variance_filter_in_a_magnitude_regime(vp, regime):
    W, H = FC.EDGE_W, FC.EDGE_H
    dev = FC.Dev(vp)
    try:
        dst = dev.out((H, W))
        for kind in ("block", "isolated"):
            u, q = FC.regime_planes(regime, kind)
            du, dq = dev.put(u), dev.put(q)
            for R, F in ((1, 3), (10, 3)):
                want = once((regime, "fv", kind, R), lambda: V.filter_variance(u, q, R, F, K))
                got, = FC.hold(vp, lambda: vp.filter_variance(dst.ptr, du, dq, W, H, R, F, K), [dst], [want], (regime, "vp_filter_variance", kind, R, F))
                assert not got[u == 0].any()
        assert dev.untouched()
    finally:
        dev.free()


@pytest.mark.parametrize("Rs,Rb", [(3, 3), (1, 0)])
def test_selection_among_subnormal_errors(vp, Rs, Rb):
    W, H = FC.EDGE_W, FC.EDGE_H
    errs = FC.tiny_errors()
    imgs = once("imgs", lambda: tuple(S.images_for(W, H, 4, 440)))
    want = once(("tiny", Rs, Rb), lambda: S.select(list(imgs), errs, Rs, Rb))
    dev = FC.Dev(vp)
    try:
        dimg, derr = [dev.put(a) for a in imgs], [dev.put(a) for a in errs]
        dst, idx = dev.out((H, W, 4)), dev.out((H, W), np.uint8)
        FC.hold(vp, lambda: vp.select(dst.ptr, idx.ptr, dimg, derr, W, H, Rs, Rb), [dst, idx], list(want), ("vp_select on subnormal errors", Rs, Rb))
        assert dev.untouched()
    finally:
        dev.free()
