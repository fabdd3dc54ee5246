"""Every compiled tiled kernel of the output-stage filters runs once and is held to its restatement.

csrc/vp_denoise.hip compiles denoise_tiled_k<F> for F = 0..3 and denoise_guided_tiled_k<F, NF> for F = 0..3 x NF = 1..4, each with
and without vp_denoise_var's variance plane (8 + 32 instances), variance_tiled_k<F> (4), select_tiled_k, and the plain forms.  The
LDS layout differs per (F, NF): the pitch of the (y, v) planes is 64 + 2F, the e planes are (32 + 2F)(8 + 2F), and NF feature planes
lie behind them.  INSTANCES lists them all; it is data, written from the launchers, and tests/test_filter_instances_cpu.py holds it to
the launch sites of the source, so an instance added later without a row fails there.

Every row runs on one 40 x 17 image -- two tile columns and three tile rows, partial on both axes, a halo that clamps on all four
sides -- at R = 2, k = 0.45, with a source pair and a separate guide pair, in both forms, and is compared tobytes() with the numpy
restatement (filter_cases_lib.hold); the inputs are downloaded again afterwards.  A guided row must differ from the feature-less call
at the same (R, F): a row that ran another instance's feature count would show.  vp_select, one kernel with loops guarded by n: n = 1,
2, 3, 4 at the radii (2, 1), (1, 2), (2, 2) that the rest of the suite does not use.

Measured on an MI355X: the slowest case takes 0.05 s (a vp_select case: three kinds x four candidate counts, restatement included), a
colour or variance row 0.01 s; all 48 cases 0.5 s, 0.26 s of it the first use of the device.  Before this test the suite's tiled
launches reached 9 of the 16 plane-less and 2 of the 16 plane instances of denoise_guided_tiled_k, 3 of the 4 plane instances of
denoise_tiled_k and 3 of the 4 of variance_tiled_k (BEFORE); the table runs them all, and vp_select with n = 3 and a radius of 2."""
import numpy as np
import pytest

import denoise_guided_lib as G
import denoise_lib as D
import filter_cases_lib as FC
import select_lib as S
import variance_lib as V
from test_denoise_guided_gpu import NF_LISTS

pytestmark = pytest.mark.gpu

W, H, R, K = 40, 17, 2, 0.45
SRC_SEED, GUIDE_SEED = 140, 141
PATCHES, FEATURE_COUNTS = (0, 1, 2, 3), (1, 2, 3, 4)

# (call, kernel, explicit integer template arguments, with vp_denoise_var's plane) -- from launch_denoise_v, launch_guided_tiled,
# launch_denoise_guided_v, launch_filter_variance and launch_select of csrc/vp_denoise.hip
INSTANCES = (
    [("vp_denoise", "denoise_tiled_k", (F,), False) for F in PATCHES]
    + [("vp_denoise_guided", "denoise_guided_tiled_k", (F, NF), False) for F in PATCHES for NF in FEATURE_COUNTS]
    + [("vp_denoise_var", "denoise_tiled_k", (F,), True) for F in PATCHES]
    + [("vp_denoise_var", "denoise_guided_tiled_k", (F, NF), True) for F in PATCHES for NF in FEATURE_COUNTS]
    + [("vp_filter_variance", "variance_tiled_k", (F,), False) for F in PATCHES]
    + [("vp_select", "select_tiled_k", (), False)])
# the plain forms: F and NF are arguments there, the plane is the one template parameter.  Every row above runs them as its form 1
PLAIN_INSTANCES = [("denoise_plain_k", (), False), ("denoise_plain_k", (), True), ("denoise_guided_plain_k", (), False),
                   ("denoise_guided_plain_k", (), True), ("variance_plain_k", (), False), ("select_plain_k", (), False)]
# what the suite launched before this test (tiled form), read off the older tests' parameters
BEFORE = {
    ("denoise_tiled_k", False): {(0,), (1,), (2,), (3,)},
    ("denoise_tiled_k", True): {(1,), (2,), (3,)},
    ("variance_tiled_k", False): {(0,), (2,), (3,)},
    ("denoise_guided_tiled_k", False): {(1, 1), (1, 2), (1, 3), (1, 4), (0, 2), (2, 2), (2, 3), (3, 1), (3, 4)},
    ("denoise_guided_tiled_k", True): {(1, 2), (3, 2)},
}

COLOUR_ROWS = [r for r in INSTANCES if r[1] in ("denoise_tiled_k", "denoise_guided_tiled_k")]
VARIANCE_ROWS = [r for r in INSTANCES if r[1] == "variance_tiled_k"]
SELECT_RADII = [(2, 1), (1, 2), (2, 2)]


def row_id(row):
    return "%s-%s%s%s" % (row[0], row[1], "".join("-%d" % a for a in row[2]), "-plane" if row[3] else "")


@pytest.fixture(autouse=True)
def _restore(vp):
    yield
    vp.set_denoise_form(0)


_memo = {}


def inputs():
    """the source pair, the guide pair, the feature planes and vp_denoise_var's per-sample variance plane, made once"""
    if "in" not in _memo:
        acc, rec = D.synthetic(W, H, SRC_SEED)
        gacc, grec = D.synthetic(W, H, GUIDE_SEED)
        alpha, depth = G.synthetic_features(W, H, SRC_SEED)
        # a zero block over the whole tile at rows 8..15, columns 0..31, and scattered single zeros elsewhere
        plane, _ = V.halves_variance(rec, grec)
        plane[np.random.default_rng(SRC_SEED).random((H, W)) < 0.05] = 0
        plane[8:16, 0:32] = 0
        for a in (acc, rec, gacc, grec, alpha, depth, plane):
            a.setflags(write=False)
        _memo["in"] = dict(acc=acc, rec=rec, gacc=gacc, grec=grec, a=alpha, d=depth, plane=plane)
    return _memo["in"]


def want_colour(F, NF, with_plane):
    """the restatement's answer, computed once and never changed; NF = 0: no feature"""
    key = ("colour", F, NF, with_plane)
    if key not in _memo:
        i = inputs()
        feats = [(i[p], c, s) for p, c, s in NF_LISTS[NF]] if NF else []
        out = V.denoise_var(i["acc"], i["rec"], i["plane"] if with_plane else None, R, F, K, feats, guide=i["gacc"], guide_rec=i["grec"])
        out.setflags(write=False)
        _memo[key] = out
    return _memo[key]


def test_the_image_has_what_the_rows_need():
    i = inputs()
    v, vg = D.variance(i["rec"]), D.variance(i["grec"])
    assert (W, H) == (40, 17) and W > FC.TILE_W and W % FC.TILE_W and H > 2 * FC.TILE_H and H % FC.TILE_H
    assert (v != 0).sum() > 400 and (vg != 0).sum() > 400 and (vg == 0).sum() > 20
    assert i["acc"].tobytes() != i["gacc"].tobytes()
    assert not i["plane"][8:16, 0:32].any() and (i["plane"] == 0).sum() > 256 + 10 and (i["plane"] != 0).sum() > 300
    assert np.isinf(i["d"][..., 1]).any() and np.isfinite(i["d"][..., 1]).any()


@pytest.mark.parametrize("row", COLOUR_ROWS, ids=row_id)
def test_colour_filter_instance_equals_the_restatement(vp, row):
    call, kernel, targs, with_plane = row
    F, NF = targs[0], (targs[1] if len(targs) > 1 else 0)
    assert (call == "vp_denoise_var") == with_plane and (kernel == "denoise_guided_tiled_k") == (NF > 0)
    i = inputs()
    dev = FC.Dev(vp)
    try:
        src, stats = dev.pair(i["acc"], i["rec"])
        guide, gstats = dev.pair(i["gacc"], i["grec"])
        planes = {"a": dev.put(i["a"]), "d": dev.put(i["d"])}
        plane = dev.put(i["plane"]) if with_plane else None
        feats = [(planes[p], c, s) for p, c, s in NF_LISTS[NF]] if NF else []
        dst = dev.out((H, W, 4))
        kw = dict(guide_ptr=guide, guide_stats_ptr=gstats)

        def run(features):
            if call == "vp_denoise":
                vp.denoise(dst.ptr, src, stats, W, H, R, F, K, **kw)
            elif call == "vp_denoise_guided":
                vp.denoise_guided(dst.ptr, src, stats, W, H, features, R, F, K, **kw)
            else:
                vp.denoise_var(dst.ptr, src, stats, W, H, plane, features, R, F, K, **kw)

        got, = FC.hold(vp, lambda: run(feats), [dst], [want_colour(F, NF, with_plane)], row_id(row))
        if with_plane:                                                # the zero block comes back as the plain mean
            c, _ = D.mean_image(i["acc"], i["rec"]["n"])
            assert got[8:16, 0:32, :3].tobytes() == c[8:16, 0:32].tobytes()
        if NF:
            # the feature-less call at the same (R, F): its own row holds it to the restatement, this row must differ from it
            dst.poison()
            run([])
            bare = dst.download()
            assert bare.tobytes() == want_colour(F, 0, with_plane).tobytes()
            assert got.tobytes() != bare.tobytes()
            for other in FEATURE_COUNTS:                              # ... and from every other feature count
                assert other == NF or got.tobytes() != want_colour(F, other, with_plane).tobytes(), other
        assert dev.untouched()
    finally:
        dev.free()


def variance_planes(kind):
    if ("uq", kind) not in _memo:
        u, q = V.planes(W, H, 300 + W, kind)
        u.setflags(write=False); q.setflags(write=False)
        _memo[("uq", kind)] = (u, q)
    return _memo[("uq", kind)]


@pytest.mark.parametrize("row", VARIANCE_ROWS, ids=row_id)
def test_variance_filter_instance_equals_the_restatement(vp, row):
    F = row[2][0]
    for kind in ("block", "isolated"):
        u, q = variance_planes(kind)
        assert (u == 0).sum() > 15 and (u != 0).sum() > 400
        key = ("var", kind, F)
        if key not in _memo:
            _memo[key] = V.filter_variance(u, q, R, F, K)
            _memo[key].setflags(write=False)
        dev = FC.Dev(vp)
        try:
            du, dq, dst = dev.put(u), dev.put(q), dev.out((H, W))
            got, = FC.hold(vp, lambda: vp.filter_variance(dst.ptr, du, dq, W, H, R, F, K), [dst], [_memo[key]], (row_id(row), kind))
            assert not got[u == 0].any() and (got != u).sum() > 300
            assert dev.untouched()
        finally:
            dev.free()


def select_inputs(kind):
    if ("sel", kind) not in _memo:
        imgs, errs = S.images_for(W, H, 4, 400 + W), S.error_planes(W, H, 4, 500 + W, kind)
        for a in imgs + errs:
            a.setflags(write=False)
        _memo[("sel", kind)] = (imgs, errs)
    return _memo[("sel", kind)]


@pytest.mark.parametrize("Rs,Rb", SELECT_RADII)
def test_select_with_every_candidate_count_equals_the_restatement(vp, Rs, Rb):
    """n = 3 beside 1, 2, 4, and a radius of 2: candidates are the LAST n of four, so that the block's winner is among them"""
    for kind in ("noise", "ties", "block"):
        imgs, errs = select_inputs(kind)
        dev = FC.Dev(vp)
        try:
            dimg, derr = [dev.put(a) for a in imgs], [dev.put(a) for a in errs]
            dst, idx = dev.out((H, W, 4)), dev.out((H, W), np.uint8)
            for n in (1, 2, 3, 4):
                key = ("select", kind, n, Rs, Rb)
                if key not in _memo:
                    _memo[key] = S.select(imgs[4 - n:], errs[4 - n:], Rs, Rb)
                want, want_k = _memo[key]
                if n > 1:
                    assert len(np.unique(want_k)) == n, (kind, n)               # every candidate wins somewhere
                if n > 1 and kind == "ties":
                    E = [S.smooth_error(e, Rs) for e in errs[4 - n:]]
                    assert ((E[0] == E[1]) & (want_k == 0)).sum() > 20 if n != 3 else ((E[1] == E[2]) & (want_k == 1)).sum() > 20
                FC.hold(vp, lambda: vp.select(dst.ptr, idx.ptr, dimg[4 - n:], derr[4 - n:], W, H, Rs, Rb), [dst, idx], [want, want_k],
                        ("vp_select", kind, n, Rs, Rb))
            assert dev.untouched()
        finally:
            dev.free()
