"""The cases of tests/test_filter_edges_gpu.py reach the edges they are named for, and the safe range that include/volpath.h states for
the colour filters and vp_cross_error is the one the definition has.  Everything here is the numpy restatement alone: conditions on the
inputs and on the reference's answers, no GPU."""
import hashlib
import os
import re

import numpy as np
import pytest

import adaptive_lib as A
import denoise_guided_lib as G
import denoise_lib as D
import filter_cases_lib as FC
import halves_lib as HL
import oracle_lib
import select_lib as S
import variance_lib as V
from test_denoise_cpu import records
from test_denoise_guided_gpu import NF_LISTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
K = 0.45
FLT_MAX = np.finfo(F32).max
COLOUR_CALLS = ((2, 1, 0.45), (5, 3, 2.0))


def finite(*arrays):
    return all(np.isfinite(a).all() for a in arrays)


def weights(acc, rec, R, F, k, guide=None, guide_rec=None):
    """(out, w, used): the restatement's answer, its weights (offsets in raster order, H, W) and which of them enter a sum: the offset
    stays inside the image and the pixel is filtered"""
    seen = []

    def expf(x):
        w = oracle_lib.math_array(1, x)
        seen.append(np.array(w, F32).reshape(rec.shape))
        return w
    kw = dict(guide=guide, guide_rec=guide_rec) if guide is not None else {}
    out = D.denoise(acc, rec, R, F, k, expf=expf, **kw)
    H, W = rec.shape
    filtered = D.variance(guide_rec if guide is not None else rec) != 0
    used = np.stack([S.in_image(H, W, ox, oy) & filtered for oy in range(-R, R + 1) for ox in range(-R, R + 1)])
    return out, np.stack(seen), used


def largest_squared_difference(acc, rec, R):
    """the largest d * d, binary32, over the pixel pairs of a window of radius R"""
    y = A.luminance(D.mean_image(acc, rec["n"])[0])
    H, W = y.shape
    yp = np.pad(y, R, mode="edge")
    with np.errstate(over="ignore"):
        return max(float(((y - yp[R + oy:R + oy + H, R + ox:R + ox + W]) ** 2).max()) for oy in range(-R, R + 1) for ox in range(-R, R + 1))


# ---- the generators' new keywords default to what they gave before
def test_new_keywords_default_to_the_old_bytes():
    def digest(*arrays):
        return hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)).hexdigest()[:16]
    for W, H, seed in ((70, 37, 170), (17, 9, 11)):
        assert digest(*D.synthetic(W, H, seed)) == digest(*D.synthetic(W, H, seed, scale=1.0, flat_rect=None))
    assert digest(*V.planes(70, 37, 370, "block")) == digest(*V.planes(70, 37, 370, "block", scale=1.0))
    # the bytes of the generators before the keywords existed
    assert digest(*D.synthetic(70, 37, 170)) == "68762771bc5f6c38"
    assert digest(*V.planes(70, 37, 370, "block")) == "274fede4bb8f3e58"
    assert digest(*S.error_planes(70, 37, 4, 570, "ties")) == "340fac312b7912f1"
    # scale: sum_y times c, sum_y2 times c * c, the colours times c; n, flags and the heat channel as they were
    (a1, r1), (a2, r2) = D.synthetic(9, 7, 5), D.synthetic(9, 7, 5, scale=0.25)       # a power of two: exact
    assert (r2["sum_y"] == r1["sum_y"] * 0.25).all() and (r2["sum_y2"] == r1["sum_y2"] * 0.0625).all()
    assert (a2[..., :3] == a1[..., :3] * F32(0.25)).all() and a2[..., 3].tobytes() == a1[..., 3].tobytes()
    assert r2["n"].tobytes() == r1["n"].tobytes() and r2["flags"].tobytes() == r1["flags"].tobytes()


# ---- part C: the colour filters' regimes
@pytest.mark.parametrize("regime", list(FC.REGIMES))
def test_a_colour_regime_reaches_its_edge(regime):
    W, H = FC.EDGE_W, FC.EDGE_H
    (h0, r0), (h1, r1) = FC.regime_pairs(regime)
    v0, v1 = D.variance(r0), D.variance(r1)
    mean = A.scale_by_count(h0, r0["n"], 1.0)
    sub, zero = int(FC.subnormal(v0).sum()), int((v0 == 0).sum())
    print("%s: %d subnormal and %d zero variances of %d; v up to %g; luminances up to %g" % (regime, sub, zero, W * H, v0.max(), A.luminance(mean).max()))
    between = {}
    for R, F, k in COLOUR_CALLS:
        for guide in (None, (h1, r1)):
            kw = dict(guide=guide[0], guide_rec=guide[1]) if guide else {}
            out, w, used = weights(h0, r0, R, F, k, **kw)
            assert finite(out), (regime, R, F, k)
            assert (out[..., :3] != mean[..., :3]).any(-1).sum() > 500
            between[(R, F, k, guide is not None)] = int(((w > 0) & (w < 1) & used).sum())
    print("    weights strictly between 0 and 1:", between)
    assert min(between.values()) >= 100
    k2 = F32(0.45) * F32(0.45)
    pair_sums = v0[:, :-1] + v0[:, 1:]                                     # v_a + v_b of horizontal neighbours
    dd = largest_squared_difference(h0, r0, 5)
    print("    largest d * d %g" % dd)
    if regime == "dark":
        # subnormal variances, variances that underflow to 0, and eps = 1e-20f carries every denominator -- also where v_a + v_b != 0
        assert sub >= 50 and zero >= 50
        flat_anyway = int((D.variance(FC.regime_pairs("normal")[0][1]) == 0).sum())
        assert zero > flat_anyway                                          # some are zero by underflow, not by flatness
        assert ((k2 * pair_sums < D.EPS) & (pair_sums > 0)).sum() > 100 and F32(4.0) * (v0.max() + v0.max()) < D.EPS
    if regime == "bright":
        assert 1e30 < dd < FLT_MAX and v0.max() > 1e34 and sub == 0
    if regime == "normal":
        assert sub == 0 and v0[v0 > 0].min() > 1e-20 and dd < 1e10                 # the control: nothing near either end
    # the other calls of the regime
    feats = [({"a": a, "d": d}[p], c, s) for (a, d) in [G.synthetic_features(W, H, 140)] for p, c, s in NF_LISTS[2]]
    assert finite(G.denoise_guided(h0, r0, feats, 5, 1, K))
    fa, fb = D.denoise(h0, r0, 2, 1, K, guide=h1, guide_rec=r1), D.denoise(h1, r1, 2, 1, K, guide=h0, guide_rec=r0)
    dst, resid = HL.merge_halves(fa, r0, fb, r1, float(F32(1e-3 * FC.REGIMES[regime])))
    err = S.cross_error(fa, fb, h0, r0, h1, r1)
    total = HL.accumulate_stats(r0, r1)
    assert finite(fa, fb, dst, resid, err, total["sum_y"], total["sum_y2"]) and (err < 0).any() and (err > 0).any()
    u, q = V.halves_variance(r0, r1)
    uf = V.filter_variance(u, q, 1, 3, K)
    assert finite(u, uf) and (uf != 0).sum() > 400
    assert finite(V.denoise_var(h0, r0, uf, 3, 1, K, guide=h1, guide_rec=r1))
    if regime == "bright":
        # u is a squared luminance of up to 1e35 here, and q, its square, is +inf by the definition: vp_halves_variance's one output
        # beyond binary32 in these regimes (the header's 3e9 for vp_filter_variance says as much).  The plane uf made from it is finite
        # and is only an input of vp_denoise_var's case
        assert np.isinf(q).any() and not np.isnan(q).any()
    else:
        assert finite(q)
    if regime == "dark":
        assert FC.subnormal(u).sum() > 50 and FC.subnormal(err).sum() + (err == 0).sum() > 50 and FC.subnormal(uf).sum() > 50


# ---- part C: vp_filter_variance's regimes
@pytest.mark.parametrize("regime", list(FC.VARIANCE_REGIMES))
def test_a_variance_regime_reaches_its_edge(regime):
    for kind in ("block", "isolated"):
        u, q = FC.regime_planes(regime, kind)
        print("%s %s: u %g .. %g, q %g .. %g; %d subnormal q, %d q == 0 where u != 0" % (
            regime, kind, u[u > 0].min(), u.max(), q[q > 0].min(), q.max(), FC.subnormal(q).sum(), ((q == 0) & (u != 0)).sum()))
        assert finite(u, q) and (u == 0).sum() > 15
        for R, F in ((1, 3), (10, 3)):
            out = V.filter_variance(u, q, R, F, K)
            assert finite(out) and (out != u).sum() > 250
        if regime == "dark":      # u 1e-26 .. 3e-9, q 1e-45 .. 1e-17: subnormal q, and q that underflows to 0 under a u that is not 0
            assert FC.subnormal(q).sum() > 100 and ((q == 0) & (u != 0)).sum() > 50 and u.max() < 1e-8 and q.max() < 1e-16
        if regime == "bright":    # u 1 .. 3e17, q 0.5 .. 1e35: inside the header's range (luminances to 5e8 of 3e9), near its end
            assert 1e17 < u.max() < 1e18 and 1e34 < q.max() < FLT_MAX and not FC.subnormal(q).any()


# ---- part C: vp_select on subnormal errors
@pytest.mark.parametrize("Rs", [3, 1])
def test_tiny_errors_are_subnormal_and_tie(Rs):
    errs = FC.tiny_errors()
    assert all((FC.subnormal(e) | (e == 0)).all() and FC.subnormal(e).sum() > 500 for e in errs)
    E = np.stack([S.smooth_error(e, Rs) for e in errs])
    assert (FC.subnormal(E) | (E == 0)).all() and FC.subnormal(E).sum() > 2000            # every smoothed error, too
    k = S.pick(errs, Rs)
    tied = (E == E.min(0)).sum(0) > 1                                                      # the smallest value is held by several
    assert tied.sum() > 20 and (k[tied] == np.argmax(E == E.min(0), 0)[tied]).all()        # ... and the lowest index has it
    assert len(np.unique(k)) >= 2
    # a power of two keeps the ties planes exact: scaled back they are the dyadic values they were
    left = FC.EDGE_W // 2
    back = errs[0][:, :left].astype(np.float64) / float(S.TINY)
    assert np.isin(back, [-0.5, -0.25, 0.0, 0.25, 0.5]).all()


# ---- part B: the flat block covers whole tiles of the launch grid
def test_the_flat_block_covers_whole_tiles_and_its_neighbours_read_it():
    W, H = FC.FLAT_TILE_SIZE
    y0, y1, x0, x1 = FC.FLAT_TILE_RECT
    acc, rec = FC.flat_tile_pair()
    v = D.variance(rec)
    assert not D.lhs_of(rec)[y0:y1, x0:x1].any() and not v[y0:y1, x0:x1].any()                 # lhs == 0 to the bit
    tiles = [(bx, by) for by in range(-(-H // FC.TILE_H)) for bx in range(-(-W // FC.TILE_W))
             if not v[by * FC.TILE_H:(by + 1) * FC.TILE_H, bx * FC.TILE_W:(bx + 1) * FC.TILE_W].any()]
    assert tiles == [(1, 1), (1, 2)]                                                            # whole tiles, with noisy ones all round
    assert y0 % FC.TILE_H == 0 and x0 % FC.TILE_W == 0 and y1 - y0 == 2 * FC.TILE_H and x1 - x0 == FC.TILE_W
    # today's block covers none (rows 12..20, columns 17..39)
    assert not any(not D.variance(D.synthetic(W, H, FC.FLAT_TILE_SEED)[1])[by * 8:by * 8 + 8, bx * 32:bx * 32 + 32].any() for by in range(4) for bx in range(2))
    # the neighbours' answers depend on the block: with other colours in it, the noisy pixels within R of it change
    out = D.denoise(acc, rec, 5, 2, K)
    other = acc.copy()
    other[y0:y1, x0:x1, :3] *= F32(1.5)
    moved = (D.denoise(other, rec, 5, 2, K)[..., :3] != out[..., :3]).any(-1)
    near = np.zeros((H, W), bool)
    near[y0 - 5:y1 + 5, x0 - 5:x1 + 5] = True
    near[y0:y1, x0:x1] = False
    near &= v != 0
    mean = A.scale_by_count(acc, rec["n"], 1.0)
    differs = (out[..., :3] != mean[..., :3]).any(-1)
    print("noisy pixels within 5 of the block: %d, %d of them differ from their mean, %d move with the block's colours" % (near.sum(), differs[near].sum(), moved[near].sum()))
    assert near.sum() > 300 and differs[near].sum() > 0.75 * near.sum() and moved[near].sum() > 0.5 * near.sum()
    assert out[y0:y1, x0:x1].tobytes() == mean[y0:y1, x0:x1].tobytes()


# ---- part D: where the finite contract of the colour filters and of vp_cross_error ends
def two_pixels(y, v, n=4):
    """a 2 x 1 pair: grey pixels of mean luminances y and variances of the mean v (binary64 records)"""
    rec = records(2, 1, n, np.array([y], np.float64), np.array([v], np.float64))
    acc = np.zeros((1, 2, 4), F32)
    acc[0, :, :3] = (np.array(y, np.float64) * n)[:, None]
    return acc, rec


def test_the_stated_safe_range_is_the_definitions():
    text = re.sub(r"\s*\n \*\s*", " ", open(os.path.join(ROOT, "include", "volpath.h")).read())      # comment lines joined
    assert "Inputs are assumed finite; then no NaN arises" not in text
    stated = re.findall(r"every variance of the mean at most ([0-9.e+]+) / max\(1, k2\)", text)
    assert len(stated) == 1 and float(stated[0]) == 1.7e38 and 2 * F32(1.7e38) <= FLT_MAX < 2 * F32(1.71e38)
    assert re.search(r"vp_cross_error:.*?variances of the mean up to 3\.4e38", text, re.S) and F32(3.4e38) <= FLT_MAX
    y = (1e18, 1.9e19)                                            # d * d = 3.24e38: finite, near the end
    with np.errstate(all="ignore"):
        # just inside: v_a + v_b = 3.4e38 is finite.  e = (3.24e38 - 3.4e38) / (1e-20 + k2 * 3.4e38) < 0: D = 0, weight 1, by the definition
        acc, rec = two_pixels(y, (1.7e38, 1.7e38))
        va = D.variance(rec)
        assert np.isfinite(va[0, 0] + va[0, 1])
        inside = D.denoise(acc, rec, 1, 0, 1.0)
        assert finite(inside)
        # inside with small variances the pair is told apart: e = 3.2e38 / 2e36 = 160, w = expf_(-160) = 0 to binary32 beside 1
        acc, rec = two_pixels(y, (1e36, 1e36))
        apart = D.denoise(acc, rec, 1, 0, 1.0)
        assert finite(apart) and apart.tobytes() == A.scale_by_count(acc, rec["n"], 1.0).tobytes()
        # d * d alone may overflow: e = +inf, w = 0 -- harmless
        acc, rec = two_pixels((1e18, 2.5e19), (1e36, 1e36))
        assert F32(2.4e19) * F32(2.4e19) == np.inf
        assert D.denoise(acc, rec, 1, 0, 1.0).tobytes() == A.scale_by_count(acc, rec["n"], 1.0).tobytes()
        # beyond: v_a + v_b = +inf.  The pair term is (finite - inf) / inf = NaN; the clamp at 0 makes D = 0 of it (NaN > 0 is false): no
        # NaN in dst, but two pixels that the same variances scaled into range tell apart (w = 0) are mixed with weight 1
        acc, rec = two_pixels(y, (1.8e38, 1.8e38))
        va = D.variance(rec)
        e = (F32(y[0]) - F32(y[1])) ** 2 - (va[0, 0] + va[0, 1])
        assert np.isinf(va[0, 0] + va[0, 1]) and np.isnan(e / (D.EPS + (va[0, 0] + va[0, 1])))
        beyond = D.denoise(acc, rec, 1, 0, 1.0)
        c = D.mean_image(acc, rec["n"])[0]
        assert finite(beyond) and beyond[0, 0, 0] == beyond[0, 1, 0] == (c[0, 0, 0] + c[0, 1, 0]) / F32(2)
        # vp_cross_error has no clamp: beyond its bound -- a variance of the mean that is +inf as binary32 -- it gives a NaN
        fa = fb = np.full((1, 2, 4), 1e18, F32)
        acc, rec = two_pixels(y, (3.4e38, 3.4e38))
        assert np.isfinite(D.variance(rec)).all() and not np.isnan(S.cross_error(fa, fb, acc, rec, acc, rec)).any()
        acc, rec = two_pixels((1e18, 2.5e19), (3.5e38, 3.5e38))
        assert np.isinf(D.variance(rec)).all()
        err = S.cross_error(fa, fb, acc, rec, acc, rec)
        assert np.isnan(err[0, 1]) and err[0, 0] == -np.inf          # inf - inf where d * d overflows too; -inf where it does not
