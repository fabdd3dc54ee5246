"""What the variance-stage tests share: the numpy restatement of include/volpath.h's vp_halves_variance, vp_filter_variance and
vp_denoise_var, and the cross-filter with the stage.  A helper, not a test.

Written like denoise_lib / denoise_guided_lib, whose pieces it reuses: float32 arrays handled one operation at a time (numpy rounds
every operation to its dtype and contracts nothing), the oracle's expf_, whole images one offset at a time.  nlm() is the loop of
those two restatements with the guide's (y, v) and the colours handed in; test_variance_cpu.py holds it to them byte for byte."""
import numpy as np

import adaptive_lib as A
import denoise_guided_lib as G
import denoise_lib as D
import halves_lib as HL
import oracle_lib

F32 = np.float32
F64 = np.float64


def sample_variance(rec):
    """(u, measured): the unbiased per-sample luminance variance, binary64 rounded once to binary32; n < 2: not measured, 0"""
    nd = rec["n"].astype(F64)
    lhs = D.lhs_of(rec)
    with np.errstate(all="ignore"):
        u = (np.where(lhs > 0.0, lhs, 0.0) / (nd * (nd - 1.0))).astype(F32)
    measured = rec["n"] >= 2
    u[~measured] = 0
    return u, measured


def halves_variance(a_rec, b_rec):
    """vp_halves_variance: (u, q) float32, shaped like the records"""
    ua, ma = sample_variance(a_rec)
    ub, mb = sample_variance(b_rec)
    d = ua - ub
    u = np.where(ma & mb, F32(0.5) * (ua + ub), np.where(ma, ua, ub))      # (a half that is not measured carries 0)
    q = np.where(ma & mb, F32(0.25) * (d * d), u * u)
    assert u.dtype == F32 and q.dtype == F32
    return u, q


def nlm(y, v, c, radius, patch, k, features=(), expf=None):
    """the filter loop of vp_denoise / vp_denoise_guided on a guide's (y, v) planes and colours c (H, W, C): num / den per channel,
    with none of the exceptions; features as denoise_guided_lib takes them"""
    expf = expf or (lambda x: oracle_lib.math_array(1, x))
    y, v, c = np.asarray(y, F32), np.asarray(v, F32), np.asarray(c, F32)
    H, W = y.shape
    R, Fp = int(radius), int(patch)
    k2 = F32(k) * F32(k)
    h = R + Fp
    yp, vp_ = np.pad(y, h, mode="edge"), np.pad(v, h, mode="edge")     # clamp(): position q lives at [q + h]
    he, we = H + 2 * Fp, W + 2 * Fp
    ya, va = yp[R:R + he, R:R + we], vp_[R:R + he, R:R + we]
    inv_area = F32(1.0) / F32((2 * Fp + 1) * (2 * Fp + 1))
    den = np.zeros((H, W), F32)
    num = np.zeros(c.shape, F32)
    yy, xx = np.mgrid[0:H, 0:W]
    cp = np.pad(c, ((R, R), (R, R), (0, 0)), mode="edge")
    fa = [np.ascontiguousarray(np.asarray(p, F32)[..., ch]) for p, ch, _ in features]
    fp = [np.pad(f, R, mode="edge") for f in fa]
    g = [G.g_of(sg) for _, _, sg in features]
    with np.errstate(all="ignore"):
        for oy in range(-R, R + 1):
            for ox in range(-R, R + 1):
                yb, vb = yp[R + oy:R + oy + he, R + ox:R + ox + we], vp_[R + oy:R + oy + he, R + ox:R + ox + we]
                d = ya - yb
                e = (d * d - (va + np.where(vb < va, vb, va))) / (D.EPS + k2 * (va + vb))
                Dp = np.zeros((H, W), F32)
                for ty in range(2 * Fp + 1):
                    row = np.zeros((H, W), F32)
                    for tx in range(2 * Fp + 1):
                        row = row + e[ty:ty + H, tx:tx + W]
                    Dp = Dp + row
                Dp = Dp * inv_area
                Dp = np.where(Dp > 0, Dp, F32(0.0))
                if fa:
                    Df = np.zeros((H, W), F32)
                    for j in range(len(fa)):
                        fb = fp[j][R + oy:R + oy + H, R + ox:R + ox + W]
                        df = fa[j] - fb
                        Df = Df + np.where(fa[j] == fb, F32(0.0), (df * df) * g[j])
                    Dp = np.where(Df > Dp, Df, Dp)
                assert Dp.dtype == F32
                w = expf(-Dp).reshape(H, W)
                ok = (yy + oy >= 0) & (yy + oy < H) & (xx + ox >= 0) & (xx + ox < W)
                den = np.where(ok, den + w, den)
                num = np.where(ok[..., None], num + w[..., None] * cp[R + oy:R + oy + H, R + ox:R + ox + W], num)
        out = num / den[..., None]
    assert den.dtype == F32 and num.dtype == F32 and out.dtype == F32
    return out, den


def filter_variance(u, q, radius, patch, k, expf=None, want_den=False):
    """vp_filter_variance: y := u, v := q, the one colour c := u; u == 0 stays 0"""
    u, q = np.asarray(u, F32), np.asarray(q, F32)
    out, den = nlm(u, q, u[..., None], radius, patch, k, expf=expf)
    out = np.where(u == 0, F32(0.0), out[..., 0])
    assert out.dtype == F32
    return (out, den) if want_den else out


def denoise_var(src, rec, sample_var, radius, patch, k, features=(), guide=None, guide_rec=None, expf=None):
    """vp_denoise_var: vp_denoise_guided with the guide's v = sample_var * s, s the guide pair's 1 / n; sample_var None: that call"""
    assert (guide is None) == (guide_rec is None)
    if sample_var is None:
        return G.denoise_guided(src, rec, list(features), radius, patch, k, guide=guide, guide_rec=guide_rec, expf=expf)
    src = np.asarray(src, F32)
    c, s = D.mean_image(src, rec["n"])
    if guide is None:
        guide, guide_rec = src, rec
    gc, gs = D.mean_image(guide, guide_rec["n"])
    y = A.luminance(gc)
    v = np.asarray(sample_var, F32) * gs
    assert v.dtype == F32 and v.shape == y.shape
    rgb, _ = nlm(y, v, c, radius, patch, k, features, expf)
    out = np.empty(src.shape, F32)
    out[..., :3] = rgb
    flat = v == 0
    out[flat, :3] = c[flat]
    out[..., 3] = src[..., 3] * s
    return out


def denoise_cross_var(h0, r0, h1, r1, radius, patch, k, variance=(1, 3, 0.45), features=(), floor_y=1e-3):
    """the cross-filter with the variance stage: (dst, resid, A, B, filtered plane); variance (R, F, k) of the variance pass"""
    u, q = halves_variance(r0, r1)
    uf = filter_variance(u, q, *variance)
    fa = denoise_var(h0, r0, uf, radius, patch, k, features, guide=h1, guide_rec=r1)
    fb = denoise_var(h1, r1, uf, radius, patch, k, features, guide=h0, guide_rec=r0)
    dst, resid = HL.merge_halves(fa, r0, fb, r1, floor_y)
    return dst, resid, fa, fb, uf


def planes(W, H, seed, kind, scale=1.0):
    """(u, q) synthetic planes for vp_filter_variance, shaped like vp_halves_variance's output of a made-up pair of halves.
    kind "block": u == 0 in a block that covers the 32 x 8 tiles it can (rows 8..23, columns 32..95 clipped to the image; whole image
    rows 0.. at small sizes) plus noise elsewhere; kind "isolated": single zeros scattered inside noisy tiles.
    scale: denoise_lib.synthetic's, on the luminances of both halves -- u grows with its square and q with its fourth power"""
    rng = np.random.default_rng(seed)
    _, ra = D.synthetic(W, H, seed, flat_block=False, scale=scale)
    _, rb = D.synthetic(W, H, seed + 1000, flat_block=False, scale=scale)
    u, q = halves_variance(ra, rb)
    if kind == "block":
        u[8:24, 32:96] = 0
        u[:min(H, 3), :min(W, 5)] = 0
    else:
        u[rng.random((H, W)) < 0.1] = 0
    q = np.where(u == 0, F32(0.0), q)
    return np.ascontiguousarray(u, F32), np.ascontiguousarray(q, F32)
