"""What the denoiser tests share: the numpy restatement of include/volpath.h's vp_denoise.

numpy rounds every operation to its dtype and contracts nothing, so float32 arrays handled one operation at a time carry the
definition's bits; the exponential is the oracle's expf_ (oracle_lib.math_array(1, .)), the restatement of vp_math.h's.  The
restatement works on whole images, one offset at a time: the pair terms of the image plus an F halo, their row sums left to right,
the sum of the rows top to bottom, the weight, and the two running sums in raster order of the offsets."""
import numpy as np

import adaptive_lib as A
import oracle_lib

F32 = np.float32
F64 = np.float64
EPS = F32(1e-20)
MAX_RADIUS, MAX_PATCH = 10, 3


def mean_image(acc, n):
    """(c, s): c = A.xyz * s with s = 1.0f / (float)n, 0 where n == 0, and s itself (vp_scale_by_count's bits at scale 1)"""
    acc = np.asarray(acc, F32)
    with np.errstate(all="ignore"):
        s = F32(1.0) / n.astype(F32)
    s[n == 0] = 0
    c = acc[..., :3] * s[..., None]
    assert c.dtype == F32 and s.dtype == F32
    return c, s


def lhs_of(rec):
    nd = rec["n"].astype(F64)
    return nd * rec["sum_y2"] - rec["sum_y"] * rec["sum_y"]


def variance(rec):
    """variance of the mean luminance: binary64, rounded once to binary32; n < 2 gives 0"""
    nd = rec["n"].astype(F64)
    lhs = lhs_of(rec)
    with np.errstate(all="ignore"):
        v = (np.where(lhs > 0.0, lhs, 0.0) / (nd * nd * (nd - 1.0))).astype(F32)
    v[rec["n"] < 2] = 0
    return v


def denoise(src, rec, radius, patch, k, guide=None, guide_rec=None, expf=None):
    """vp_denoise: src (H, W, 4) float32 sums, rec (H, W) records; returns the (H, W, 4) float32 mean image"""
    assert (guide is None) == (guide_rec is None)
    expf = expf or (lambda x: oracle_lib.math_array(1, x))
    src = np.asarray(src, F32)
    H, W = src.shape[:2]
    R, Fp = int(radius), int(patch)
    c, s = mean_image(src, rec["n"])
    if guide is None:
        guide, guide_rec = src, rec
    gc, _ = mean_image(guide, guide_rec["n"])
    y = A.luminance(gc)
    v = variance(guide_rec)
    k2 = F32(k) * F32(k)
    h = R + Fp
    yp, vp_ = np.pad(y, h, mode="edge"), np.pad(v, h, mode="edge")     # clamp(): position q lives at [q + h]
    he, we = H + 2 * Fp, W + 2 * Fp                                     # the image plus an F halo
    ya, va = yp[R:R + he, R:R + we], vp_[R:R + he, R:R + we]
    inv_area = F32(1.0) / F32((2 * Fp + 1) * (2 * Fp + 1))
    den = np.zeros((H, W), F32)
    num = np.zeros((H, W, 3), F32)
    yy, xx = np.mgrid[0:H, 0:W]
    cp = np.pad(c, ((R, R), (R, R), (0, 0)), mode="edge")
    with np.errstate(all="ignore"):
        for oy in range(-R, R + 1):
            for ox in range(-R, R + 1):
                yb, vb = yp[R + oy:R + oy + he, R + ox:R + ox + we], vp_[R + oy:R + oy + he, R + ox:R + ox + we]
                d = ya - yb
                e = (d * d - (va + np.where(vb < va, vb, va))) / (EPS + k2 * (va + vb))
                D = np.zeros((H, W), F32)
                for ty in range(2 * Fp + 1):
                    row = np.zeros((H, W), F32)
                    for tx in range(2 * Fp + 1):
                        row = row + e[ty:ty + H, tx:tx + W]
                    D = D + row
                D = D * inv_area
                D = np.where(D > 0, D, F32(0.0))
                w = expf(-D).reshape(H, W)
                ok = (yy + oy >= 0) & (yy + oy < H) & (xx + ox >= 0) & (xx + ox < W)
                den = np.where(ok, den + w, den)
                num = np.where(ok[..., None], num + w[..., None] * cp[R + oy:R + oy + H, R + ox:R + ox + W], num)
        out = np.empty((H, W, 4), F32)
        out[..., :3] = num / den[..., None]
    flat = v == 0
    out[flat, :3] = c[flat]
    out[..., 3] = src[..., 3] * s
    assert den.dtype == F32 and num.dtype == F32
    return out


def rel_l2(img, ref):
    """relative L2 of the RGB channels, float64"""
    a, b = np.asarray(img, F64)[..., :3], np.asarray(ref, F64)[..., :3]
    return float(np.sqrt(((a - b) ** 2).sum() / (b ** 2).sum()))


def synthetic(W, H, seed, flat_block=True, scale=1.0, flat_rect=None):
    """(acc, records) of a made-up render: n in {0, 1, 2, ...}, luminances from 1e-4 to 5e4, a block of identical samples (v = 0),
    some FROZEN bits; the records are consistent with samples that could have been drawn (sum_y2 >= sum_y^2 / n up to rounding).
    scale c: every luminance and colour times c -- sum_y and the colours times c, sum_y2 times c * c, in binary64; 1.0 changes no bit.
    flat_rect (y0, y1, x0, x1): rows y0..y1-1, columns x0..x1-1 hold identical samples of dyadic luminances, lhs == 0 to the bit in
    EVERY pixel of it (the flat block's odd columns are only rounding-small) -- a block that can cover whole 32 x 8 tiles"""
    rng = np.random.default_rng(seed)
    n = rng.choice(np.array([0, 1, 2, 3, 5, 16, 64, 1000], np.uint32), size=(H, W), p=[0.04, 0.04, 0.3, 0.25, 0.2, 0.1, 0.04, 0.03])
    # mean luminance per pixel: a ramp over the whole range with 10 % texture (so that patches resemble each other and the weights
    # take every value between 0 and 1), and a few pixels anywhere in the range
    ramp = np.exp(np.log(1e-4) + (np.log(5e4) - np.log(1e-4)) * (np.add.outer(np.arange(H), np.arange(W)) / max(H + W - 2, 1)))
    level = np.where(rng.random((H, W)) < 0.97, ramp * np.exp(rng.normal(0, 0.1, (H, W))), np.exp(rng.uniform(np.log(1e-4), np.log(5e4), size=(H, W))))
    spread = rng.uniform(0.2, 1.5, size=(H, W))                                   # relative standard deviation of a sample
    if flat_block:
        by, bx = slice(H // 3, H // 3 + max(H // 4, 1)), slice(W // 4, W // 4 + max(W // 3, 1))
        spread[by, bx] = 0.0
        level[by, bx][:, ::2] = 0.5           # every other column exactly representable: lhs == 0 to the bit
    if flat_rect is not None:
        y0, y1, x0, x1 = flat_rect
        spread[y0:y1, x0:x1] = 0.0
        level[y0:y1, x0:x1] = (2.0 ** ((np.add.outer(np.arange(H), 2 * np.arange(W)) % 5) - 2))[y0:y1, x0:x1]      # 0.25 .. 4, all dyadic
    nd = n.astype(F64)
    rec = np.zeros((H, W), np.dtype([("sum_y", F64), ("sum_y2", F64), ("n", np.uint32), ("flags", np.uint32)]))
    rec["n"] = n
    rec["sum_y"] = nd * level
    rec["sum_y2"] = nd * level * level * (1.0 + spread * spread)
    flat = spread == 0.0                      # identical samples: lhs == 0, or rounding-small with either sign where level is not dyadic
    rec["sum_y2"][flat] = (rec["sum_y"] * rec["sum_y"] / np.maximum(nd, 1.0))[flat]
    rec["flags"] = (rng.random((H, W)) < 0.3).astype(np.uint32)
    tint = rng.uniform(0.5, 1.5, size=(H, W, 3))
    acc = np.empty((H, W, 4), F32)
    acc[..., :3] = ((nd * level)[..., None] * tint) * F64(scale)
    acc[..., 3] = rng.uniform(0, 50, size=(H, W)) * nd
    acc[n == 0] = 0
    rec["sum_y"] = rec["sum_y"] * F64(scale)
    rec["sum_y2"] = rec["sum_y2"] * (F64(scale) * F64(scale))
    return acc, rec
