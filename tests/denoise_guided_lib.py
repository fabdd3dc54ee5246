"""What the guided-denoiser tests share: the numpy restatement of include/volpath.h's vp_denoise_guided.

denoise_lib.denoise, one offset at a time on whole images, with the one change of the header: the weight of an offset is
expf_(-max(Df, D)), Df the sum over the features of (fa - fb)^2 * g_j (0 where fa == fb, so that two equal infinities agree), g_j =
1 / ((2 sigma_j) sigma_j).  float32 arrays, one operation at a time.  Offsets that leave the image are skipped, so the padded
(clamped) feature values that numpy computes for them are never used.  Also the synthetic feature planes of the GPU tests."""
import numpy as np

import adaptive_lib as A
import denoise_lib as D
import oracle_lib

F32 = np.float32
MAX_FEATURES = 4


def g_of(sigma):
    """1.0f / ((2.0f * sigma) * sigma), binary32 at every step"""
    s = F32(sigma)
    with np.errstate(all="ignore"):
        return F32(1.0) / ((F32(2.0) * s) * s)


def denoise_guided(src, rec, features, radius, patch, k, guide=None, guide_rec=None, expf=None):
    """vp_denoise_guided: features is a sequence of (plane (H, W, 4) float32, channel, sigma); returns the (H, W, 4) mean image"""
    assert (guide is None) == (guide_rec is None) and len(features) <= MAX_FEATURES
    expf = expf or (lambda x: oracle_lib.math_array(1, x))
    src = np.asarray(src, F32)
    H, W = src.shape[:2]
    R, Fp = int(radius), int(patch)
    c, s = D.mean_image(src, rec["n"])
    if guide is None:
        guide, guide_rec = src, rec
    gc, _ = D.mean_image(guide, guide_rec["n"])
    y = A.luminance(gc)
    v = D.variance(guide_rec)
    k2 = F32(k) * F32(k)
    h = R + Fp
    yp, vp_ = np.pad(y, h, mode="edge"), np.pad(v, h, mode="edge")
    he, we = H + 2 * Fp, W + 2 * Fp
    ya, va = yp[R:R + he, R:R + we], vp_[R:R + he, R:R + we]
    inv_area = F32(1.0) / F32((2 * Fp + 1) * (2 * Fp + 1))
    den = np.zeros((H, W), F32)
    num = np.zeros((H, W, 3), F32)
    yy, xx = np.mgrid[0:H, 0:W]
    cp = np.pad(c, ((R, R), (R, R), (0, 0)), mode="edge")
    fa = [np.ascontiguousarray(np.asarray(p, F32)[..., ch]) for p, ch, _ in features]
    fp = [np.pad(f, R, mode="edge") for f in fa]
    g = [g_of(sg) for _, _, sg in features]
    assert all(f.shape == (H, W) for f in fa) and all(np.isfinite(x) and x > 0 for x in g)
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
                Df = np.zeros((H, W), F32)
                for j in range(len(fa)):
                    fb = fp[j][R + oy:R + oy + H, R + ox:R + ox + W]
                    df = fa[j] - fb
                    Df = Df + np.where(fa[j] == fb, F32(0.0), (df * df) * g[j])
                Dg = np.where(Df > Dp, Df, Dp)
                assert Dg.dtype == F32
                w = expf(-Dg).reshape(H, W)
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


def synthetic_features(W, H, seed):
    """(alpha, depth): two (H, W, 4) float32 planes shaped like vp_render_features' output.
    alpha.y: a [0, 1] ramp along x with a step edge (0.35 up) at 55 % of the width, and a little texture; alpha.x the ramp alone
    depth.y: a depth-like plane, finite 1..3 with a gentle slope, +inf in a region of about 30 % of the image that touches the left
             and the top border (a quarter disc round the corner); depth.x the same slope without the region
    depth.w: a 0/1 cover plane: 0 exactly where depth.y is +inf, and in a band of columns on the right"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    u = (xx / max(W - 1, 1)).astype(F32)
    ramp = (F32(0.6) * u).astype(F32)
    alpha = np.zeros((H, W, 4), F32)
    alpha[..., 0] = ramp
    alpha[..., 1] = np.clip(ramp + np.where(xx >= int(0.55 * W), F32(0.35), F32(0.0)) + rng.uniform(0, 0.05, (H, W)).astype(F32), 0, 1).astype(F32)
    alpha[..., 2] = rng.uniform(0, 1, (H, W)).astype(F32)
    alpha[..., 3] = rng.uniform(0, 4, (H, W)).astype(F32)
    depth = np.zeros((H, W, 4), F32)
    slope = (1.0 + 1.5 * u + 0.5 * (yy / max(H - 1, 1))).astype(F32)
    # a quarter ellipse round the corner (0, 0) with semi-axes (a W, a H): area pi a^2 / 4 of the image = 0.3 at a = 0.618
    hole = (xx / (0.618 * W)) ** 2 + (yy / (0.618 * H)) ** 2 < 1.0
    depth[..., 0] = slope
    depth[..., 1] = np.where(hole, F32(np.inf), slope)
    depth[..., 2] = slope + F32(0.25)
    depth[..., 3] = np.where(hole | (xx >= W - max(W // 6, 1)), F32(0.0), F32(1.0))
    return alpha, depth
