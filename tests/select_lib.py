"""What the selection tests share: the numpy restatement of include/volpath.h's vp_cross_error and vp_select,
and the pipeline of volpath.denoise_select.  A helper, not a test.

Written like variance_lib / halves_lib / denoise_lib, whose pieces it reuses: float32 arrays handled one operation at a time (numpy
rounds every operation to its dtype and contracts nothing), whole images one window offset at a time.  A position outside the image is
SKIPPED, as the definition says it: np.where keeps the running sum where the mask is false."""
import numpy as np

import adaptive_lib as A
import denoise_lib as D
import halves_lib as HL
import variance_lib as V

F32 = np.float32
MAX_CANDIDATES, MAX_RADIUS = 4, 3
TINY = F32(2.0 ** -137)       # error_planes(..., "tiny"): 49 values below 8 sum to less than 2^-126, the smallest normal number


def cross_error(fa, fb, h0, r0, h1, r1):
    """vp_cross_error: fa, fb (H, W, 4) float32 MEAN images of the filtered halves, (h0, r0), (h1, r1) accumulators and records"""
    fa, fb = np.asarray(fa, F32), np.asarray(fb, F32)
    c0, _ = D.mean_image(h0, r0["n"])
    c1, _ = D.mean_image(h1, r1["n"])
    y0, y1 = A.luminance(c0), A.luminance(c1)
    v0, v1 = D.variance(r0), D.variance(r1)
    with np.errstate(all="ignore"):
        da = A.luminance(fa) - y1
        ea = da * da - v1
        db = A.luminance(fb) - y0
        eb = db * db - v0
        err = F32(0.5) * (ea + eb)
    err = np.where((r0["n"] >= 2) & (r1["n"] >= 2), err, F32(0.0))
    assert err.dtype == F32
    return err


def _shifted(plane, R, dx, dy, fill):
    """plane at p + (dx, dy), `fill` where that leaves the image"""
    H, W = plane.shape
    pad = np.pad(plane, R, mode="constant", constant_values=fill)
    return pad[R + dy:R + dy + H, R + dx:R + dx + W]


def in_image(H, W, dx, dy):
    yy, xx = np.mgrid[0:H, 0:W]
    return (yy + dy >= 0) & (yy + dy < H) & (xx + dx >= 0) & (xx + dx < W)


def window_count(H, W, R):
    """the number of in-image positions of the (2R+1)^2 window of every pixel"""
    T = np.zeros((H, W), np.int64)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            T += in_image(H, W, dx, dy)
    return T


def smooth_error(err, Rs):
    """E_c of vp_select: row sums left to right from 0.0f, the rows top to bottom from 0.0f, one divide by the in-image count"""
    err = np.asarray(err, F32)
    H, W = err.shape
    S = np.zeros((H, W), F32)
    with np.errstate(all="ignore"):
        for ty in range(-Rs, Rs + 1):
            row = np.zeros((H, W), F32)
            for tx in range(-Rs, Rs + 1):
                row = np.where(in_image(H, W, tx, ty), row + _shifted(err, Rs, tx, ty, 0), row)
            S = np.where(in_image(H, W, 0, ty), S + row, S)
        E = S / window_count(H, W, Rs).astype(F32)
    assert E.dtype == F32
    return E


def pick(errors, Rs):
    """k(p): the lowest index of the smallest smoothed error"""
    E = [smooth_error(e, Rs) for e in errors]
    k = np.zeros(E[0].shape, np.uint8)
    best = E[0]
    for c in range(1, len(E)):
        lower = E[c] < best
        k = np.where(lower, np.uint8(c), k)
        best = np.where(lower, E[c], best)
    return k


def select(images, errors, Rs, Rb):
    """vp_select: (dst (H, W, 4) float32, index (H, W) uint8)"""
    images = [np.asarray(i, F32) for i in images]
    n = len(images)
    assert 1 <= n <= MAX_CANDIDATES and len(errors) == n and 0 <= Rs <= MAX_RADIUS and 0 <= Rb <= MAX_RADIUS
    H, W = images[0].shape[:2]
    k = pick(errors, Rs)
    Wc = np.zeros((n, H, W), np.int64)
    for dy in range(-Rb, Rb + 1):
        for dx in range(-Rb, Rb + 1):
            kq = _shifted(k.astype(np.int64), Rb, dx, dy, -1)
            for c in range(n):
                Wc[c] += kq == c
    T = window_count(H, W, Rb)
    assert (Wc.sum(0) == T).all()
    stack = np.stack(images)                                              # (n, H, W, 4)
    own = np.take_along_axis(stack, k[None, ..., None].astype(np.int64), 0)[0]
    Wk = np.take_along_axis(Wc, k[None].astype(np.int64), 0)[0]
    num = np.zeros((H, W, 3), F32)
    with np.errstate(all="ignore"):
        for c in range(n):
            num = num + Wc[c].astype(F32)[..., None] * images[c][..., :3]
        blend = num / T.astype(F32)[..., None]
    dst = own.copy()
    mixed = Wk != T
    dst[mixed, :3] = blend[mixed]
    assert dst.dtype == F32 and blend.dtype == F32
    return dst, k


def denoise_select(h0, r0, h1, r1, candidates=((5, 1, 0.45), (10, 3, 0.45)), smooth=1, blend=1, variance=(1, 3, 0.45), features=(), floor_y=1e-3):
    """volpath.denoise_select: the variance stage once, per candidate the two filtered halves, their error estimate and their merge, then
    the selection; returns a dict with dst, index, images, errors and the filtered variance plane uf"""
    u, q = V.halves_variance(r0, r1)
    uf = V.filter_variance(u, q, *variance)
    images, errors = [], []
    for R, Fp, k in candidates:
        fa = V.denoise_var(h0, r0, uf, R, Fp, k, features, guide=h1, guide_rec=r1)
        fb = V.denoise_var(h1, r1, uf, R, Fp, k, features, guide=h0, guide_rec=r0)
        errors.append(cross_error(fa, fb, h0, r0, h1, r1))
        images.append(HL.merge_halves(fa, r0, fb, r1, floor_y, want_resid=False)[0])
    dst, index = select(images, errors, smooth, blend)
    return dict(dst=dst, index=index, images=images, errors=errors, uf=uf)


def error_planes(W, H, n, seed, kind):
    """n synthetic error planes (H, W) float32.  kind "noise": normal values of both signs; "ties": values from a small set of dyadic
    numbers, so that whole windows sum to equal values in several candidates, and candidates 2 j and 2 j + 1 equal in the left half; "block":
    noise, with the last candidate far below the others in rows 0..23, columns 32..(whole tiles plus their halo of 6) -- clipped to the
    image -- so that it wins 32 x 8 tiles throughout; "tiny": the "ties" planes in the left half of the image and the "noise" planes in
    the right half, times TINY, a power of two that makes every value and every box sum of up to 7 x 7 of them subnormal or zero (the
    dyadic values stay exact, so ties stay ties; the noise keeps 12 bits or so)"""
    if kind == "tiny":
        ties, noise = error_planes(W, H, n, seed, "ties"), error_planes(W, H, n, seed, "noise")
        left = np.arange(W) < max(W // 2, 1)
        out = [np.ascontiguousarray(np.where(left, t, z) * TINY, F32) for t, z in zip(ties, noise)]
        assert all(p.dtype == F32 for p in out)
        return out
    rng = np.random.default_rng(seed)
    if kind == "ties":
        e = rng.choice(np.array([-0.5, -0.25, 0.0, 0.25, 0.5], F32), size=(n, H, W))
        for c in range(1, n, 2):
            e[c, :, :max(W // 2, 1)] = e[c - 1, :, :max(W // 2, 1)]
    else:
        e = rng.normal(0.0, 1.0, (n, H, W)).astype(F32)
        e[:, rng.random((H, W)) < 0.05] *= F32(1e-3)
    if kind == "block":
        e[n - 1, 0:30, 26:70] = F32(-100.0)
        e[n - 1, :min(H, 3), :min(W, 4)] = F32(-100.0)
    return [np.ascontiguousarray(p, F32) for p in e]


def images_for(W, H, n, seed):
    """n synthetic float4 mean images: candidates that differ, with a block of pixels on which all agree bit for bit"""
    rng = np.random.default_rng(seed)
    base = rng.uniform(0.0, 4.0, (H, W, 4)).astype(F32)
    out = []
    for c in range(n):
        img = (base * F32(1.0 + 0.1 * c) + rng.normal(0, 0.05, (H, W, 4)).astype(F32)).astype(F32)
        img[H // 3:H // 3 + max(H // 4, 1), W // 4:W // 4 + max(W // 3, 1)] = base[H // 3:H // 3 + max(H // 4, 1), W // 4:W // 4 + max(W // 3, 1)]
        out.append(np.ascontiguousarray(img))
    return out
