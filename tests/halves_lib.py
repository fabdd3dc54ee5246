"""What the half-buffer tests share: the numpy restatement of include/volpath.h's vp_render_frames_halves_stats rule, vp_merge_halves
and vp_accumulate_stats, and the cross-filter built from denoise_lib / denoise_guided_lib.  A helper, not a test.

numpy rounds every operation to its dtype and contracts nothing, so float32 / float64 arrays handled one operation at a time carry the
definition's bits."""
import numpy as np

import adaptive_lib as A
import denoise_guided_lib as G
import denoise_lib as D

F32 = np.float32
F64 = np.float64


def half_of_frame(f, S=1):
    """h(f) = (f >> 2m) & 1, m = log2 S: blocks of S^2 consecutive frames alternate"""
    m = int(S).bit_length() - 1
    assert 1 << m == S
    return (int(f) >> (2 * m)) & 1


def frames_of_half(first, n, h, S=1):
    return [f for f in range(first, first + n) if half_of_frame(f, S) == h]


def runs_of_half(first, n, h, S=1):
    """the maximal runs (first frame, length) of consecutive frames of half h in [first, first + n)"""
    runs = []
    for f in frames_of_half(first, n, h, S):
        if runs and runs[-1][0] + runs[-1][1] == f:
            runs[-1][1] += 1
        else:
            runs.append([f, 1])
    return [tuple(r) for r in runs]


def render_halves(st0, st1, frame, first, n, S=1, owned=None):
    """vp_render_frames_halves_stats on two adaptive_lib.Stats: frame f goes to half h(f) alone, as a one-frame uniform render"""
    owned = A.all_pixels(st0.W, st0.H) if owned is None else owned
    for f in range(first, first + n):
        (st1 if half_of_frame(f, S) else st0).add_frame(frame(f), owned)
    return st0, st1


def merge_halves(a, a_rec, b, b_rec, floor_y=1e-3, want_resid=True):
    """vp_merge_halves: a, b (..., 4) float32 MEAN images, of the records only n is read; returns (dst, resid) -- resid None if not wanted"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    ua, ub = np.asarray(a_rec["n"]), np.asarray(b_rec["n"])
    na, nb = ua.astype(F32), ub.astype(F32)
    nt = na + nb
    with np.errstate(all="ignore"):
        dst = (a * na[..., None] + b * nb[..., None]) / nt[..., None]
    dst[nt == 0] = 0
    assert dst.dtype == F32
    if not want_resid:
        return dst, None
    fl = F32(floor_y)
    d = A.luminance(a) - A.luminance(b)
    e = F32(0.5) * np.abs(d)
    ym = A.luminance(dst)
    den = np.where(ym > fl, ym, fl)
    with np.errstate(all="ignore"):
        resid = e / den
    resid[(ua == 0) | (ub == 0)] = 0
    assert resid.dtype == F32
    return dst, resid


def accumulate_stats(dst, src):
    """vp_accumulate_stats on structured record arrays: a new array, dst + src"""
    out = dst.copy()
    out["sum_y"] = dst["sum_y"] + src["sum_y"]
    out["sum_y2"] = dst["sum_y2"] + src["sum_y2"]
    out["n"] = dst["n"] + src["n"]
    out["flags"] = dst["flags"] | src["flags"]
    assert out["sum_y"].dtype == F64
    return out


def denoise_cross(h0, r0, h1, r1, radius, patch, k, features=(), floor_y=1e-3):
    """the cross-filter: each half filtered with the other as guide, then merged; returns (dst, resid, A, B)"""
    feats = list(features)
    if feats:
        fa = G.denoise_guided(h0, r0, feats, radius, patch, k, guide=h1, guide_rec=r1)
        fb = G.denoise_guided(h1, r1, feats, radius, patch, k, guide=h0, guide_rec=r0)
    else:
        fa = D.denoise(h0, r0, radius, patch, k, guide=h1, guide_rec=r1)
        fb = D.denoise(h1, r1, radius, patch, k, guide=h0, guide_rec=r0)
    dst, resid = merge_halves(fa, r0, fb, r1, floor_y)
    return dst, resid, fa, fb


def prefill(W, H, seed):
    """(acc, rec) of a buffer that already holds something: finite floats of both signs with -0.0f, +0.0f and tiny values among them,
    records with non-zero sums, counts and flags"""
    rng = np.random.default_rng(seed)
    acc = rng.normal(0, 3, (H, W, 4)).astype(F32)
    pick = rng.integers(0, 4, (H, W, 4))
    acc[pick == 0] = F32(-0.0)
    acc[pick == 1] = F32(0.0)
    rec = np.zeros((H, W), np.dtype([("sum_y", F64), ("sum_y2", F64), ("n", np.uint32), ("flags", np.uint32)]))
    rec["n"] = rng.integers(0, 9, (H, W))
    rec["sum_y"] = rng.uniform(0, 4, (H, W)) * rec["n"]
    rec["sum_y2"] = rng.uniform(0, 9, (H, W)) * rec["n"]
    rec["flags"] = rng.integers(0, 4, (H, W))
    assert np.signbit(acc[acc == 0]).any() and (~np.signbit(acc[acc == 0])).any()
    return acc, rec
