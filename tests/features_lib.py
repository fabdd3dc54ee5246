"""The feature pass (include/volpath.h vp_render_features) restated in numpy binary32, operation by operation: the camera ray of
degenerate_cases.camera_rays, the oracle's box test (vpo_intersect_box), density fetch (vpo_sample_density) and exponential
(math_array(1, ...)).  Every intermediate is an np.float32; a ray's sum is np.cumsum in float32 (sequential, one rounding per step).
Needs no GPU and no product library."""
import ctypes as C

import numpy as np

import degenerate_cases as D

F32 = np.float32
INF = F32(np.inf)
TAU_Z_DEFAULT = F32(0.6931472)       # VP_FEATURE_TAU_Z_DEFAULT
MAX_STEPS = 1 << 20                  # VP_FEATURE_MAX_STEPS


def luminance_sigma(sigma_t):
    s = [F32(v) for v in sigma_t]
    return F32(F32(F32(F32(0.2126) * s[0]) + F32(F32(0.7152) * s[1])) + F32(F32(0.0722) * s[2]))


def box_tests(oracle, osc, width, height):
    """(ro[3], rd[H, W, 3], hit[H, W], tn[H, W], tf[H, W]): the camera rays of the scene's view and what intersect_box leaves for them
    (tn as the box test leaves it: not clamped)"""
    ro, rd = D.camera_rays(list(osc.S.inv_view), width, height)
    hit = np.zeros((height, width), bool)
    tn = np.zeros((height, width), F32)
    tf = np.zeros((height, width), F32)
    org = (C.c_float * 3)(*[float(v) for v in ro])
    a, b = C.c_float(), C.c_float()
    f = oracle.lib().vpo_intersect_box
    for y in range(height):
        for x in range(width):
            d = (C.c_float * 3)(*[float(v) for v in rd[y, x]])
            hit[y, x] = bool(f(org, d, osc.S.box_min, osc.S.box_max, C.byref(a), C.byref(b)))
            tn[y, x], tf[y, x] = a.value, b.value
    return ro, rd, hit, tn, tf


def march_ray(oracle, osc, ro, d, tn, tf, step, density, sigma_t, sy, tau_z):
    """one hit pixel: (alpha[4], depth[4], steps) by the definition's loop"""
    step, density, tau_z = F32(step), F32(density), F32(tau_z)
    tn = F32(tn) if tn > 0 else F32(0.0)                      # if (tn <= 0.0f) tn = 0.0f
    with np.errstate(over="ignore", invalid="ignore"):
        # t_k for every k that can come before the stop (t is monotone in k; the first k with !(t < tf) ends the march)
        n_max = int(min(max(float(F32(tf) - tn) / float(step), 0.0) + 4.0, float(1 << 24)))
        k = np.arange(n_max, dtype=np.float64).astype(F32)    # (float)k: exact below 2^24
        t = (tn + ((k + F32(0.5)) * step).astype(F32)).astype(F32)
        ok = t < F32(tf)
        n = int(np.argmin(ok)) if not ok.all() else n_max
        assert n < n_max, "the march did not stop inside the candidate range"
        t = t[:n]
        pos = (ro[None, :] + (d[None, :] * t[:, None]).astype(F32)).astype(F32)
        f, S = oracle.lib().vpo_sample_density, C.byref(osc.S)
        rho = np.array([f(S, (C.c_float * 3)(*p)) for p in pos.tolist()], F32).reshape(n)
        s = np.cumsum(rho, dtype=F32) if n else np.zeros(0, F32)
        zf = zt = zb = INF
        cover = F32(0.0)
        pos_idx = np.flatnonzero(rho > 0)
        if len(pos_idx):
            zf, zb, cover = t[pos_idx[0]], t[pos_idx[-1]], F32(1.0)
        reach = ((((s * step).astype(F32) * density).astype(F32)) * sy).astype(F32) >= tau_z
        if reach.any():
            zt = t[int(np.argmax(reach))]
        s_end = s[-1] if n else F32(0.0)
        tau = F32(F32(s_end * step) * density)
        x = np.array([-(F32(tau * F32(c))) for c in sigma_t], F32)
        alpha = np.empty(4, F32)
        alpha[:3] = F32(1.0) - oracle.math_array(1, x)
        alpha[3] = tau
    return alpha, np.array([zf, zt, zb, cover], F32), n


def features(oracle, osc, width, height, step, density, sigma_t, tau_z=TAU_Z_DEFAULT, pixels=None):
    """(alpha[H, W, 4], depth[H, W, 4], steps[H, W]) of the scene's view; pixels: an (H, W) bool mask of the pixels to compute (the
    others keep the miss constant and steps = -1)"""
    ro, rd, hit, tn, tf = box_tests(oracle, osc, width, height)
    sy = luminance_sigma(sigma_t)
    alpha = np.zeros((height, width, 4), F32)
    depth = np.empty((height, width, 4), F32)
    depth[...] = (INF, INF, INF, F32(0.0))
    steps = np.full((height, width), -1, np.int64)
    for y in range(height):
        for x in range(width):
            if pixels is not None and not pixels[y, x]:
                continue
            steps[y, x] = 0
            if hit[y, x]:
                alpha[y, x], depth[y, x], steps[y, x] = march_ray(oracle, osc, ro, rd[y, x], tn[y, x], tf[y, x], step, density, sigma_t, sy, tau_z)
    return alpha, depth, steps


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)
