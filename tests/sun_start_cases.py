"""The sun shadow ray's constants (csrc/vp_device.h sun_row_fill, sun_start) restated in numpy binary32, shared by
tests/test_sun_start_cpu.py and tests/test_sun_start_gpu.py.

Every operation below is a single correctly rounded binary32 operation of numpy (no contraction, left to right), which is what
the exact translation unit computes; the fast unit differs in the root and the factor only, which nothing here predicts."""
import numpy as np

f32, u32 = np.float32, np.uint32

OBLIQUE = (0.48507127, 0.72760689, -0.48507127)
PLUS_ZERO = (0.0, 0.8, -0.6)
MINUS_ZERO = (-0.0, 0.8, -0.6)
TINY = (1.0e-8, 0.8, -0.6)
DEFAULT_BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))


def bench_sun():
    """the sun bench.py renders with: setup_sunsky(0.5, 0.2) baked by the host library"""
    from volpath import scene as vscene
    return tuple(float(v) for v in vscene.default_sunsky()[1])


def bits(x):
    return np.ascontiguousarray(x, f32).view(u32)


def far_end(sun):
    return np.asarray(sun, f32) * f32(1e10)


def dot(v):
    """dot(v, v) as vp_device.h evaluates it: (x x + y y) + z z"""
    v = np.asarray(v, f32)
    return (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]


def general(sun, ro):
    """start_shadow's set-up in the exact arithmetic for collision points ro [n, 3]: (dv, d2, len, r, sd, 1 / sd)"""
    with np.errstate(all="ignore"):
        dv = far_end(sun)[None, :] - np.asarray(ro, f32).reshape(-1, 3)
        d2 = dot(dv)
        ln = np.sqrt(d2)
        r = f32(1.0) / ln
        sd = dv * r[:, None]
        return dv, d2, ln, r, sd, f32(1.0) / sd


def row(sun):
    """the row's words in the exact arithmetic, by sun_row_fill's expressions: (E[3], D2, LEN, R, SD[3], IR[3])"""
    with np.errstate(all="ignore"):
        e = far_end(sun)
        d2 = dot(e)
        ln = np.sqrt(d2)
        r = f32(1.0) / ln
        sd = e * r
        return e, d2, ln, r, sd, f32(1.0) / sd


def taken(sun, ro):
    """the branches sun_start takes for the waves of 64 consecutive origins (the hook's eighth word), one value per origin: bit 0 =
    every lane's squared length has the row's bits, bits 1..3 = that and every lane's difference in x, y, z has the far end's"""
    e, d2_row = far_end(sun), dot(far_end(sun))
    with np.errstate(all="ignore"):
        dv, d2, *_ = general(sun, ro)
    n = dv.shape[0]
    out = np.zeros(n, u32)
    for w in range(0, n, 64):
        s = slice(w, min(w + 64, n))
        fc = bool((bits(d2[s]) == bits(d2_row)).all())
        t = 1 if fc else 0
        for c in range(3):
            if fc and bool((bits(dv[s, c]) == bits(e[c])).all()):
                t |= 2 << c
        out[s] = t
    return out
