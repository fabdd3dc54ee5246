"""Scenes and bit patterns of the density fetch's folded axis scale (csrc/vp_device.h fetch_scales), shared by
tests/test_fetch_fold_cpu.py and tests/test_fetch_fold_gpu.py.

The fetch forms the texel coordinate of an axis as fl(fl(s * linv) * n - 0.5), s = p - bmin.  Where linv is a power of two it takes
fl(s * (linv * n) - 0.5) instead: the same real number rounded once.  SCENES are the smallest volumes that reach every form."""
import numpy as np

f32, u32 = np.float32, np.uint32
W, H, FIRST, NFRAMES = 32, 24, 0, 8
KEY = (5, 6)


def _julia(oracle, shape):
    """a uchar grid [nz][ny][nx] cut from the 16^3 Julia set, so that every shape keeps part of the fractal's surface"""
    nz, ny, nx = shape
    g = oracle.julia(16)
    return np.ascontiguousarray(g[(16 - nz) // 2:(16 - nz) // 2 + nz, (16 - ny) // 2:(16 - ny) // 2 + ny, :nx])


# name -> (grid builder, box or None, linear, fold expected, axes expected to fold)
SCENES = {
    "cube16": (lambda o: _julia(o, (16, 16, 16)), None, True, 1, (1, 1, 1)),
    # extents 2, 1, 0.5: linv 0.5, 1, 2 -- three different powers of two, linv * n = 8 on every axis
    "slab16x8x4": (lambda o: _julia(o, (4, 8, 16)), None, True, 1, (1, 1, 1)),
    # extent 1.5 in y: linv = 2/3
    "y12": (lambda o: _julia(o, (16, 12, 16)), None, True, 0, (1, 0, 1)),
    # an explicit box of extent 1.6: no axis folds
    "box1.6": (lambda o: _julia(o, (16, 16, 16)), ((-0.7, -0.7, -0.7), (0.9, 0.9, 0.9)), True, 0, (0, 0, 0)),
    # float and binary16 volumes: the HOST's scales fold (the getter reports them), but their kernels are built without the folded
    # fetch and scale in two steps from linv and n -- the image tests pin that these volumes keep their bits beside the change
    "float16cube": (lambda o: o.cloud(16), None, True, 1, (1, 1, 1)),
    "half16cube": (lambda o: o.cloud(16).astype(np.float16), None, True, 1, (1, 1, 1)),
    # point sampling never folds: its product has no -0.5 behind it
    "point16": (lambda o: _julia(o, (16, 16, 16)), None, False, 0, (0, 0, 0)),
}
ESTIMATORS = {"global": 0, "decomp": 1}


def linv_of(grid, box):
    nz, ny, nx = grid.shape
    if box is None:
        lo = np.array([-1.0, -f32(ny) / f32(nx), -f32(nz) / f32(nx)], f32)
        hi = np.array([1.0, f32(ny) / f32(nx), f32(nz) / f32(nx)], f32)
    else:
        lo, hi = np.array(box[0], f32), np.array(box[1], f32)
    return (f32(1.0) / (hi - lo)).astype(f32), (nx, ny, nz)


def is_pow2(x):
    """the precondition on linv, restated on the bits: positive, normal, mantissa field 0"""
    b = int(np.array([x], f32).view(u32)[0])
    return (b & 0x007FFFFF) == 0 and 1 <= (b >> 23) <= 254


# ------------------------------------------------------------------------------------------------------------ bit patterns
def _straddle(x64):
    """the binary32 neighbours of real numbers: the nearest float and one step to either side"""
    c = np.asarray(x64, np.float64).astype(f32)
    return np.concatenate([c, np.nextafter(c, f32(-np.inf)), np.nextafter(c, f32(np.inf))]).view(u32)


def fixed_patterns():
    """+-0, the subnormals' ends and 2^-126, every exponent with mantissas 0, 1 and all-ones, +-inf and a NaN"""
    pos = [0x00000000, 0x00000001, 0x007FFFFF, 0x00800000, 0x7F800000, 0x7FC00000]
    for e in range(1, 255):
        pos += [e << 23, (e << 23) | 1, (e << 23) | 0x7FFFFF]
    pos = np.array(pos, u32)
    return np.concatenate([pos, pos | u32(0x80000000)])


def grid_patterns(n, linv, seed=3):
    """offsets s at which xb = s * linv * n - 0.5 straddles every texel centre (xb an integer) and the boundaries of the 8-bit
    weight (xb = c + (w + 0.5) / 256): every boundary of every cell for n <= 256; for n = 4096 every boundary of the two first, the
    two middle, the two last and 58 drawn cells"""
    scale = float(linv) * n
    centres = (np.arange(-1, n + 1, dtype=np.float64) + 0.5) / scale
    if n <= 256:
        cells = np.arange(n)
    else:
        rng = np.random.default_rng(seed)
        cells = np.unique(np.concatenate([[0, 1, n // 2 - 1, n // 2, n - 2, n - 1], rng.integers(0, n, 58)]))
    bounds = (cells[:, None] + (np.arange(256)[None, :] + 0.5) / 256.0 + 0.5).ravel() / scale
    return np.concatenate([_straddle(centres), _straddle(bounds)])
