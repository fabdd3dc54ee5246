"""What the output-stage filter tests of test_filter_instances_gpu.py and test_filter_edges_gpu.py share: device copies of host arrays
that remember their originals, the one way a call is held to its restatement, and the inputs of the edge cases.  A helper, not a test.

hold(): the call runs in both forms of the kernels (vp_set_denoise_form 1, then 0) into destinations filled with a NaN pattern (index
bytes: 0xA5); each form's outputs must be fully overwritten and tobytes()-equal to the restatement's; a mismatch names the first
differing pixel with its 32 x 8 tile and its lane there.  Dev.untouched(): every uploaded input downloaded again, byte for byte."""
import ctypes as C

import numpy as np

import denoise_lib as D
import select_lib as S
import variance_lib as V

F32 = np.float32
NAN_PATTERN = np.uint32(0x7FC12345)
INDEX_POISON = 0xA5
TILE_W, TILE_H = 32, 8
SMALLEST_NORMAL = np.finfo(F32).tiny


def subnormal(a):
    a = np.asarray(a, F32)
    return (a != 0) & (np.abs(a) < SMALLEST_NORMAL)


class Out:
    """a device destination of a shape and dtype (float32: planes and float4 images; uint8: the index map)"""

    def __init__(self, vp, shape, dtype=F32):
        self.vp, self.shape, self.dtype = vp, tuple(shape), np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        self.ptr = vp.lib().vp_malloc(max(self.nbytes, 4))
        assert self.ptr

    def poison(self):
        fill = np.full(self.shape, NAN_PATTERN, np.uint32).view(F32) if self.dtype == F32 else np.full(self.shape, INDEX_POISON, self.dtype)
        assert self.vp.lib().vp_upload(self.ptr, fill.ctypes.data_as(C.c_void_p), fill.nbytes) == 0

    def download(self):
        out = np.empty(self.shape, self.dtype)
        assert self.vp.lib().vp_download(out.ctypes.data_as(C.c_void_p), self.ptr, out.nbytes) == 0
        return out

    def overwritten(self, got):
        return not np.isnan(got).any() if self.dtype == F32 else bool((got != INDEX_POISON).all())


class Dev:
    """the device memory of one test: inputs (kept with the bytes they were uploaded from) and destinations, freed together"""

    def __init__(self, vp):
        self.vp, self.inputs, self.outs = vp, [], []

    def put(self, arr, dtype=None):
        """upload a host array (records: pass vp.PIXEL_STATS_DTYPE); returns the device pointer"""
        arr = np.ascontiguousarray(arr, dtype or arr.dtype)
        ptr = self.vp.lib().vp_malloc(max(arr.nbytes, 4))
        assert ptr
        assert self.vp.lib().vp_upload(ptr, arr.ctypes.data_as(C.c_void_p), arr.nbytes) == 0
        self.inputs.append((ptr, arr.tobytes()))
        return ptr

    def pair(self, acc, rec):
        return self.put(acc, F32), self.put(rec, self.vp.PIXEL_STATS_DTYPE)

    def out(self, shape, dtype=F32):
        self.outs.append(Out(self.vp, shape, dtype))
        return self.outs[-1]

    def untouched(self):
        for ptr, raw in self.inputs:
            back = np.empty(len(raw), np.uint8)
            assert self.vp.lib().vp_download(back.ctypes.data_as(C.c_void_p), ptr, len(raw)) == 0
            if back.tobytes() != raw:
                return False
        return True

    def free(self):
        for ptr, _ in self.inputs:
            self.vp.lib().vp_free(ptr)
        for o in self.outs:
            self.vp.lib().vp_free(o.ptr)
        self.inputs, self.outs = [], []


def first_difference(got, want):
    """where two (H, W[, C]) arrays first differ in raster order: the pixel, its tile and its lane in the tile's workgroup"""
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if g.shape != w.shape or g.dtype != w.dtype:
        return "shapes %s %s against %s %s" % (g.shape, g.dtype, w.shape, w.dtype)
    H, W = g.shape[:2]
    differs = (g.reshape(H, W, -1).view(np.uint8) != w.reshape(H, W, -1).view(np.uint8)).any(-1)
    if not differs.any():
        return "no difference"
    y, x = np.argwhere(differs)[0]
    return "%d of %d pixels differ, the first at (x %d, y %d): tile (%d, %d), lane %d of 256; got %s want %s" % (
        int(differs.sum()), H * W, x, y, x // TILE_W, y // TILE_H, (y % TILE_H) * TILE_W + x % TILE_W, g[y, x], w[y, x])


def hold(vp, call, outs, wants, what, pointwise=False):
    """run call() in both forms into the poisoned destinations `outs`; each must equal its restatement in `wants`.  Returns form 0's
    outputs.  pointwise: a call without forms (the kernels of vp_kernels.hip) -- it runs twice all the same"""
    got = {}
    try:
        for form in (1, 0):
            vp.set_denoise_form(form)
            for o in outs:
                o.poison()
            call()
            assert pointwise or vp.last_denoise_form() == form, what
            got[form] = [o.download() for o in outs]
            for o, g in zip(outs, got[form]):
                assert o.overwritten(g), (what, "form %d left poison behind" % form)
    finally:
        vp.set_denoise_form(0)
    for form, name in ((0, "tiled"), (1, "plain")):
        for g, w in zip(got[form], wants):
            assert g.tobytes() == np.ascontiguousarray(w).tobytes(), (what, name + " form", first_difference(g, w))
    return got[0]


# ---- the cases of test_filter_edges_gpu.py; test_filter_edges_cpu.py asserts on the restatement that each reaches its edge
EDGE_W, EDGE_H = 40, 17
# luminance scales of the colour filters' regimes (denoise_lib.synthetic's `scale`): variances of the mean go with the square
REGIMES = {"dark": 1e-17, "normal": 1.0, "bright": 1e13}
# ... and of vp_filter_variance's, whose u is a squared luminance and q a fourth power: bright stays inside the header's 3e9
VARIANCE_REGIMES = {"dark": 1e-9, "normal": 1.0, "bright": 1e4}
REGIME_SEEDS = (140, 141)
FLAT_TILE_SIZE, FLAT_TILE_SEED, FLAT_TILE_RECT = (70, 37), 170, (8, 24, 32, 64)      # rows 8..23, columns 32..63: two whole tiles

_cases = {}


def regime_pairs(regime):
    """((h0, r0), (h1, r1)): two synthetic pairs of one luminance scale, made once and read-only"""
    if regime not in _cases:
        pairs = tuple(D.synthetic(EDGE_W, EDGE_H, seed, scale=REGIMES[regime]) for seed in REGIME_SEEDS)
        for acc, rec in pairs:
            acc.setflags(write=False); rec.setflags(write=False)
        _cases[regime] = pairs
    return _cases[regime]


def regime_planes(regime, kind):
    key = ("uq", regime, kind)
    if key not in _cases:
        _cases[key] = V.planes(EDGE_W, EDGE_H, 340, kind, scale=VARIANCE_REGIMES[regime])
        for a in _cases[key]:
            a.setflags(write=False)
    return _cases[key]


def tiny_errors():
    if "tiny" not in _cases:
        _cases["tiny"] = S.error_planes(EDGE_W, EDGE_H, 4, 540, "tiny")
        for a in _cases["tiny"]:
            a.setflags(write=False)
    return _cases["tiny"]


def flat_tile_pair():
    if "flat" not in _cases:
        _cases["flat"] = D.synthetic(*FLAT_TILE_SIZE, FLAT_TILE_SEED, flat_rect=FLAT_TILE_RECT)
        for a in _cases["flat"]:
            a.setflags(write=False)
    return _cases["flat"]
