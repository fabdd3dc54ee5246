"""ctypes binding of oracle/_ref/libkernel_ref*.so: the reference's own kernel file and bound builder, compiled for the CPU
behind oracle/refshim (oracle/Makefile, target `ref`).  TEST-ONLY, CPU-only: no gpu-marked test may import this module.

Each library keeps ONE scene in file-scope symbols, as the reference does, and is not thread-safe: a RefScene is the scene of
its library only until the next RefScene of the same variant is made.
"""
import ctypes as C
import os

import numpy as np

from oracle_lib import Param  # param.h:4-12, the same 44 bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
REFERENCE = os.environ.get("VP_REFERENCE", "/root/reference")     # oracle/Makefile's REF
VARIANTS = ("", "_mis", "_scalar", "_multichannel")               # shipped; PASSIVE_ENVMAP 0; SPECTRAL_TRACKING 0; MULTI_CHANNEL 1
_LIBS = {}


def path(variant=""):
    return os.path.join(REF_DIR, f"libkernel_ref{variant}.so")


def status(variant=""):
    """'ok'; 'missing' = the reference tree is here but the library is not (a broken build: tests fail); 'absent' = neither is
    here (a machine without the reference: live comparisons skip, the committed fixtures still hold)"""
    if os.path.exists(path(variant)):
        return "ok"
    return "missing" if os.path.isdir(os.path.join(REFERENCE, "src")) else "absent"


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def lib(variant=""):
    if variant not in _LIBS:
        L = C.CDLL(path(variant))
        L.ref_init_volume.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        L.ref_render.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        for f in (L.ref_get_bounds, L.ref_get_opacity):
            f.restype, f.argtypes = C.c_size_t, [C.c_void_p]
        L.ref_get_env.restype, L.ref_get_env.argtypes = C.c_size_t, [C.c_int, C.c_void_p]
        L.ref_get_pdfnorm_alt.restype = C.c_float
        L.init_envmap.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.set_sun.argtypes = [C.c_void_p, C.c_void_p]
        L.precompute_opacity.argtypes = [C.c_void_p]
        L.copy_inv_view_matrix.argtypes = [C.c_void_p, C.c_size_t]
        L.scale.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_float]
        L.gamma_correct.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float]
        cfg = (C.c_int * 3)()
        L.ref_get_config(cfg)
        want = {"": (1, 1, 0), "_mis": (0, 1, 0), "_scalar": (1, 0, 0), "_multichannel": (1, 0, 1)}[variant]
        assert tuple(cfg) == want, (variant, tuple(cfg))
        _LIBS[variant] = L
    return _LIBS[variant]


class RefScene:
    """The arguments of oracle_lib.OracleScene, handed to the reference's own entry points (init_cuda, set_texture_filter_mode,
    init_envmap, set_sun, copy_inv_view_matrix)."""

    def __init__(self, grid, env, sun_dir, sun_power, box=None, linear=True, inv_view=None, variant=""):
        self.L = L = lib(variant)
        self.grid = np.ascontiguousarray(grid)
        if self.grid.dtype != np.uint8:
            self.grid = self.grid.astype(np.float32)
        self.shape = nz, ny, nx = self.grid.shape
        if box is None:
            lo = hi = None
        else:
            lo, hi = (np.asarray(b, np.float32) for b in box)
        L.ref_init_volume(_p(self.grid), nx, ny, nz, int(self.grid.dtype == np.uint8), None if lo is None else _p(lo),
                          None if hi is None else _p(hi), int(linear))
        self.env = np.ascontiguousarray(env, np.float32)
        L.init_envmap(_p(self.env), self.env.shape[1], self.env.shape[0])
        d, p = np.asarray(sun_dir, np.float32), np.asarray(sun_power, np.float32)
        L.set_sun(_p(d), _p(p))
        self.sun_dir = d
        if inv_view is None:
            import oracle_lib
            m = (C.c_float * 12)()
            oracle_lib.lib().vpo_default_camera(m)        # an input: the camera is the host's, not the kernel file's
            inv_view = np.array(m[:], np.float32)
        m = np.ascontiguousarray(np.asarray(inv_view, np.float32).ravel()[:12])
        L.copy_inv_view_matrix(_p(m), 48)
        self.has_opacity = False

    def precompute_opacity(self, light_dir=None):
        d = self.sun_dir if light_dir is None else np.asarray(light_dir, np.float32)
        self.L.precompute_opacity(_p(d))
        self.has_opacity = True
        return self.opacity()

    def opacity(self):
        out = np.empty(self.shape, np.float32)
        assert self.L.ref_get_opacity(_p(out)) == out.nbytes
        return out

    def bounds(self):
        out = np.empty(self.shape + (2,), self.grid.dtype)
        assert self.L.ref_get_bounds(_p(out)) == out.nbytes
        return out

    def render_frame(self, est, P, frame, accum=None):
        """est: oracle_lib.EST_*; accumulates as the kernels do"""
        assert est != 1 or frame <= 10 or self.has_opacity, "frames past 10 read the opacity table of the last precompute_opacity"
        if accum is None:
            accum = np.zeros((P.height, P.width, 4), np.float32)
        assert self.L.ref_render(est, _p(accum), frame, C.byref(P)) == 0
        return accum

    def env_tables(self):
        """pdfY, cdfY, pdfX, cdfX, HDRpdfnormAlt (only the PASSIVE_ENVMAP 0 build fills them)"""
        h, w = self.env.shape[:2]
        out = []
        for which, shape in ((1, (h,)), (2, (h,)), (3, (h, w)), (4, (h, w))):
            a = np.empty(shape, np.float32)
            assert self.L.ref_get_env(which, _p(a)) == a.nbytes
            out.append(a)
        return out + [np.float32(self.L.ref_get_pdfnorm_alt())]

    def sun(self):
        out = np.empty(9, np.float32)
        self.L.ref_get_sun(_p(out))
        return out[0:3], out[3:6], out[6:9]


def scale(src, s, variant=""):
    src = np.ascontiguousarray(src, np.float32)
    dst = np.empty_like(src)
    lib(variant).scale(_p(dst), _p(src), src.size // 4, s)
    return dst


def gamma_correct(src, s, gamma, variant=""):
    src = np.ascontiguousarray(src, np.float32)
    dst = np.empty_like(src)
    lib(variant).gamma_correct(_p(dst), _p(src), src.size // 4, s, gamma)
    return dst
