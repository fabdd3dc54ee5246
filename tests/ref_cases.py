"""The cases on which the reference's own kernel code (oracle/_ref/libkernel_ref*.so, tests/ref_lib.py) is held against the
oracle, and of which tests/golden/ref_kernel.npz keeps the reference-made results.  Every input is rebuilt from tests/scenes.py
and the few constants below, so the fixture stores results only.  This module imports neither the oracle, the reference libraries
nor the product: the functions that render a case take the binding module (oracle_lib / ref_lib) as an argument.

All cases run on the sampler.h stream with the dense (brick = 1) bound table: the reference has no other.
"""
import hashlib

import numpy as np

import degenerate_cases as DC
import long_ray_cases as LC
import scenes

EST_GLOBAL, EST_DECOMP, EST_BOUNDED = 0, 1, 2      # oracle_lib.EST_* / vp.EST_* / ref_render's `which`
EST_NAMES = {EST_GLOBAL: "global", EST_DECOMP: "decomp", EST_BOUNDED: "bounded"}
ALL_EST = (EST_DECOMP, EST_GLOBAL, EST_BOUNDED)
W, H = 32, 24

CHROMATIC = dict(g=0.5, albedo=(0.95, 0.8, 0.6), sigma_t=(1.0, 0.7, 0.45), density=120.0)   # chromatic and absorbing
USER_BOX = ((-0.3, -1.1, 0.2), (1.2, 0.4, 1.9))
# a camera that is not the default: to the side of and above the default box, rolled, looking past the centre (rows: right, up,
# -forward | position; the kernels take any 3x4 matrix)


def _camera():
    f = np.array([-0.62, -0.31, -0.72])
    f /= np.linalg.norm(f)
    r = np.cross(f, [0.15, 1.0, 0.05])
    r /= np.linalg.norm(r)
    u = np.cross(r, f)
    pos = np.array([2.1, 1.2, 2.6])
    return np.concatenate([np.stack([r, u, -f], 1), pos[:, None]], 1).astype(np.float32).ravel()


CAMERA = _camera()
# light directions for the optical-depth tables: together they leave the box through all six faces
LIGHTS = {"ppp": (0.48, 0.64, 0.6), "nnn": (-0.6, -0.48, -0.64), "sun": scenes.DEFAULT_SUN_DIR}


def soft_u8():
    """the soft, nowhere-empty volume of test_whatif_switches_are_live_on_a_soft_chromatic_volume: windows with positive minima"""
    rs = np.random.default_rng(5)
    g = rs.random((24, 24, 24), dtype=np.float32)
    for _ in range(2):
        g = (g + np.roll(g, 1, 0) + np.roll(g, 1, 1) + np.roll(g, 1, 2)) / 4.0
    return np.ascontiguousarray((40 + 215 * (g - g.min()) / (g.max() - g.min())).astype(np.uint8))


def ragged(quantized):
    """120 x 14 x 9, 60 % empty (the volume of test_gpu_bound_table_builder)"""
    rng = np.random.default_rng(11)
    g = rng.random((9, 14, 120), dtype=np.float32)
    g[rng.random(g.shape) < 0.6] = 0
    return (g * 255).astype(np.uint8) if quantized else g


def grid(name, oracle):
    if name.startswith("julia"):
        return oracle.julia(int(name[5:]))
    if name in ("odd_u8", "solid7"):
        return DC.grid(name, oracle)
    if name == "long_box":
        return LC.long_box()
    return {"blob_f32": scenes.blob_volume_f32, "blob_u8": scenes.blob_volume_u8, "soft_u8": soft_u8,
            "tiny": lambda: np.array([[[0, 255], [128, 7], [3, 90]]], np.uint8),           # nz = 1, ny = 3, nx = 2
            "solid16": lambda: np.full((16, 16, 16), 255, np.uint8),
            "ragged_u8": lambda: ragged(True), "ragged_f32": lambda: ragged(False)}[name]()


def env(name):
    e = scenes.synthetic_env()
    if name == "one_texel":
        return np.full((1, 1, 4), 0.25, np.float32)
    if name == "black_texel":
        e[3, 5, :3] = 0.0           # a zero-probability entry inside a row of the CDF
    elif name == "black_column":
        e[:, 0, :3] = 0.0           # a zero-probability FIRST entry of every row: a draw of exactly 0 samples a zero pdf
    else:
        assert name == "sky"
    return e


def _case(name, grid="julia32", env="sky", kw=None, preset=None, box=None, linear=True, cam=None, frames=(0, 1), est=ALL_EST,
          variant="", size=(W, H), golden=None, gframes=None, sun=scenes.DEFAULT_SUN_DIR):
    """golden: the estimators whose reference-made accumulators the fixture keeps (over gframes, default: frames)"""
    return dict(name=name, grid=grid, env=env, kw=kw or {}, preset=preset, box=box, linear=linear, cam=cam, frames=tuple(frames),
                est=tuple(est), variant=variant, size=size, golden=tuple(golden or ()), gframes=tuple(gframes or frames),
                sun=tuple(sun))


def _degenerate(name, grid, position, axis, sign, **kw):
    """a camera of tests/degenerate_cases.py at 16x12 in a medium thin enough that rays cross the volume (density 60)"""
    return _case(name, grid=grid, kw=dict(density=60.0), cam=DC.camera(grid, position, axis, sign), size=(DC.W, DC.H), **kw)


def _far(name, **kw):
    """a telephoto camera of tests/long_ray_cases.py, `name` units in front of the Julia box, at 16x12 in the medium of _degenerate"""
    return _case("far_" + name, grid=LC.FAR_GRID, kw=dict(density=60.0), cam=LC.far_camera(name), size=(DC.W, DC.H), frames=(0, 11), **kw)


# frames: 10 is the last that never reads the optical-depth table, 11 the first that may (spp > 10, kernel.cu:2183)
RENDERS = [
    _case("julia_default", frames=(0, 1, 10, 11, 12), golden=ALL_EST, gframes=(0, 1, 11, 12)),
    _case("preset1", preset=scenes.PRESET1, frames=(0, 1, 11, 12), golden=ALL_EST),
    _case("soft_f32_chromatic", grid="blob_f32", kw=CHROMATIC, frames=(0, 1, 11, 12), golden=ALL_EST),
    _case("blob_u8", grid="blob_u8", kw=dict(density=200.0), frames=(0, 11)),
    _case("soft_u8_chromatic", grid="soft_u8", kw=dict(density=40.0), preset=(2.29, 2.39, 1.97, 0.30, 0.34, 0.46), frames=(0, 12)),
    _case("point_filter", linear=False, frames=(0, 12), golden=(EST_DECOMP, EST_GLOBAL)),
    _case("user_box", box=USER_BOX, env="one_texel", frames=(0, 1, 12), golden=(EST_DECOMP,), gframes=(0, 12)),
    _case("camera", cam=CAMERA, frames=(0, 11)),
    _case("tiny_volume", grid="tiny", kw=dict(density=5.0), frames=(0, 1, 12)),
    _case("g_zero", kw=dict(g=0.0, albedo=(0.5, 0.7, 0.9), sigma_t=(1.0, 0.8, 0.6), density=300.0), frames=(0, 12)),
    _case("g_negative", kw=dict(g=-0.4), frames=(0, 12)),
    _case("density_zero", kw=dict(density=0.0), frames=(0, 12)),
    _case("brightness", kw=dict(brightness=2.5), frames=(1, 11)),
    # a solid, dense, non-absorbing block: paths run into max_depth = 800 (kernel.cu:34): heat 0.8 (segments) / 800 (scatters)
    _case("caps", grid="solid16", kw=dict(density=4000.0, g=0.0), frames=(0,), size=(24, 16), golden=(EST_DECOMP, EST_BOUNDED)),
    # degenerate geometry (tests/degenerate_cases.py): signed-permutation cameras whose centre row, column and pixel have exact zero
    # direction components, snapped to a face plane (inf * 0 = NaN in the slab test: fminf / fmaxf decide), a box edge, a face, a
    # cell-boundary plane of an odd grid and the box centre; axis-parallel suns
    _degenerate("deg_in_face_plane", "julia32", "in_face_plane", 0, 1, golden=ALL_EST),
    _degenerate("deg_along_edge", "julia32", "along_edge", 1, -1, golden=(EST_DECOMP, EST_GLOBAL)),
    _degenerate("deg_on_face", "julia32", "on_face", 2, 1),
    _degenerate("deg_in_cell_plane", "odd_u8", "in_cell_plane", 0, -1, golden=ALL_EST),
    _degenerate("deg_centre", "solid7", "centre", 1, 1),
    _degenerate("deg_sun_zenith", "julia32", "outside", 2, -1, sun=DC.SUNS["+y"], frames=(0, 11), golden=(EST_DECOMP, EST_GLOBAL)),
    _degenerate("deg_sun_x", "julia32", "outside", 0, 1, sun=DC.SUNS["+x"], frames=(0, 11)),
    # long rays (tests/long_ray_cases.py): the restart crawl in front of the box over 699 and over more than 700 segments of 0.05 (the
    # HIP path tabulates 700 of them per pixel and walks the rest), the bounded kernel's segment count running into max_depth = 800
    # on the way (from 38.5 units some paths arrive, from 41.5 none: heat 0.8, no radiance), and a box seven units long that is
    # empty between its ends (110 and more restart segments inside the box before the first brick that holds anything)
    _far("d34.97"),
    _far("d35.2", golden=(EST_DECOMP, EST_BOUNDED)),
    _far("d38.5"),
    _far("d41.5", golden=(EST_BOUNDED,)),
    _case("long_box", grid="long_box", box=LC.LONG_BOX, cam=LC.long_camera("axis"), frames=(0, 1, 11), golden=(EST_DECOMP,), gframes=(0, 11)),
]
VARIANT_RENDERS = [
    _case("mis_black_texel", env="black_texel", kw=dict(density=150.0, g=0.6), frames=(8, 12), variant="_mis", golden=ALL_EST),
    _case("mis_black_column", env="black_column", kw=dict(density=150.0, g=0.6), frames=(8, 12), variant="_mis"),
    _case("scalar", kw=dict(density=200.0, g=0.5, albedo=(0.9, 0.8, 0.7), sigma_t=(1.0, 0.7, 0.45)), frames=(8, 12),
          variant="_scalar", golden=ALL_EST),
    _case("multichannel", kw=dict(density=200.0, g=0.5, albedo=(0.9, 0.8, 0.7), sigma_t=(1.0, 0.7, 0.45)), frames=(8, 12),
          variant="_multichannel", golden=ALL_EST),
]
# (estimator, frame) at 64x48 on the black first column whose render takes the zero-pdf `continue` (kernel.cu:1540, :1900, :2266):
# found by scanning frames with the oracle's hit counter (vpo_debug_mis_zero_pdf), sampler.h stream
MIS_ZERO_PDF = [(EST_DECOMP, 2645), (EST_GLOBAL, 1513), (EST_BOUNDED, 771)]
BY_NAME = {c["name"]: c for c in RENDERS + VARIANT_RENDERS}
TRACK_OF_VARIANT = {"": 0, "_mis": 0, "_scalar": 1, "_multichannel": 2}


def needs_opacity(c, est, frames=None):
    """only the decomposition kernel reads the optical-depth table, and only past frame 10"""
    return est == EST_DECOMP and max(frames or c["frames"]) > 10


def param(make, mat, c):
    """make / mat: oracle_lib.default_param / oracle_lib.mat, or the product's make_param / mat"""
    P = make(c["size"][0], c["size"][1], **c["kw"])
    if c["preset"]:
        mat(P, *c["preset"])
    return P


def key(c, est):
    return f"{c['name']}/{EST_NAMES[est]}"


def oracle_scene(oracle, c, est):
    track = TRACK_OF_VARIANT[c["variant"]]
    return oracle.OracleScene(grid(c["grid"], oracle), env(c["env"]), c["sun"], scenes.DEFAULT_SUN_POWER, box=c["box"],
                              brick=1, linear=c["linear"], estimator=est, rng_mode=oracle.RNG_SAMPLERH, inv_view=c["cam"],
                              env_mis=c["variant"] == "_mis", track_mode=track)


def reference_scene(ref, oracle, c):
    """ref: tests/ref_lib.py; the oracle module supplies inputs only (the Julia voxels, the default camera)"""
    return ref.RefScene(grid(c["grid"], oracle), env(c["env"]), c["sun"], scenes.DEFAULT_SUN_POWER, box=c["box"],
                        linear=c["linear"], inv_view=c["cam"], variant=c["variant"])


def runs(frames):
    """(first, count) of each stretch of consecutive frames"""
    out = []
    for f in frames:
        if out and out[-1][0] + out[-1][1] == f:
            out[-1][1] += 1
        else:
            out.append([f, 1])
    return [tuple(r) for r in out]


class OracleBackend:
    """what the fixture's entries are, computed by oracle/vp_oracle.c"""

    def __init__(self, oracle):
        self.O = oracle

    def render(self, c, est, frames, each=False):
        """the accumulator after `frames` (each: a copy after every frame)"""
        sc = oracle_scene(self.O, c, est)
        if needs_opacity(c, est, frames):
            sc.precompute_opacity()
        P = param(self.O.default_param, self.O.mat, c)
        acc, out = None, []
        for f in frames:
            acc, _ = sc.render_frame(P, f, acc)
            out.append(acc.copy())
        return out if each else acc

    def bounds(self, g):
        g = grid(g, self.O)
        return self.O.bounds(g, self.O.bound_radius(g.shape[2]))

    def opacity(self, g, light):
        sc = self.O.OracleScene(grid(g, self.O), env("sky"), scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER)
        return sc.precompute_opacity(light_dir=LIGHTS[light])

    def env_tables(self, e):
        cdf_y, cdf_x, pdf_y, pdf_x, norm = self.O.env_tables_pdf(env(e))
        return dict(cdf_y=cdf_y, cdf_x=cdf_x, pdf_y=pdf_y, pdf_x=pdf_x, pdfnorm_alt=np.float32(norm))

    def sun_power(self):
        sc = self.O.OracleScene(grid("tiny", self.O), env("one_texel"), scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER)
        return np.array(sc.S.sun_power[:], np.float32)

    def scale(self, a, s):
        out = np.empty_like(a)
        self.O.lib().vpo_scale(out.ctypes.data, a.ctypes.data, a.size // 4, s)
        return out

    def gamma_correct(self, a, s, gamma):
        out = np.empty_like(a)
        self.O.lib().vpo_gamma_correct(out.ctypes.data, a.ctypes.data, a.size // 4, s, gamma)
        return out


class ReferenceBackend:
    """the same, computed by the reference's own code (oracle/_ref/libkernel_ref*.so): the authority"""

    def __init__(self, ref, oracle):
        self.R, self.O = ref, oracle

    def render(self, c, est, frames, each=False):
        sc = reference_scene(self.R, self.O, c)
        if needs_opacity(c, est, frames):
            sc.precompute_opacity()
        P = param(self.O.default_param, self.O.mat, c)
        acc, out = None, []
        for f in frames:
            acc = sc.render_frame(est, P, f, acc)
            out.append(acc.copy())
        return out if each else acc

    def _scene(self, g, e="sky", variant=""):
        return self.R.RefScene(grid(g, self.O), env(e), scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER, variant=variant)

    def bounds(self, g):
        return self._scene(g).bounds()

    def opacity(self, g, light):
        return self._scene(g).precompute_opacity(LIGHTS[light])

    def env_tables(self, e):
        pdf_y, cdf_y, pdf_x, cdf_x, norm = self._scene("tiny", e, "_mis").env_tables()
        return dict(cdf_y=cdf_y, cdf_x=cdf_x, pdf_y=pdf_y, pdf_x=pdf_x, pdfnorm_alt=np.float32(norm))

    def sun_power(self):
        return self._scene("tiny", "one_texel").sun()[1].copy()

    def scale(self, a, s):
        return self.R.scale(a, s)

    def gamma_correct(self, a, s, gamma):
        return self.R.gamma_correct(a, s, gamma)


BOUND_GRIDS = ("ragged_u8", "ragged_f32", "julia32", "julia64")
OPACITY_TABLES = [(g, l) for g in ("julia32", "ragged_u8") for l in ("ppp", "nnn", "sun")]
ENV_TABLES = ("sky", "black_texel", "black_column")
ENV_KEYS = ("cdf_y", "cdf_x", "pdf_y", "pdf_x", "pdfnorm_alt")


def entries(b):
    """(name, thunk) of every entry of tests/golden/ref_kernel.npz; a thunk computes its entry with backend `b` (None: a backend
    that cannot produce this entry)"""
    out = []
    for c in RENDERS + VARIANT_RENDERS:
        for est in c["golden"]:
            out.append((f"render/{key(c, est)}", lambda c=c, est=est: b.render(c, est, c["gframes"])))
    for g in BOUND_GRIDS:
        out.append((f"bounds/{g}", lambda g=g: b.bounds(g)))
    for g, l in OPACITY_TABLES:
        out.append((f"opacity/{g}/{l}", lambda g=g, l=l: b.opacity(g, l)))
    for e in ENV_TABLES:
        for k in ENV_KEYS:
            out.append((f"env/{e}/{k}", lambda e=e, k=k: b.env_tables(e).get(k)))
    out.append(("sun_power", lambda: b.sun_power()))
    out.append(("scale", lambda: b.scale(post_inputs(), POST["scale"])))
    out.append(("gamma_correct", lambda: b.gamma_correct(post_inputs(), POST["gamma_scale"], POST["gamma"])))
    return out


ENTRY_NAMES = [n for n, _ in entries(None)]


# ---- fixture entries: small arrays as they are, large tables as the digest of their bytes and every STRIDE-th element
RAW_LIMIT = 16384
STRIDE = 97


def pack(out, name, a):
    a = np.ascontiguousarray(a)
    if a.nbytes <= RAW_LIMIT:
        out[name] = a
    else:
        out[name + "#sha256"] = np.frombuffer(hashlib.sha256(a.tobytes()).digest(), np.uint8)
        out[name + "#sample"] = a.ravel()[::STRIDE].copy()
        out[name + "#shape"] = np.array(a.shape, np.int64)


def same(fix, name, a):
    """tobytes()-equality of `a` with the fixture's entry `name`"""
    a = np.ascontiguousarray(a)
    if name in fix:
        return a.dtype == fix[name].dtype and a.shape == fix[name].shape and a.tobytes() == fix[name].tobytes()
    return (a.dtype == fix[name + "#sample"].dtype and a.shape == tuple(fix[name + "#shape"]) and
            a.ravel()[::STRIDE].tobytes() == fix[name + "#sample"].tobytes() and
            hashlib.sha256(a.tobytes()).digest() == fix[name + "#sha256"].tobytes())


def post_inputs():
    """the accumulator handed to scale and gamma_correct: zeros, ones, tiny, large and negative-free random values"""
    rng = np.random.default_rng(17)
    a = (10.0 ** rng.uniform(-6, 4, (96, 4))).astype(np.float32)
    a[0, :] = 0.0
    a[1, :] = 1.0
    return a


POST = dict(scale=1.0 / 37.0, gamma_scale=1.0 / 12.0, gamma=2.2)
