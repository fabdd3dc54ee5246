"""Long rays, inputs only (no oracle, no product): cameras tens of units from the box seen through a telephoto matrix, and a box
seven units long that is empty but for its two ends.  Every number is an exact binary32 value.

Why these: three limits of the kernels lie beyond the reach of cameras within 15 units of a box with a diagonal of 5:
  * crawl_table_k ends the restart crawl in front of the box after 700 segments of 0.05 (35 units): from further away render_k,
    approach_local_k or the segment table go on OUTSIDE the box, and the bounded estimator starts its segment count at 700;
  * the bounded estimator's max_depth = 800 counts the crawl's segments (kernel.cu:1716): from 40 units away no path arrives;
  * approach_segments_k ends a pixel's chain of restart segments at record VP_SEG_CAP - 1 with the stop bit set, and
    approach_local_tab_k hands the sample over at that record's origin: 4.75 units of empty bricks inside the box (`long_box`), or
    a crawl that did not finish (the camera at 60 units).

Beside the inputs, numpy binary32 restatements, operation by operation, of the crawl (crawl_table_k) and of the chain
(approach_segments_k), on the restatement of intersect_box that tests/test_pins_gpu.py holds the kernel to, and a bound table handed in.
"""
import numpy as np

import degenerate_cases as DC
import scenes

f32 = np.float32
W, H = 32, 24
SEGMENT = f32(0.05)             # the restart segment (kernel.cu:1653)
CRAWL_CAP = 700                 # crawl_table_k's `segs < 700u`
MAX_DEPTH = 800                 # kernel.cu:34
# what `long_box` must offer a launch, per camera and brick size: general pixels whose chain of restart segments stops at the segment
# table's last record for no other reason, and general pixels whose chain stops earlier
MIN_CAPPED, MIN_EARLY = 50, 20
# the segment table's records per pixel where no library can be asked (tests/test_long_rays_cpu.py); tests/test_long_rays_gpu.py holds
# vp_get_segment_table's answer to it and makes its own census under the library's cap
SEG_CAP_ASSUMED = 96


# ---- shared with tests/test_pins_gpu.py: the camera ray and the slab test in float64, fminf / fmaxf on binary32
CAM = np.array([0.0, 0.207912, 0.978148, 3.922986, 0.0, 0.978148, -0.207912, -0.782739, -1.0, 0.0, 0.0, 0.03])  # H4


def camera_rays64(W, H, cam=None):
    """kernel.cu:1977-1987 in float64: origin and unit direction per pixel, arrays [H, W, 3]"""
    M = (CAM if cam is None else np.asarray(cam, np.float64)).reshape(3, 4)
    x = np.arange(W)[None, :].repeat(H, 0).astype(np.float64)
    y = np.arange(H)[:, None].repeat(W, 1).astype(np.float64)
    u = (x * 2 - W) / W
    v = (y * 2 - H) / W
    z = -1.0 / np.tan(54.43 * 0.00872664626)
    dv = np.stack([u, v, np.full_like(u, z)], -1)
    d = dv @ M[:, :3].T
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o = np.broadcast_to(M[:, 3], d.shape)
    return o, d


def slab64(o, d, bmin=-1.0, bmax=1.0):
    """intersectBox kernel.cu:654-680 in float64"""
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / d
        tb = inv * (bmin - o)
        tt = inv * (bmax - o)
    tmin = np.minimum(tt, tb).max(-1)
    tmax = np.maximum(tt, tb).min(-1)
    return (tmax > tmin) & (tmax >= 1e-3), tmin, tmax


def fmin32(a, b):
    """fminf on binary32: the operand that is not NaN (np.fmin); of two zeros the negative one -- the reference's device orders
    -0 below +0 in min and max (PTX ISA, min.f32 / max.f32), where C leaves the choice open"""
    r = np.fmin(a, b)
    return np.where((a == 0) & (b == 0), np.where(np.signbit(a) | np.signbit(b), np.float32(-0.0), np.float32(0.0)), r).astype(np.float32)


def fmax32(a, b):
    r = np.fmax(a, b)
    return np.where((a == 0) & (b == 0), np.where(np.signbit(a) & np.signbit(b), np.float32(-0.0), np.float32(0.0)), r).astype(np.float32)


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def telephoto(pos, fwd, up, zoom):
    """the 12 floats of inv_view (rows: right | up | -forward * zoom | position): camera_ray normalises u * col0 + v * col1 +
    cam_z * col2, so scaling the third column narrows the field of view by `zoom`"""
    f = _unit(fwd)
    r = _unit(np.cross(f, np.asarray(up, np.float64)))
    u = np.cross(r, f)
    m = np.concatenate([np.stack([r, u, -f * float(zoom)], 1), np.asarray(pos, np.float64)[:, None]], 1).astype(f32)
    return m.ravel()


# ---------------------------------------------------------------------------------------------------------------- far cameras
# Julia 32^3 in the default +-1 box, seen from the direction FAR_FROM (no exact zero direction component: that is
# tests/degenerate_cases.py' subject); the centre ray (pixel (W/2, H/2): u = v = 0) enters the box through the face z = 1 after
# `t_near` units.  zoom = distance / 3: the box covers the image from every distance.
FAR_FROM = _unit((0.06, 0.09, 1.0))
FAR = {"d34.97": 34.97,         # the crawl ends by itself after 699 segments
       "d35.2": 35.2,           # ... is cut at 700 with four segments to go
       "d38.5": 38.5,           # bounded estimator: some paths reach segment 800 inside the box
       "d41.5": 41.5,           # ... no path arrives: heat 0.8, no radiance
       "d60": 60.0}             # 1200 segments to the box: 700 crawled, 480 and more walked outside it; the chain's 96 records lie outside
FAR_GRID = "julia32"


def far_camera(name):
    t_near = FAR[name]
    distance = t_near + 1.0 / FAR_FROM[2]
    return telephoto(FAR_FROM * distance, -FAR_FROM, (0.0, 1.0, 0.0), distance / 3.0)


# ------------------------------------------------------------------------------------------------------------------- long_box
LONG_SHAPE = (32, 32, 112)                                  # nz, ny, nx
LONG_BOX = ((-3.5, -1.0, -1.0), (3.5, 1.0, 1.0))            # cubic cells of 0.0625
LONG_CAMERAS = {"axis": ((-7.5, 0.13, 0.07), (1.0, 0.0, 0.0), 2.0),
                "above": ((-5.0, 0.9, 0.6), (1.0, -0.16, -0.11), 1.5)}


def long_box(kind="u8"):
    """empty but for a blob in x-cells 96..111 (110 and more empty restart segments in front of it) and a small one without a zero
    voxel in x-cells 4..19 near the -x face, over a quarter of the cross-section (16^3: bricks of 8 with a positive minimum under
    the builder's radius of 3 + 1): camera rays that pass it are general pixels whose chains stop early -- in a brick with a positive
    minimum, or where they leave the box through a side face -- next to those that stop at the table's cap.
    kind: "u8", or "f32" / "f16" for the same grid with soft values (no segment table: approach_local_k walks)"""
    g = np.zeros(LONG_SHAPE, f32)
    g[:, :, 96:112] = scenes.blob_volume_f32(32, seed=3)[:, :, 8:24]
    g[4:20, 12:28, 4:20] = np.maximum(scenes.blob_volume_f32(16, seed=5), f32(0.25))
    if kind == "u8":
        return np.ascontiguousarray((g * 255.0).astype(np.uint8))
    if kind == "f16":
        return np.ascontiguousarray(g.astype(np.float16))
    assert kind == "f32"
    return np.ascontiguousarray(g)


def long_camera(name):
    pos, fwd, zoom = LONG_CAMERAS[name]
    return telephoto(pos, fwd, (0.0, 1.0, 0.0), zoom)


def box_of(box, shape):
    """(bmin, bmax) in binary32: `box`, or the default +-(1, ny/nx, nz/nx) of the shape (kernel.cu:373-378)"""
    if box is not None:
        return np.array(box[0], f32), np.array(box[1], f32)
    nz, ny, nx = shape
    hi = np.array([1.0, f32(ny) / f32(nx), f32(nz) / f32(nx)], f32)
    return -hi, hi


# ------------------------------------------------------------------------------------------------------------- restatements
class Geometry:
    """what the two walks read of a scene: the box, the grid's dimensions and the (max, min) bound table [bnz, bny, bnx, 2] of
    brick edge `brick` (uint8, or float32 for float volumes)"""

    def __init__(self, shape, box, bounds, brick):
        self.bmin, self.bmax = box_of(box, shape)
        self.linv = (f32(1.0) / (self.bmax - self.bmin)).astype(f32)          # kernel.cu:313
        self.n = np.array([shape[2], shape[1], shape[0]])
        self.bounds = np.asarray(bounds)
        self.shift = {1: 0, 2: 1, 4: 2, 8: 3}[brick]

    def intersect(self, o, inv):
        """intersect_box_inv (intersectBox kernel.cu:654-680 with 1 / d handed in): (hit, t_near, t_far)"""
        with np.errstate(all="ignore"):
            tbot, ttop = (inv * (self.bmin - o)).astype(f32), (inv * (self.bmax - o)).astype(f32)
            tmin, tmax = fmin32(ttop, tbot), fmax32(ttop, tbot)
            near = fmax32(fmax32(tmin[..., 0], tmin[..., 1]), tmin[..., 2])
            far = fmin32(fmin32(tmax[..., 0], tmax[..., 1]), tmax[..., 2])
            return (far > near) & (far >= f32(1e-3)), near, far

    def bound(self, pos):
        """sample_bound (vol_bound_minmax kernel.cu:1610-1624): the (max, min) entry of the brick that holds `pos`, point sampled
        and clamped"""
        p = ((pos - self.bmin).astype(f32) * self.linv).astype(f32)
        assert np.isfinite(p).all()
        idx = [np.clip(np.floor((p[..., a] * f32(self.n[a])).astype(f32)), 0, self.n[a] - 1).astype(np.int64) >> self.shift for a in range(3)]
        return self.bounds[idx[2], idx[1], idx[0]]


def segment_setup(geo, ro, d, inv):
    """segment_setup() of render_k (intersectSuperVolume kernel.cu:1626-1661) up to the bound fetch: hit, t_near clamped at 0,
    t_far = min(exit, 0.05), the bound entry at the point of entry"""
    hit, near, far = geo.intersect(ro, inv)
    t_near = fmax32(near, f32(0.0))
    t_far = fmin32(far, SEGMENT)
    return hit, t_near, t_far


def advance(ro, d, t):
    """origin += d * t (kernel.cu:2151-2155): a product and a sum, each rounded"""
    return (ro + (d * t[..., None]).astype(f32)).astype(f32)


def crawl(geo, inv_view, width, height, control_draw):
    """crawl_table_k per pixel: (origin [H, W, 3] the crawl ends at, segments, draws).  control_draw: the decomposition estimator
    with spectral tracking draws a control distance where the entry brick has a positive minimum"""
    o, d = DC.camera_rays(inv_view, width, height)
    ro = np.broadcast_to(o, d.shape).astype(f32)
    with np.errstate(divide="ignore"):
        inv = (f32(1.0) / d).astype(f32)
    segs = np.zeros(d.shape[:2], np.uint32)
    draws = np.zeros(d.shape[:2], np.uint32)
    go = np.ones(d.shape[:2], bool)
    for _ in range(CRAWL_CAP):
        hit, t_near, t_far = segment_setup(geo, ro, d, inv)
        go = go & hit & (t_near >= t_far)          # (a NaN ends the walk)
        if not go.any():
            break
        entry = np.where(go[..., None], advance(ro, d, t_near), geo.bmin)
        positive_min = geo.bound(entry)[..., 1] > 0
        draws += np.where(go, np.where(positive_min & bool(control_draw), 2, 1), 0).astype(np.uint32)
        segs += go
        ro = np.where(go[..., None], advance(ro, d, t_far), ro)
    return ro, segs, draws


STOP_MISS, STOP_MINIMUM, STOP_CAP = 1, 2, 4


def chain(geo, origin, d, t_empty, cap):
    """approach_segments_k for rays (origin [n, 3] where the crawl ended, d [n, 3], t_empty [n] the certified-empty distance left
    there) on a uchar bound table: records [n, cap, 4] (t_near, t_far, max byte | stop << 8 as the float of those bits, t_empty at
    the segment's start), origins [n, cap, 3], the number of records written [n] and why each chain stopped (STOP_* bits)"""
    assert geo.bounds.dtype == np.uint8
    n = len(origin)
    ro, t_empty = np.array(origin, f32), np.array(t_empty, f32)
    with np.errstate(divide="ignore"):
        inv = (f32(1.0) / d).astype(f32)
    rec = np.zeros((n, cap, 4), f32)
    org = np.zeros((n, cap, 3), f32)
    count = np.zeros(n, np.int64)
    why = np.zeros(n, np.int64)
    live = np.ones(n, bool)
    for k in range(cap):
        hit, t_near, t_far = segment_setup(geo, ro, d, inv)
        assert np.isfinite(t_near[live]).all() and np.isfinite(t_far[live]).all()
        b = geo.bound(np.where(live[:, None], advance(ro, d, t_near), geo.bmin))
        reason = np.where(~hit, STOP_MISS, 0) | np.where(b[:, 1] != 0, STOP_MINIMUM, 0) | (STOP_CAP if k == cap - 1 else 0)
        bits = (b[:, 0].astype(np.uint32) | np.where(reason != 0, 0x100, 0).astype(np.uint32)).view(f32)
        rec[live, k] = np.stack([t_near, t_far, bits, t_empty], 1)[live]
        org[live, k] = ro[live]
        count[live] = k + 1
        why[live] = reason[live]
        live = live & (reason == 0)
        ro = advance(ro, d, t_far)
        t_empty = (t_empty - t_far).astype(f32)
    assert not live.any()
    return rec, org, count, why


# ------------------------------------------------------------------------------------------------------ float64 geometry
def nonempty_cells(grid):
    """[nz, ny, nx] bool: a trilinear fetch in cell c = floor(p * N - 0.5) filters the clamped 2x2x2 texels from c on; the cell is
    non-empty when any of them is non-zero"""
    nz, ny, nx = grid.shape
    g = np.pad(np.asarray(grid) != 0, ((0, 1), (0, 1), (0, 1)), mode="edge")
    out = np.zeros(grid.shape, bool)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                out |= g[dz:dz + nz, dy:dy + ny, dx:dx + nx]
    return out


def cells_on_ray(cells, bmin, bmax, o, d, t0, t1):
    """the cells a float64 walk at 1/20 cell over [t0, t1) of the ray o + t d passes: bool per step"""
    nz, ny, nx = cells.shape
    n = np.array([nx, ny, nz])
    extent = np.asarray(bmax, np.float64) - np.asarray(bmin, np.float64)
    tt = np.arange(t0, t1, (extent / n).min() / 20)
    p = (o + d * tt[:, None] - np.asarray(bmin, np.float64)) / extent * n - 0.5
    idx = np.clip(np.floor(np.maximum(p, 0)).astype(int), 0, n - 1)
    return cells[idx[:, 2], idx[:, 1], idx[:, 0]]


def meets_medium(grid, box, inv_view, width, height):
    """[H, W] bool: the pixel's camera ray, walked in float64 at 1/20 cell over its chord of the box, passes a non-empty cell.  No
    sound certificate can call such a ray's chord empty: these pixels are general pixels (class 0) whatever else is"""
    bmin, bmax = box_of(box, grid.shape)
    o, d = camera_rays64(width, height, inv_view)
    hit, tmin, tmax = slab64(o, d, bmin.astype(np.float64), bmax.astype(np.float64))
    cells = nonempty_cells(grid)
    out = np.zeros((height, width), bool)
    for y, x in zip(*np.nonzero(hit & (tmax - tmin > 1e-4))):
        out[y, x] = cells_on_ray(cells, bmin, bmax, o[y, x], d[y, x], max(tmin[y, x], 0.0), tmax[y, x]).any()
    return out
