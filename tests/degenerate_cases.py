"""Degenerate geometry, inputs only (no oracle, no product): axis-parallel cameras and suns, cameras snapped to the faces, edges,
centre and cell-boundary planes of the box.  Every number is an exact binary32 value, so that "the ray lies IN the plane" is a
statement about the floats the kernels see: a zero direction component is exactly 0, an origin coordinate is exactly bmax.

Why these: a ray with a zero direction component has invR = +-inf in the slab test (kernel.cu:654-680); if its origin also lies in
that slab's plane, inv * (bmin - o) = inf * 0 = NaN and the answer rests on how fminf / fmaxf treat NaN.  A ray inside a cell plane
of the density grid has x * N - 0.5 an exact integer all along.  Axis directions tie or zero the class bits of the exit flights.

Cameras (rows of the 3x4 inv_view: right | up | -forward | position, as the kernels read it): view along axis `a` from the side
of sign `s`: forward = -s e_a, up = e_(a+1 mod 3), right = forward x up.  With an even image size column W/2 has u = 0, row H/2 has
v = 0 and pixel (W/2, H/2) has both: one resp. two exact zero direction components.
"""
import numpy as np

import scenes

f32 = np.float32
W, H = 16, 12                   # even: u = 0 at x = W/2, v = 0 at y = H/2
LONG_W, LONG_H = 8, 6           # the 64-frame launches
POSITIONS = ("outside", "on_face", "centre", "in_face_plane", "along_edge", "in_cell_plane")
VIEWS = tuple((a, s) for a in range(3) for s in (1, -1))
SUNS = {"+x": (1.0, 0.0, 0.0), "-x": (-1.0, 0.0, 0.0), "+y": (0.0, 1.0, 0.0), "-y": (0.0, -1.0, 0.0),
        "+z": (0.0, 0.0, 1.0), "-z": (0.0, 0.0, -1.0)}
# nz, ny, nx = 6, 16, 8 in a box of edges 2, 1, 0.75: cell edges 0.25, 0.0625, 0.125 -- a world diagonal (1, 1, 0) is (4, 16, 0) in
# cell units, so the dominant axis in cell units (y) is not the world's (a tie)
USER_BOX = ((-0.5, -1.0, 0.25), (1.5, 0.0, 1.0))
GRIDS = ("julia32", "odd_u8", "odd_f32", "solid7", "user_u8")


def grid(name, oracle):
    """oracle: the module that voxelises the Julia set (oracle_lib, or the product: the two are held equal elsewhere)"""
    if name.startswith("julia"):
        return oracle.julia(int(name[5:]))
    if name == "odd_u8":
        return np.ascontiguousarray(scenes.blob_volume_u8(13, seed=2)[:9, :11, :13])
    if name == "odd_f32":
        return np.ascontiguousarray(scenes.blob_volume_f32(13, seed=2)[:9, :11, :13])
    if name == "solid7":
        return np.full((7, 7, 7), 200, np.uint8)
    assert name == "user_u8"
    return np.ascontiguousarray(scenes.blob_volume_u8(16, seed=4)[4:10, :, 4:12])


SHAPES = {"julia32": (32, 32, 32), "julia48": (48, 48, 48), "odd_u8": (9, 11, 13), "odd_f32": (9, 11, 13), "solid7": (7, 7, 7), "user_u8": (6, 16, 8)}


def user_box(name):
    """the `box` argument of init_volume / OracleScene: None = the default box of the grid's shape"""
    return USER_BOX if name == "user_u8" else None


def box(name):
    """(bmin, bmax) as binary32 arrays: the user box, or the default +-(1, ny/nx, nz/nx) (kernel.cu:373-378, divided in binary32)"""
    if name == "user_u8":
        return np.array(USER_BOX[0], f32), np.array(USER_BOX[1], f32)
    nz, ny, nx = SHAPES[name]
    hi = np.array([1.0, f32(ny) / f32(nx), f32(nz) / f32(nx)], f32)
    return -hi, hi


def dims(name):
    nz, ny, nx = SHAPES[name]
    return np.array([nx, ny, nz])


def cell_coordinate(x, bmin, bmax, n):
    """x * N - 0.5 of the texture fetch along one axis, in binary32 as the kernels form it (normalised coordinate (x - bmin) *
    (1 / (bmax - bmin)), then one rounding of the scaling): an exact integer means `x` lies in a cell-boundary plane"""
    linv = f32(1.0) / f32(f32(bmax) - f32(bmin))
    p = f32(f32(f32(x) - f32(bmin)) * linv)
    return f32(np.float64(p) * n - 0.5)


def cell_plane_coordinate(bmin, bmax, n):
    """the coordinate of the cell-boundary plane nearest the middle of the box whose normalised coordinate (m + 0.5) / N is a binary
    fraction: the box centre for odd N, -0.03125 for N = 32 and -0.0625 for N = 48 in [-1, 1] (m = 15 and 22)"""
    m = (n - 1) // 2
    while ((2 * m + 1) * 2 ** 20) % (2 * n):
        m -= 1
    return f32(f32(bmin) + f32(f32(m + 0.5) / f32(n)) * f32(f32(bmax) - f32(bmin)))


def camera(name, position, axis, sign):
    """the 12 floats of inv_view for `position` (one of POSITIONS) in front of the box of grid `name`, looking along -sign * e_axis"""
    bmin, bmax = box(name)
    a, b, c = axis, (axis + 1) % 3, (axis + 2) % 3
    fwd = np.zeros(3, f32)
    fwd[a] = -sign
    up = np.zeros(3, f32)
    up[b] = 1.0
    right = np.cross(fwd, up).astype(f32)
    centre = ((bmin + bmax) * f32(0.5)).astype(f32)
    pos = centre.copy()
    pos[a] = centre[a] + f32(4.0 * sign)
    snap = bmax if sign > 0 else bmin           # views from the negative side snap to bmin: the NaN is then tbot's, not ttop's
    if position == "on_face":
        pos[a] = snap[a]
    elif position == "centre":
        pos[a] = centre[a]
    elif position == "in_face_plane":
        pos[b] = snap[b]                        # row H/2 (v = 0) lies in the face plane of axis b: the NaN slab
    elif position == "along_edge":
        pos[b], pos[c] = snap[b], snap[c]       # pixel (W/2, H/2) runs along a box edge
    elif position == "in_cell_plane":
        n = dims(name)
        pos[b] = cell_plane_coordinate(bmin[b], bmax[b], n[b])
        pos[c] = cell_plane_coordinate(bmin[c], bmax[c], n[c])
    else:
        assert position == "outside", position
    m = np.concatenate([np.stack([right, up, -fwd], 1), pos[:, None]], 1).astype(f32)
    assert set(np.unique(np.abs(m[:, :3]))) == {0.0, 1.0} and (np.abs(m[:, :3]).sum(0) == 1).all()
    return m.ravel()


def camera_rays(inv_view, width, height):
    """camera_ray (vp_oracle.c:829-840, kernel.cu:1977-1987) in numpy binary32, operation by operation: (origin[3], unit
    directions[H, W, 3])"""
    m = np.asarray(inv_view, f32).reshape(3, 4)
    x = np.arange(width, dtype=f32)[None, :].repeat(height, 0)
    y = np.arange(height, dtype=f32)[:, None].repeat(width, 1)
    u = (x * f32(2.0) - f32(width)) / f32(width)
    v = (y * f32(2.0) - f32(height)) / f32(width)
    cz = f32(-1.0 / np.tan(np.float64(f32(54.43)) * 0.00872664626))
    r = np.stack([(u * m[k, 0] + v * m[k, 1]) + cz * m[k, 2] for k in range(3)], -1).astype(f32)
    dot = (r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]) + r[..., 2] * r[..., 2]
    inv = f32(1.0) / np.sqrt(dot, dtype=f32)
    return m[:, 3].copy(), (r * inv[..., None]).astype(f32)


def ray_census(inv_view, width, height):
    """per pixel, the number of direction components that are exactly zero (+0 or -0): int array [H, W]"""
    _, d = camera_rays(inv_view, width, height)
    return (d == 0).sum(-1)
