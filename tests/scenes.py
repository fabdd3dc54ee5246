"""Small deterministic scenes shared by the parity tests (inputs only; no oracle, no product), and the seeded random scenes of the
randomised tests (random_case: the caller hands in the host module for the camera matrix)."""
import numpy as np

DEFAULT_SUN_DIR = (-0.0, 0.951057, -0.309017)          # SURVEY.md section 4 anchor, setup_sunsky(0.5, 0.2)
DEFAULT_SUN_POWER = (51797.34, 42480.11, 32578.49)     # sunColor * 0.02
PRESET1 = (2.29, 2.39, 1.97, 0.0030, 0.0034, 0.046)    # host.cpp:1296


def synthetic_env(w=64, h=32, seed=7):
    """A smooth-ish positive lat-long map; values of the order of the baked sky."""
    rng = np.random.default_rng(seed)
    env = np.zeros((h, w, 4), np.float32)
    yy = np.linspace(0, 1, h, dtype=np.float32)[:, None]
    base = np.stack([0.09 + 0.3 * (1 - yy), 0.12 + 0.3 * (1 - yy), 0.2 + 0.4 * (1 - yy)], -1)
    env[..., :3] = base + 0.05 * rng.random((h, w, 3), dtype=np.float32)
    env[..., 3] = 1.0
    return env


def blob_volume_f32(n=24, seed=3):
    """A float density volume in [0,1] with empty regions (for quantized=false paths)."""
    rng = np.random.default_rng(seed)
    z, y, x = np.mgrid[0:n, 0:n, 0:n].astype(np.float32)
    c = (n - 1) / 2
    r = np.sqrt((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2) / c
    v = np.clip(1.2 - r * 1.6, 0, 1) * (0.6 + 0.4 * rng.random((n, n, n), dtype=np.float32))
    v[r > 0.8] = 0
    return v.astype(np.float32)


def blob_volume_u8(n=24, seed=3):
    return (blob_volume_f32(n, seed) * 255.0).astype(np.uint8)


# ---- seeded random scenes (tests/test_fuzz_gpu.py against the oracle, tests/test_fuzz_fast_gpu.py in the fast arithmetic)
def random_volume(rng):
    kind = rng.integers(0, 5)
    if kind == 0:
        nz, ny, nx = (int(rng.integers(8, 33)) for _ in range(3))       # ragged, mostly empty with a few dense boxes
        g = np.zeros((nz, ny, nx), np.float32)
        for _ in range(int(rng.integers(1, 5))):
            z0, y0, x0 = (int(rng.integers(0, n)) for n in (nz, ny, nx))
            z1, y1, x1 = (int(min(n, a + rng.integers(1, 9))) for n, a in ((nz, z0), (ny, y0), (nx, x0)))
            g[z0:z1, y0:y1, x0:x1] = rng.random() * rng.random((z1 - z0, y1 - y0, x1 - x0), dtype=np.float32)
    elif kind == 1:
        n = int(rng.integers(16, 33))
        g = blob_volume_f32(n, seed=int(rng.integers(0, 1000)))
    elif kind == 2:
        nz, ny, nx = (int(rng.integers(6, 25)) for _ in range(3))       # nowhere empty: no pixel is "light"
        g = 0.05 + 0.95 * rng.random((nz, ny, nx), dtype=np.float32)
    elif kind == 3:
        nz, ny, nx = (int(rng.integers(12, 29)) for _ in range(3))      # a shell: empty inside and outside
        z, y, x = np.mgrid[0:nz, 0:ny, 0:nx].astype(np.float32)
        r = np.sqrt(((x - nx / 2) / nx) ** 2 + ((y - ny / 2) / ny) ** 2 + ((z - nz / 2) / nz) ** 2)
        g = ((r > 0.25) & (r < 0.4)).astype(np.float32) * rng.random((nz, ny, nx), dtype=np.float32)
    else:
        nz, ny, nx = (int(rng.integers(4, 21)) for _ in range(3))       # sparse single voxels
        g = (rng.random((nz, ny, nx)) < 0.02).astype(np.float32) * rng.random((nz, ny, nx), dtype=np.float32)
    if rng.random() < 0.6:
        return np.ascontiguousarray((g * 255.0).astype(np.uint8))
    return np.ascontiguousarray(g.astype(np.float32))


def random_camera(rng, host, centre, extent):
    """position on a shell around the box centre (sometimes inside the box), looking at a point near it (sometimes past it)"""
    d = rng.normal(size=3)
    d /= np.linalg.norm(d)
    radius = float(rng.choice([0.15, 0.6, 1.5, 3.0, 6.0])) * float(np.linalg.norm(extent))
    pos = centre + d * radius
    target = centre + rng.normal(size=3) * extent * float(rng.choice([0.1, 0.3, 0.5, 2.5], p=[0.4, 0.3, 0.2, 0.1]))
    fwd = target - pos
    fwd /= np.linalg.norm(fwd)
    up = np.cross(fwd, rng.normal(size=3))
    up /= np.linalg.norm(up)
    return host.camera_matrix(pos.astype(np.float32), fwd.astype(np.float32), up.astype(np.float32))


def random_case(seed, host):
    """everything a random scene consists of, from its seed"""
    rng = np.random.default_rng(1000 + seed)
    grid = random_volume(rng)
    nz, ny, nx = grid.shape
    if rng.random() < 0.5:
        box = None
        bmin, bmax = np.array([-1.0, -ny / nx, -nz / nx]), np.array([1.0, ny / nx, nz / nx])
    else:
        bmin = rng.uniform(-2.0, 0.5, 3)
        bmax = bmin + rng.uniform(0.3, 3.0, 3)
        box = (tuple(float(np.float32(v)) for v in bmin), tuple(float(np.float32(v)) for v in bmax))
    est = int(rng.integers(0, 3))
    rng_mode = int(rng.integers(0, 3))
    linear = bool(rng.random() < 0.75)
    brick = int(rng.choice([1, 2, 4, 8])) if est else 1
    W, H = int(rng.integers(3, 57)), int(rng.integers(3, 41))
    # optical thickness of the box diagonal at the volume's densest: 2 to ~600 mean free paths
    thickness = 10.0 ** rng.uniform(0.3, 2.8)
    scale = float(np.linalg.norm(bmax - bmin)) * max(float(grid.max()) / (255.0 if grid.dtype == np.uint8 else 1.0), 1e-3)
    kw = dict(density=float(np.float32(thickness / scale)), g=float(np.float32(rng.uniform(-0.9, 0.95))))
    if rng.random() < 0.6:
        kw["sigma_t"] = tuple(float(np.float32(v)) for v in rng.uniform(0.2, 1.0, 3))
        kw["albedo"] = tuple(float(np.float32(v)) for v in rng.uniform(0.3, 1.0, 3))
    sun = rng.normal(size=3)
    sun /= np.linalg.norm(sun)
    sun_dir = tuple(float(np.float32(v)) for v in sun)
    sun_power = tuple(float(np.float32(v)) for v in rng.uniform(0.0, 5.0e4, 3))
    env = synthetic_env(w=int(rng.integers(1, 40)), h=int(rng.integers(1, 20)), seed=seed)
    cam = random_camera(rng, host, (bmin + bmax) / 2, (bmax - bmin) / 2)
    key = (int(rng.integers(0, 2 ** 31)), int(rng.integers(0, 2 ** 31)))
    late = est == 1 and nx * ny * nz <= 16 ** 3 and rng.random() < 0.5     # across the frame-11 estimator switch (quirk Q5)
    first = 9 if late else int(rng.choice([0, 0, 3, 977, 123456]))
    nframes = 4 if late else int(rng.integers(1, 5))
    if est == 1 and not late and first + nframes - 1 > 10:
        first = 0
    # the reference's compiled-out builds: active environment sampling (one-sample MIS), scalar / multi-channel tracking
    build = rng.random()
    env_mis = bool(build < 0.15)
    track = int(rng.integers(1, 3)) if 0.15 <= build < 0.3 else 0
    if (env_mis or track) and rng_mode == 2:
        rng_mode = 1            # Philox2x32-7 is built for the shipped configuration only
    world = int(rng.choice([1, 1, 2, 3, 8]))
    return dict(grid=grid, box=box, est=est, rng_mode=rng_mode, linear=linear, brick=brick, W=W, H=H, kw=kw, sun_dir=sun_dir,
                sun_power=sun_power, env=env, cam=cam, key=key, late=late, first=first, nframes=nframes, env_mis=env_mis,
                track=track, world=world)
