"""Images past one scan chunk and at the 16-bit coordinate limit: the sizes, and the definition of the pixel lists restated in
vectorised numpy.  A helper, not a test (tests/test_large_images_cpu.py, tests/test_large_images_gpu.py).

The pixel lists are built on the GPU in padded slots of 64 per owned 8x8 tile; pixlist_scan_k scans the per-block class counts in
chunks of 1024 blocks of 1024 slots, so one chunk is exactly 2^20 padded slots.  The sizes below are the smallest that reach the
second chunk (L1), the third and fourth (L2), the largest coordinate a render call accepts in either half of y << 16 | x with 8192
tiles in a row (L3) or 8192 tile rows (L4), and the sub-pixel limit S W = 65536 (L5).  The scene is the suite's small one (Julia-32,
scenes.synthetic_env(), default sun and camera): the cost is in the pixels, not in the medium."""
import numpy as np

from long_ray_cases import CAM, slab64
from volpath import dist as vd

TILE = 8
SCAN_BLOCK = 1024                 # VP_PIXLIST_BLOCK: slots per block, and blocks per chunk of pixlist_scan_k
CHUNK_SLOTS = SCAN_BLOCK * SCAN_BLOCK
EDGE = 1 << 20                    # the list slot at which the second chunk of a world = 1 list begins, were no slot padding

# name -> (W, H, S)
SIZES = {"L1": (1100, 1000, 1), "L2": (2560, 1440, 1), "L3": (65535, 17, 1), "L4": (17, 65535, 1), "L5": (32768, 40, 2)}
# what the issue counted under the default camera with the float64 slab test: (box-hitting, box-missing) rays
COUNTED = {"L1": (489283, 610717), "L3": (724965, 389130), "L4": (121, 1113974)}
MIN_PER_KIND = 100


def scan_blocks(W, H, rank=0, world=1):
    """blocks of SCAN_BLOCK padded slots that the pixel lists of this shard are built from (vp_tables.cpp pixel_list_blocks)"""
    owned = len(vd.owned_tiles(rank, world, W, H))
    return (owned * TILE * TILE + SCAN_BLOCK - 1) // SCAN_BLOCK


def scan_chunks(W, H, rank=0, world=1):
    return (scan_blocks(W, H, rank, world) + SCAN_BLOCK - 1) // SCAN_BLOCK


def box_hits(W, H, S=1):
    """(H, W) int: how many of the S x S camera rays of each pixel hit the default box, by the float64 slab test on the float64
    camera rays of the S W x S H image (tests/test_pins_gpu.py holds the kernels to both); computed in bands of fine rows"""
    fw, fh = W * S, H * S
    out = np.zeros((H, W), np.int64)
    band = max(S, (1 << 21) // fw // S * S)
    for y0 in range(0, fh, band):
        y1 = min(fh, y0 + band)
        hit = _hits_rows(fw, fh, y0, y1)
        out[y0 // S:y1 // S] += hit.reshape((y1 - y0) // S, S, W, S).sum(axis=(1, 3))
    return out


def _hits_rows(W, H, y0, y1):
    """long_ray_cases.camera_rays64 + slab64 for the rows y0 .. y1-1 of a W x H image: the same float64 operations, a band at a time
    (tests/test_large_images_cpu.py holds the two against each other)"""
    M = CAM.reshape(3, 4)
    x = np.arange(W)[None, :].repeat(y1 - y0, 0).astype(np.float64)
    y = np.arange(y0, y1)[:, None].repeat(W, 1).astype(np.float64)
    u = (x * 2 - W) / W
    v = (y * 2 - H) / W
    z = -1.0 / np.tan(54.43 * 0.00872664626)
    d = np.stack([u, v, np.full_like(u, z)], -1) @ M[:, :3].T
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return slab64(np.broadcast_to(M[:, 3], d.shape), d)[0]


def tile_order(W, H, rank=0, world=1):
    """(y, x) of the rank's pixels in the order the lists are partitioned from: its 8x8 tiles row-major (volpath.dist.owned_tiles),
    the pixels row-major within a tile, the edge tiles clipped to the image"""
    tiles_x, _ = vd.tile_grid(W, H)
    t = vd.owned_tiles(rank, world, W, H).astype(np.int64)
    ty, tx = t // tiles_x, t % tiles_x
    r = np.arange(TILE, dtype=np.int64)
    y = np.broadcast_to(ty[:, None, None] * TILE + r[None, :, None], (len(t), TILE, TILE)).ravel()
    x = np.broadcast_to(tx[:, None, None] * TILE + r[None, None, :], (len(t), TILE, TILE)).ravel()
    keep = (x < W) & (y < H)
    return y[keep], x[keep]


def pixel_lists(cls, rank=0, world=1):
    """the three lists (general, light, misses the box) of y << 16 | x that the class image cls (H, W; values 0, 1, 2) defines for
    the rank: the stable partition of tile_order by class"""
    H, W = cls.shape
    y, x = tile_order(W, H, rank, world)
    c = np.asarray(cls)[y, x]
    pix = (y << 16 | x).astype(np.uint32)
    return [pix[c == k] for k in range(3)]


def unpack(pix):
    """(y, x) of list entries"""
    pix = np.asarray(pix, np.uint32)
    return (pix >> 16).astype(np.int64), (pix & 0xffff).astype(np.int64)


def class_ranges(lists):
    """[(first slot, end slot)] of the three classes in the concatenated list"""
    n = np.cumsum([0] + [len(l) for l in lists])
    return [(int(n[k]), int(n[k + 1])) for k in range(3)]


def chunk_report(lists):
    """which 2^20-slot stretch of the concatenated list each class boundary falls in, and which classes hold slot 2^20"""
    rg = class_ranges(lists)
    return {"counts": [b - a for a, b in rg], "boundary_chunk": [a // EDGE for a, _ in rg] + [rg[2][1] // EDGE],
            "classes_crossing_2^20": [k for k, (a, b) in enumerate(rg) if a < EDGE < b]}


def edge_slots(lists, rng, n_random=200):
    """slots of the concatenated list worth a look, per class: its first and last entry, the entries at slots 2^20 - 1, 2^20 and
    2^20 + 1 of the concatenated list and of the class's own list where it reaches them, and n_random random ones.  Returns
    {class: sorted unique slots of the concatenated list}"""
    out = {}
    for k, (a, b) in enumerate(class_ranges(lists)):
        if a == b:
            out[k] = np.zeros(0, np.int64)
            continue
        s = [a, b - 1]
        s += [e for e in (EDGE - 1, EDGE, EDGE + 1) if a <= e < b]
        s += [a + e for e in (EDGE - 1, EDGE, EDGE + 1) if a + e < b]
        s += list(rng.integers(a, b, n_random))
        out[k] = np.unique(np.asarray(s, np.int64))
    return out


def frozen_pattern(n, seed):
    """the caller's frozen set of the compaction tests, in LIST order over n slots: [0, 3000) frozen (the first whole blocks count
    zero), the next 5000 active, the last 2000 frozen, each slot in between frozen with probability 1/2"""
    assert n > 12000
    f = np.random.default_rng(seed).random(n) < 0.5
    f[:3000] = True
    f[3000:8000] = False
    f[n - 2000:] = True
    return f
