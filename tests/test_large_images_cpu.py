"""CPU suite: what tests/test_large_images_gpu.py rests on (no device).

1. tests/large_image_cases.py restates the pixel lists in vectorised numpy; here it is held against the per-pixel loop of
   tests/test_c4_gpu.py's test_pixel_lists_are_the_stable_partition_of_the_tile_order, on a random class image.
2. The sizes L1 .. L5 do reach what they are chosen for: more than 1024 scan blocks (L2: three chunks or more), and camera rays on
   both sides of the box test, counted in float64.  A GPU test that had lost its classes or its second chunk fails here."""
import numpy as np
import pytest

import large_image_cases as LI
from long_ray_cases import camera_rays64, slab64


def _loop_lists(volpath, cls, rank, world):
    """the loop of test_pixel_lists_are_the_stable_partition_of_the_tile_order"""
    H, W = cls.shape
    want = [[], [], []]
    for ty in range((H + 7) // 8):
        for tx in range((W + 7) // 8):
            if volpath.tile_owner(tx, ty, world) != rank:
                continue
            for y in range(ty * 8, min(ty * 8 + 8, H)):
                for x in range(tx * 8, min(tx * 8 + 8, W)):
                    want[cls[y, x]].append(y << 16 | x)
    return [np.asarray(w, np.uint32) for w in want]


@pytest.mark.parametrize("W,H,world", [(67, 45, 3), (9, 7, 4), (160, 120, 1)])
def test_vectorised_pixel_lists_equal_the_per_pixel_loop(W, H, world):
    import volpath
    cls = np.random.default_rng(W * 1000 + H).integers(0, 3, (H, W))
    seen = np.zeros((H, W), int)
    for rank in range(world):
        got = LI.pixel_lists(cls, rank, world)
        want = _loop_lists(volpath, cls, rank, world)
        for c in range(3):
            assert got[c].dtype == np.uint32 and np.array_equal(got[c], want[c]), (rank, c)
            y, x = LI.unpack(got[c])
            assert (cls[y, x] == c).all()
            seen[y, x] += 1
    assert np.all(seen == 1)
    # (a rank of (9, 7, 4) owns nothing: two tiles, four ranks)
    if (W, H, world) == (9, 7, 4):
        assert sum(sum(len(l) for l in LI.pixel_lists(cls, r, world)) == 0 for r in range(world)) == 2


def test_banded_box_test_is_the_float64_slab_test():
    """box_hits works in bands of rows; at one band and at many it is long_ray_cases' camera_rays64 + slab64"""
    for W, H in ((160, 120), (67, 45)):
        hit = slab64(*camera_rays64(W, H))[0]
        assert np.array_equal(LI.box_hits(W, H) == 1, hit) and 0 < hit.sum() < W * H
        assert np.array_equal(LI._hits_rows(W, H, 8, 19), hit[8:19])
    fine = slab64(*camera_rays64(96, 64))[0]
    assert np.array_equal(LI.box_hits(48, 32, 2), fine.reshape(32, 2, 48, 2).sum(axis=(1, 3)))


@pytest.mark.parametrize("name", sorted(LI.SIZES))
def test_sizes_reach_the_second_chunk_and_both_sides_of_the_box(name):
    W, H, S = LI.SIZES[name]
    assert max(W, H) * S <= 65536 and max(W, H) <= 65535
    blocks, chunks = LI.scan_blocks(W, H), LI.scan_chunks(W, H)
    hits = LI.box_hits(W, H, S)
    n_hit, n_miss = int((hits > 0).sum()), int((hits == 0).sum())
    print("%s: %d x %d (S = %d), %d pixels, %d scan blocks in %d chunks, %d pixels with a box-hitting ray, %d without"
          % (name, W, H, S, W * H, blocks, chunks, n_hit, n_miss))
    assert blocks > LI.SCAN_BLOCK and chunks >= (3 if name == "L2" else 2)
    assert W * H > LI.EDGE                                      # list slots beyond 2^20 at world = 1
    assert n_hit >= LI.MIN_PER_KIND and n_miss >= LI.MIN_PER_KIND
    if name in LI.COUNTED:
        assert (n_hit, n_miss) == LI.COUNTED[name]
    expect = {"L1": (1079, 2), "L2": (3600, 4), "L3": (1536, 2), "L4": (1536, 2), "L5": (1280, 2)}[name]
    assert (blocks, chunks) == expect
    if name == "L3":
        # every rank of the world = 3 run and of L4's world = 4 run owns pixels; L4: 3 tiles a row and 4 ranks, so every rank has tile
        # rows it owns nothing in
        assert all(LI.scan_blocks(W, H, r, 3) > 0 for r in range(3))
    if name == "L4":
        from volpath import dist as vd
        m = vd.tile_owner_map(4, W, H)
        assert m.shape == (8192, 3)
        for r in range(4):
            rows_with = (m == r).any(axis=1)
            assert 1000 < rows_with.sum() < 8192 - 1000


def test_frozen_pattern_of_the_compaction_tests():
    f = LI.frozen_pattern(1100000, 5)
    assert f[:3000].all() and not f[3000:8000].any() and f[-2000:].all()
    mid = f[8000:-2000]
    assert 0.49 < mid.mean() < 0.51
    active = np.flatnonzero(~f)
    assert (active >= LI.EDGE).sum() > 10000 and len(active) < 0.51 * len(f)   # active slots past 2^20; the compacted list is half as long
