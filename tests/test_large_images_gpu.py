"""GPU suite: images past one scan chunk of the pixel lists and at the 16-bit coordinate limit (tests/large_image_cases.py).

The pixel lists and every adaptive round's compaction go through pixlist_scan_k, which scans per-block class counts in chunks of 1024
blocks of 1024 padded slots; an image of more than 2^20 padded slots runs the chunk loop's second iteration and its carry.  Every
comparison is at tolerance 0: the lists against the numpy restatement of their definition (held to the per-pixel loop in
tests/test_large_images_cpu.py), images and samples against the CPU oracle, adaptive calls against tests/adaptive_lib.py and
tests/adaptive_planes_lib.py fed with the library's own one-frame renders."""
import ctypes as C

import numpy as np
import pytest

import adaptive_lib as AL
import adaptive_planes_lib as AP
import large_image_cases as LI
import plane_stats_lib as PS
import scenes
import subpixel_lib as sub

pytestmark = pytest.mark.gpu

F32 = np.float32
E_ARG = -3
FLOOR_Y = 1e-3          # the floor of tests/test_adaptive_gpu.py


@pytest.fixture(autouse=True)
def _restore(vp):
    yield
    vp.set_subpixel(1)
    vp.set_arithmetic(vp.ARITH_EXACT)
    vp.set_lookahead(vp.LOOKAHEAD_DEFAULT)
    vp.set_pipeline(True)
    vp.set_shard(0, 1)
    vp.enable_counters(False)
    vp.set_camera()


def _scene(vp, est, rng_mode, key=(1, 2)):
    vp.set_subpixel(1)
    vp.init_volume(vp.julia_volume(32), brick=1, linear=True)
    vp.init_envmap(scenes.synthetic_env())
    vp.set_sun(scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER)
    vp.set_camera()
    vp.set_estimator(est)
    vp.set_tracking(0)
    vp.set_envmap_sampling(vp.ENV_PASSIVE)
    vp.set_shard(0, 1)
    vp.set_rng(rng_mode, key)
    if est == vp.EST_DECOMP:
        vp.precompute_opacity(scenes.DEFAULT_SUN_DIR)


def _oracle_scene(oracle, est, rng_mode, key=(1, 2)):
    osc = oracle.OracleScene(oracle.julia(32), scenes.synthetic_env(), scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER, estimator=est,
                             rng_mode=rng_mode, seed=key)
    if est == oracle.EST_DECOMP:
        osc.precompute_opacity()
    return osc


def _render(vp, P, first, n, fill=None):
    buf = vp.DeviceBuffer(P.width, P.height)
    try:
        if fill is not None:
            buf.upload(fill)
        vp.render_frames(buf.ptr, first, n, P)
        return buf.download()
    finally:
        buf.free()


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


# ---- 1. the pixel lists, whole
@pytest.mark.parametrize("name,world", [("L1", 1), ("L3", 1), ("L3", 3), ("L4", 4), ("L4", 1), ("L2", 1)])
def test_pixel_lists_are_the_stable_partition_past_one_scan_chunk(vp, name, world):
    """every rank's three lists, entry by entry, against the restatement from the rank's own pixel-table classes; each pixel in
    exactly one list of one rank.  L3: x up to 65534 in the low half of y << 16 | x and 8192 tiles in a row; L4: y up to 65534 in the
    high half, 8192 tile rows for the binary search over row_start, and ranks with tile rows they own nothing in."""
    W, H, _ = LI.SIZES[name]
    _scene(vp, vp.EST_GLOBAL, vp.RNG_PHILOX7)
    P = vp.make_param(W, H)
    seen = np.zeros((H, W), np.uint8)
    for rank in range(world):
        vp.set_shard(rank, world)
        cls = vp.pixel_table(P)[..., 5].astype(np.int64)
        got = vp.pixel_lists(P)
        want = LI.pixel_lists(cls, rank, world)
        rep = LI.chunk_report(got)
        print("%s rank %d of %d: %d scan blocks in %d chunks; general / light / missing = %s; class boundaries in 2^20-slot stretch %s; "
              "classes holding slot 2^20: %s" % (name, rank, world, LI.scan_blocks(W, H, rank, world), LI.scan_chunks(W, H, rank, world),
                                                rep["counts"], rep["boundary_chunk"], rep["classes_crossing_2^20"]))
        for c in range(3):
            assert np.array_equal(got[c], want[c]), (rank, c, len(got[c]), len(want[c]))
            y, x = LI.unpack(got[c])
            seen[y, x] += 1
        if world == 1:
            assert LI.scan_chunks(W, H) >= (3 if name == "L2" else 2)
            assert rep["classes_crossing_2^20"], rep                      # entries on both sides of slot 2^20 within one class
            if name in ("L1", "L2", "L3"):
                assert all(n > 0 for n in rep["counts"]), rep
            if name == "L2":
                assert rep["counts"][0] + rep["counts"][1] > LI.EDGE      # general plus light cross it, not only the box-missing pixels
            ys = np.concatenate([LI.unpack(l)[0] for l in got]); xs = np.concatenate([LI.unpack(l)[1] for l in got])
            assert xs.max() == W - 1 and ys.max() == H - 1
    assert np.all(seen == 1)


# ---- 2. every pixel of a large frame, against the oracle
@pytest.mark.parametrize("env_size", [(64, 32), (1024, 512)], ids=["env64", "env1024"])
@pytest.mark.parametrize("name,est,rng_mode", [("L1", 0, 2), ("L3", 1, 0)], ids=["L1-global-philox7", "L3-decomp-samplerh"])
def test_every_pixel_of_a_large_frame_has_the_oracles_bits(vp, oracle, name, est, rng_mode, env_size):
    """the zero_density medium of test_edge_cases_bit_exact: a sample is a box test and at most one environment lookup, so the oracle
    renders the whole frame; one frame into a zeroed buffer, the whole image at tolerance 0 -- a dropped, duplicated or misaddressed
    slot of any class shows.  env64 is the suite's environment; its texels cover many pixels of images this large, so the same again
    under a 1024 x 512 environment, where fewer neighbours share a colour"""
    W, H, _ = LI.SIZES[name]
    env = scenes.synthetic_env(*env_size)
    osc = oracle.OracleScene(oracle.julia(32), env, scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER, estimator=est, rng_mode=rng_mode, seed=(7, 7))
    want, _ = osc.render_frame(oracle.default_param(W, H, density=0.0), 0, None)
    _scene(vp, est, rng_mode, key=(7, 7))
    vp.init_envmap(env)
    got = _render(vp, vp.make_param(W, H, density=0.0), 0, 1)
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want))).all(axis=-1)
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:5].tolist())
    assert _same(got, want)
    colours = len(np.unique(want[..., :3].reshape(-1, 3), axis=0))
    print("%s %s: %d different colours in the oracle's frame" % (name, env_size, colours))
    assert colours > 10 and (want[..., :3] > 0).all()                        # an image, not a constant, and no pixel left at zero


# ---- 3. scattering samples at the edges of the lists and of the image, against the oracle
def _chosen_pixels(name, lists, seed):
    """{(y, x)} per class from the edge slots of the lists, and the extra pixels of the image's edges"""
    W, H, _ = LI.SIZES[name]
    cat = np.concatenate(lists)
    per_class = {k: list(zip(*[a.tolist() for a in LI.unpack(cat[s])])) for k, s in LI.edge_slots(lists, np.random.default_rng(seed)).items()}
    extra = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    if name == "L3":
        extra += [(y, 65534) for y in range(H)]
    if name == "L4":
        extra += [(65534, x) for x in range(W)]
    return per_class, extra


@pytest.mark.parametrize("est,rng_mode", [(0, 2), (1, 2), (1, 0)], ids=["global-philox7", "decomp-philox7", "decomp-samplerh"])
@pytest.mark.parametrize("name", ["L1", "L3", "L4"])
def test_scattering_samples_at_the_list_and_image_edges_equal_the_oracle(vp, oracle, name, est, rng_mode):
    """the default medium, frames 0 and 1 in one call; per class the first and last list entry, the entries around slot 2^20 and 200
    random ones, the four corners, column 65534 (L3) or row 65534 (L4): each equal to the oracle's two samples summed in frame order"""
    W, H, _ = LI.SIZES[name]
    osc = _oracle_scene(oracle, est, rng_mode)
    oP = oracle.default_param(W, H)
    _scene(vp, est, rng_mode)
    P = vp.make_param(W, H)
    lists = vp.pixel_lists(P)
    got = _render(vp, P, 0, 2)
    per_class, extra = _chosen_pixels(name, lists, seed=100 * int(name[1]) + 10 * est + rng_mode)
    assert len(per_class[0]) > 0 and len(per_class[2]) > 200
    checked = 0
    for what, pixels in list(per_class.items()) + [("edge", extra)]:
        for y, x in pixels:
            want = np.zeros(4, F32)
            for f in (0, 1):
                want = want + osc.render_sample(oP, x, y, f)[0]
            assert want.dtype == F32 and _same(got[y, x], want), (name, what, x, y, got[y, x].tolist(), want.tolist())
            checked += 1
    general = per_class[0]
    heated = sum(1 for y, x in general if got[y, x, 3] > 0)
    print("%s est %d stream %d: %d pixels compared; %d of %d chosen general pixels scattered" % (name, est, rng_mode, checked, heated, len(general)))
    if name == "L4":
        assert heated >= 1
    else:
        assert heated >= 0.1 * len(general)


# ---- 4. adaptive compaction past one chunk
def _sentinel(W, H):
    """a fixed non-zero accumulator pattern, exact in binary32"""
    yy, xx = np.mgrid[0:H, 0:W]
    base = ((xx * 7 + yy * 13) % 251 + 1).astype(F32) * F32(0.125)
    return np.stack([base, base + F32(0.5), base * F32(2.0), base + F32(3.0)], -1).astype(F32)


def _caller_state(vp, P, seed):
    """an adaptive_lib.Stats holding the sentinel accumulator, records with earlier sums, and the caller's frozen pattern laid out in
    the order of the pixel lists; the frozen image (H, W) with it"""
    W, H = P.width, P.height
    cat = np.concatenate(vp.pixel_lists(P))
    assert len(cat) == W * H
    y, x = LI.unpack(cat)
    frozen = np.zeros((H, W), bool)
    frozen[y, x] = LI.frozen_pattern(len(cat), seed)
    st = AL.Stats(W, H)
    st.acc[:] = _sentinel(W, H)
    yy, xx = np.mgrid[0:H, 0:W]
    st.n[:] = (xx + yy) % 3
    st.sum_y[:] = st.n * 0.25
    st.sum_y2[:] = st.n * 0.0625
    st.flags[:] = np.where((xx + yy) % 2 == 0, 0x80, 0).astype(np.uint32)      # (the other bits are the caller's)
    st.flags[frozen] |= AL.FROZEN
    return st, frozen


@pytest.mark.parametrize("name", ["L1", "L3"])
def test_adaptive_round_on_a_callers_frozen_set_past_one_chunk(vp, name):
    """"the frozen set is exactly what d_stats says": one round of two frames on a pattern that leaves the first blocks of the list
    empty, the last ones too, and every second slot between; min_frames = 1000, so nothing freezes.  Frozen pixels keep their bytes;
    active ones hold render_frames' bits and the restatement's records."""
    W, H, _ = LI.SIZES[name]
    _scene(vp, vp.EST_GLOBAL, vp.RNG_PHILOX7)
    P = vp.make_param(W, H)
    want, frozen = _caller_state(vp, P, seed=11)
    acc0, rec0 = want.acc.copy(), want.records()
    active = int((~frozen).sum())
    plain = _render(vp, P, 0, 2, fill=acc0)
    frame, fbuf = AL.library_frames(vp, P)
    buf, stats = vp.DeviceBuffer(W, H), vp.StatsBuffer(W, H)
    try:
        buf.upload(acc0); stats.upload(rec0)
        args = dict(rel_tol=0.05, floor_y=FLOOR_Y, min_frames=1000, round_frames=2)
        res = vp.render_adaptive(buf.ptr, stats.ptr, 0, 2, P, **args)
        acc, rec = buf.download(), stats.download()
        wres = AL.render_adaptive(want, frame, 0, 2, **args)
    finally:
        fbuf.free(); buf.free(); stats.free()
    assert res == wres == {"samples": 2 * active, "rounds": 1, "active_left": active, "frames_used": 2}, (res, wres)
    assert acc[frozen].tobytes() == acc0[frozen].tobytes() and rec[frozen].tobytes() == rec0[frozen].tobytes()
    assert _same(acc[~frozen], plain[~frozen])
    assert (rec["n"][~frozen] == rec0["n"][~frozen] + 2).all()
    assert AL.same_state(want, acc, rec) is None, AL.same_state(want, acc, rec)


@pytest.mark.parametrize("name", ["L1", "L3"])
def test_adaptive_rounds_on_the_renders_own_frozen_set_past_one_chunk(vp, name):
    """zeroed records, two rounds of two frames: after round 0 every pixel whose two samples are equal has lhs == 0 and freezes, the rest
    by the criterion; round 1 compacts that data-dependent pattern.  Everything the call leaves against adaptive_lib.render_adaptive."""
    W, H, _ = LI.SIZES[name]
    _scene(vp, vp.EST_GLOBAL, vp.RNG_PHILOX7)
    P = vp.make_param(W, H)
    args = dict(rel_tol=0.05, floor_y=FLOOR_Y, min_frames=2, round_frames=2)
    frame, fbuf = AL.library_frames(vp, P)
    buf, stats = vp.DeviceBuffer(W, H), vp.StatsBuffer(W, H)
    try:
        res = vp.render_adaptive(buf.ptr, stats.ptr, 0, 4, P, **args)
        acc, rec = buf.download(), stats.download()
        want = AL.Stats(W, H)
        wres = AL.render_adaptive(want, frame, 0, 4, **args)
    finally:
        fbuf.free(); buf.free(); stats.free()
    second = int((want.n == 4).sum())
    print("%s: round 0 on %d pixels, round 1 on %d; result %s" % (name, W * H, second, res))
    assert 0 < second < W * H and wres["rounds"] == 2 and wres["samples"] == 2 * W * H + 2 * second
    assert res == wres, (res, wres)
    assert AL.same_state(want, acc, rec) is None, AL.same_state(want, acc, rec)


def test_adaptive_groups_round_on_a_frozen_set_in_one_planes_records(vp):
    """vp_render_adaptive_groups at L1 with the caller's pattern in the sky plane's records only: the compaction ORs the flags of both
    record buffers, so the pixel is left alone in both planes"""
    W, H, _ = LI.SIZES["L1"]
    _scene(vp, vp.EST_GLOBAL, vp.RNG_PHILOX7)
    P = vp.make_param(W, H)
    sky, frozen = _caller_state(vp, P, seed=12)
    sun = sky.copy()
    sun.flags &= ~np.uint32(AL.FROZEN)
    sun.acc[:] = sun.acc + F32(1.0)
    want = (sun, sky)
    start = [(s.acc.copy(), s.records()) for s in want]
    active = int((~frozen).sum())
    q = [vp.DeviceBuffer(W, H), vp.DeviceBuffer(W, H)]
    acc = [vp.DeviceBuffer(W, H), vp.DeviceBuffer(W, H)]
    rec = [vp.StatsBuffer(W, H), vp.StatsBuffer(W, H)]
    try:
        for k in (0, 1):
            acc[k].upload(start[k][0]); rec[k].upload(start[k][1])
        args = dict(rel_tol=(0.05, 0.05), floor_y=(FLOOR_Y, FLOOR_Y), min_frames=1000, round_frames=2)
        res = vp.render_adaptive_groups(acc[0].ptr, acc[1].ptr, rec[0].ptr, rec[1].ptr, 0, 2, P, **args)
        got = tuple(b.download() for b in acc + rec)
        frames = PS.library_frames(lambda f: vp.render_frames_groups(q[0].ptr, q[1].ptr, f, 1, P), q)
        wres = AP.render_adaptive_planes(want, frames, 0, 2, **args)
    finally:
        for b in q + acc + rec:
            b.free()
    assert res == wres == {"samples": 2 * active, "rounds": 1, "active_left": active, "frames_used": 2}, (res, wres)
    for k in (0, 1):
        assert got[k][frozen].tobytes() == start[k][0][frozen].tobytes() and got[2 + k][frozen].tobytes() == start[k][1][frozen].tobytes(), k
        assert (got[2 + k]["n"][~frozen] == start[k][1]["n"][~frozen] + 2).all()
    assert not (got[2]["flags"] & AL.FROZEN).any()
    assert AP.same_pair(want, got) is None, AP.same_pair(want, got)


# ---- 5. the sub-pixel limit S W = 65536
@pytest.mark.parametrize("est,rng_mode", [(0, 2), (1, 0)], ids=["global-philox7", "decomp-samplerh"])
def test_subpixel_factor_at_its_width_limit_equals_the_oracle_on_the_fine_image(vp, oracle, est, rng_mode):
    """S = 2 at W = 32768: the samples are those of a 65536-wide image, which no S = 1 render accepts, so the oracle on the fine
    image's Param is the only reference.  Frames 0 .. 3, one aligned block of S^2 frames: the four lattice points of every pixel."""
    W, H, S = LI.SIZES["L5"]
    osc = _oracle_scene(oracle, est, rng_mode)
    fP = sub.fine_of(oracle.default_param(W, H), S)
    assert (fP.width, fP.height) == (65536, 80)
    _scene(vp, est, rng_mode)
    try:
        vp.set_subpixel(S)
        P = vp.make_param(W, H)
        got = _render(vp, P, 0, 4)
        # one column more is refused, nothing rendered, and the context renders the same bits afterwards
        over = vp.make_param(W + 1, H)
        buf = vp.DeviceBuffer(W + 1, H)
        try:
            assert vp.lib().vp_render_frames(buf.ptr, 0, 4, C.byref(over)) == E_ARG
            assert b"sub-pixel" in vp.lib().vp_last_error()
            assert not buf.download().any()
        finally:
            buf.free()
        assert _render(vp, P, 0, 4).tobytes() == got.tobytes()
        lists = vp.pixel_lists(P)
    finally:
        vp.set_subpixel(1)
    cat = np.concatenate(lists)
    assert len(cat) == W * H > LI.EDGE
    rng = np.random.default_rng(5)
    slots = LI.edge_slots(lists, rng, n_random=70)
    pixels = set()
    for k in range(3):
        pixels |= set(zip(*[a.tolist() for a in LI.unpack(cat[slots[k]])]))
    pixels |= {(y, x) for y in range(H) for x in (0, W - 1)}
    pixels |= {(y, int(x)) for y in (0, H - 1) for x in rng.integers(0, W, 30)}
    assert len(pixels) >= 300
    offs = set()
    for y, x in sorted(pixels):
        want = np.zeros(4, F32)
        for f in range(4):
            i, j = vp.subpixel_offset(x, y, f, S)
            offs.add((i, j))
            want = want + osc.render_sample(fP, S * x + i, S * y + j, f)[0]
        assert _same(got[y, x], want), (x, y, got[y, x].tolist(), want.tolist())
    assert offs == {(0, 0), (0, 1), (1, 0), (1, 1)}
    general = list(zip(*[a.tolist() for a in LI.unpack(cat[slots[0]])]))
    heated = sum(1 for y, x in general if got[y, x, 3] > 0)
    print("L5 est %d stream %d: %d pixels compared, %d of %d chosen general pixels scattered" % (est, rng_mode, len(pixels), heated, len(general)))
    assert heated >= 0.1 * len(general)
