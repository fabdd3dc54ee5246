"""Half-buffer renders and the cross-filtered output stage (include/volpath.h vp_render_frames_halves_stats, vp_merge_halves,
vp_accumulate_stats) without a GPU: the ABI, the refusals that come before the device, known answers of the
numpy restatement (tests/halves_lib.py), the half rule against vp_subpixel_offset, the conditions the GPU cases rest on, the quality
table on the oracle's frames, and the CLI flags."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import adaptive_lib as A
import denoise_lib as D
import halves_lib as HL
import layers_lib as LL
import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cuda-volpath_amd", "volpath_render")
E_ARG = -3
F32 = np.float32
# the scene of DESIGN.md 2.4's table: Julia-32, 64 x 48, global majorant, Philox2x32-7, key (1, 2), synthetic environment, default sun
SCENE = dict(est="global", rng="philox7", key=(1, 2))
# DESIGN.md section 2.15, relative L2 of frames 0..15 against the mean of frames 1000..1255, filters at (5, 1, 0.45): the recorded values
NOISY, SELF_5_1, CROSS_5_1, MERGED_PLAIN = 0.145320349, 0.107198333, 0.111544635, 0.145320353    # the cross-filter does NOT beat vp_denoise here


# ---- the C ABI without a device
def test_symbols_and_mirrors():
    import volpath
    text = open(os.path.join(ROOT, "include", "volpath.h")).read()
    for sym in ("vp_render_frames_halves_stats", "vp_merge_halves", "vp_accumulate_stats"):
        assert sym in volpath.PART2_SYMBOLS and hasattr(volpath.lib(), sym), sym
        assert re.search(r"\bint\s+%s\s*\(" % sym, text), sym
    for name in ("render_frames_halves_stats", "merge_halves", "accumulate_stats", "denoise_cross", "half_of_frame"):
        assert callable(getattr(volpath, name)), name
    for S in (1, 2, 4, 8):
        for f in (0, 1, 3, 4, 15, 16, 63, 64, 65, 1000):
            assert volpath.half_of_frame(f, S) == HL.half_of_frame(f, S) == (f // (S * S)) % 2


def test_argument_refusals_come_before_the_device():
    """every refusal of the header returns VP_E_ARG; no pointer is followed and no device is asked for"""
    import volpath
    L = volpath.lib()
    h0, h1, s0, s1, dst, res = (C.c_void_p(a) for a in (0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000))   # never dereferenced
    P = volpath.make_param(16, 12)

    def halves(a=h0, b=h1, ra=s0, rb=s1, first=0, n=4, p=C.byref(P)):
        return L.vp_render_frames_halves_stats(a, b, ra, rb, first, n, p)

    assert halves(a=None) == E_ARG and halves(b=None) == E_ARG and halves(ra=None) == E_ARG and halves(rb=None) == E_ARG and halves(p=None) == E_ARG
    assert halves(b=h0) == E_ARG and halves(rb=s0) == E_ARG
    assert halves(n=0) == E_ARG and halves(n=-2) == E_ARG and halves(first=-1) == E_ARG
    assert "vp_render_frames_halves_stats" in L.vp_last_error().decode()

    def merge(d=dst, r=res, a=h0, ra=s0, b=h1, rb=s1, size=192, fl=1e-3):
        return L.vp_merge_halves(d, r, a, ra, b, rb, size, fl)

    assert merge(d=None) == E_ARG and merge(a=None) == E_ARG and merge(b=None) == E_ARG and merge(ra=None) == E_ARG and merge(rb=None) == E_ARG
    assert merge(size=-1) == E_ARG
    for fl in (0.0, -1e-3, float("nan"), float("inf"), -float("inf")):
        assert merge(fl=fl) == E_ARG, fl
    assert "vp_merge_halves" in L.vp_last_error().decode()
    assert L.vp_accumulate_stats(None, s0, 10) == E_ARG and L.vp_accumulate_stats(s0, None, 10) == E_ARG
    assert "vp_accumulate_stats" in L.vp_last_error().decode()
    with pytest.raises(volpath.VolpathError, match="different buffers"):
        volpath.render_frames_halves_stats(h0, h0, s0, s1, 0, 4, P)
    with pytest.raises(volpath.VolpathError, match="floor_y"):
        volpath.merge_halves(dst, res, h0, s0, h1, s1, 192, floor_y=0.0)


# ---- known answers of the restatement
def test_equal_halves_merge_to_the_half_with_resid_zero():
    acc, rec = D.synthetic(23, 13, 5)
    mean = A.scale_by_count(acc, rec["n"], 1.0)
    dst, resid = HL.merge_halves(mean, rec, mean, rec)
    seen = rec["n"] > 0
    # m n + m n = 2 (m n) exactly, so dst = (m n) / n with two roundings: m bit for bit where n is a power of two (both operations are
    # then exact) -- the counts of an even split of 2^k frames --, and m up to the two roundings for any n
    exact = seen & np.isin(rec["n"], (1, 2, 16, 64))
    assert exact.sum() > 100 and (seen & ~exact).sum() >= 1
    assert dst[exact].tobytes() == mean[exact].tobytes()
    assert np.allclose(dst[seen], mean[seen], rtol=2.4e-7, atol=0)
    assert not dst[~seen].any() and not resid.any()
    assert (~seen).any()
    # the halves of sixteen frames: eight samples each, everywhere
    rec8 = rec.copy()
    rec8["n"] = 8
    dst, resid = HL.merge_halves(mean, rec8, mean, rec8)
    assert dst.tobytes() == mean.tobytes() and not resid.any()


def test_an_empty_half_contributes_nothing_and_unequal_counts_weigh_as_written():
    a, ra = D.synthetic(23, 13, 5)
    b, rb = D.synthetic(23, 13, 6)
    ma, mb = A.scale_by_count(a, ra["n"], 1.0), A.scale_by_count(b, rb["n"], 1.0)
    dst, resid = HL.merge_halves(ma, ra, mb, rb)
    only_a, only_b, none, both = (ra["n"] > 0) & (rb["n"] == 0), (ra["n"] == 0) & (rb["n"] > 0), (ra["n"] == 0) & (rb["n"] == 0), (ra["n"] > 0) & (rb["n"] > 0)
    assert only_a.sum() >= 3 and only_b.sum() >= 3 and both.sum() > 100
    # x * n / n is x up to the two roundings; with b's term an exact 0
    assert np.allclose(dst[only_a], ma[only_a], rtol=2e-7, atol=0) and np.allclose(dst[only_b], mb[only_b], rtol=2e-7, atol=0)
    assert not resid[only_a].any() and not resid[only_b].any() and not resid[none].any() and not dst[none].any()
    uneq = both & (ra["n"] != rb["n"])
    assert uneq.sum() > 50
    y, x = np.argwhere(uneq)[7]
    na, nb = F32(ra["n"][y, x]), F32(rb["n"][y, x])
    for c in range(4):
        assert dst[y, x, c] == (ma[y, x, c] * na + mb[y, x, c] * nb) / (na + nb)
    lum = lambda v: (F32(0.2126) * v[0] + F32(0.7152) * v[1]) + F32(0.0722) * v[2]
    ym = lum(dst[y, x])
    assert resid[y, x] == (F32(0.5) * abs(lum(ma[y, x]) - lum(mb[y, x]))) / (ym if ym > F32(1e-3) else F32(1e-3))
    assert (resid[uneq] > 0).mean() > 0.9 and np.isfinite(resid).all() and np.isfinite(dst).all()
    # the floor takes over where the merged luminance is below it
    _, big_floor = HL.merge_halves(ma, ra, mb, rb, floor_y=1e6)
    assert (big_floor[both] == (F32(0.5) * np.abs(A.luminance(ma) - A.luminance(mb)))[both] / F32(1e6)).all()
    # the records add
    s = HL.accumulate_stats(ra, rb)
    assert np.array_equal(s["n"], ra["n"] + rb["n"]) and np.array_equal(s["flags"], ra["flags"] | rb["flags"])
    assert np.array_equal(s["sum_y"], ra["sum_y"] + rb["sum_y"]) and (s["flags"] != ra["flags"]).any()


def test_the_guide_matters():
    """a half filtered with the other half's weights is not the half filtered with its own"""
    a, ra = D.synthetic(23, 13, 5)
    b, rb = D.synthetic(23, 13, 6)
    dst, resid, fa, fb = HL.denoise_cross(a, ra, b, rb, 2, 1, 0.45)
    own = D.denoise(a, ra, 2, 1, 0.45)
    assert fa.tobytes() != own.tobytes()
    assert fa.tobytes() == D.denoise(a, ra, 2, 1, 0.45, guide=b, guide_rec=rb).tobytes()
    assert fb.tobytes() == D.denoise(b, rb, 2, 1, 0.45, guide=a, guide_rec=ra).tobytes()
    want, want_resid = HL.merge_halves(fa, ra, fb, rb)
    assert dst.tobytes() == want.tobytes() and resid.tobytes() == want_resid.tobytes()
    assert np.isfinite(dst).all()


# ---- the half rule
@pytest.mark.parametrize("S", [1, 2, 4])
def test_each_half_covers_the_lattice_in_every_aligned_window(S):
    """within any aligned window of 2 S^2 frames the frames of either half hit each of the S x S sub-pixels exactly once, whatever the
    per-pixel hash of vp_subpixel_offset"""
    import volpath
    lattice = sorted((i, j) for i in range(S) for j in range(S))
    for x, y in ((0, 0), (1, 0), (5, 7), (63, 47), (640, 359), (65535, 65535)):
        for w0 in (0, 2 * S * S, 6 * S * S, 1024):
            assert w0 % (2 * S * S) == 0
            for h in (0, 1):
                fr = HL.frames_of_half(w0, 2 * S * S, h, S)
                assert len(fr) == S * S
                assert sorted(volpath.subpixel_offset(x, y, f, S) for f in fr) == lattice, (S, x, y, w0, h)


def test_plain_parity_does_not_cover_the_lattice():
    """the reason for the rule: with S = 2 the even frames of a window see half of the footprint only"""
    import volpath
    S = 2
    for x, y in ((0, 0), (5, 7), (63, 47)):
        for parity in (0, 1):
            seen = {volpath.subpixel_offset(x, y, f, S) for f in range(0, 64) if f % 2 == parity}
            assert len(seen) == 2, (x, y, parity, seen)


# ---- what the GPU cases rest on
def test_conditions_of_the_gpu_cases(oracle):
    """the 16 x 12 Julia-32 view of layers_lib: camera rays that miss the box, rays that hit it and fetch no density in any frame (the
    light class's signature under the decomposition estimator) and rays that do; and frames 10 and 11 -- one per half -- differ"""
    osc = oracle.OracleScene(LL.grid_of("julia", oracle), LL.ENV, scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER, estimator=1, rng_mode=1, seed=LL.KEY)
    osc.precompute_opacity()
    P = oracle.default_param(LL.W, LL.H, **LL.JULIA_KW)
    E = LL.expected(oracle, "julia", 1, 1)
    img, cnt = zip(*[osc.render_samples(P, f) for f in LL.FRAMES])
    no_lookup = np.all([c["density_lookups"] == 0 for c in cnt], axis=0)
    miss, light, general = E.miss, no_lookup & ~E.miss, ~no_lookup
    print("box-missing %d, no lookup %d, general %d" % (miss.sum(), light.sum(), general.sum()))
    assert miss.sum() >= 1 and light.sum() >= 1 and general.sum() >= 1
    assert HL.half_of_frame(LL.FRAMES[0]) == 0 and HL.half_of_frame(LL.FRAMES[1]) == 1
    assert (img[0] != img[1]).any(axis=-1).sum() >= 1
    assert [HL.runs_of_half(6, 11, h, 2) for h in (0, 1)] == [[(8, 4), (16, 1)], [(6, 2), (12, 4)]]


# ---- the quality table's scene
@pytest.fixture(scope="module")
def table_scene(oracle):
    osc, oP = A.anchor_oracle(oracle, scenes, SCENE)
    frames = A.oracle_frames(osc, oP)
    whole = A.render_uniform(A.Stats(A.ANCHOR_W, A.ANCHOR_H), frames, 0, 16)
    h0, h1 = HL.render_halves(A.Stats(A.ANCHOR_W, A.ANCHOR_H), A.Stats(A.ANCHOR_W, A.ANCHOR_H), frames, 0, 16)
    ref = None
    for f in range(1000, 1256):
        ref, _ = osc.render_frame(oP, f, ref)
    return whole, h0, h1, ref / F32(256)


def test_quality_on_sixteen_frames_is_the_recorded_table(table_scene):
    """frames 0..15 against the mean of frames 1000..1255, filters at (5, 1, 0.45): the plain mean, vp_denoise self-guided on all sixteen
    frames, the cross-filter of the two halves of eight, and the merge of the unfiltered halves (the plain mean up to rounding).  The
    values are pinned as measured; no order is asserted in advance"""
    whole, h0, h1, ref = table_scene
    assert (h0.n == 8).all() and (h1.n == 8).all() and (whole.n == 16).all()
    noisy = D.rel_l2(A.scale_by_count(whole.acc, whole.n, 1.0), ref)
    plain = D.rel_l2(D.denoise(whole.acc, whole.records(), 5, 1, 0.45), ref)
    r0, r1 = h0.records(), h1.records()
    out, resid, _, _ = HL.denoise_cross(h0.acc, r0, h1.acc, r1, 5, 1, 0.45)
    cross = D.rel_l2(out, ref)
    merged, _ = HL.merge_halves(A.scale_by_count(h0.acc, h0.n, 1.0), r0, A.scale_by_count(h1.acc, h1.n, 1.0), r1)
    merged_plain = D.rel_l2(merged, ref)
    print("noisy %.9f  self-guided %.9f  cross %.9f  merged unfiltered %.9f" % (noisy, plain, cross, merged_plain))
    assert abs(noisy - NOISY) <= 1e-6 * NOISY
    assert abs(plain - SELF_5_1) <= 1e-6 * SELF_5_1
    assert abs(cross - CROSS_5_1) <= 1e-6 * CROSS_5_1
    assert abs(merged_plain - MERGED_PLAIN) <= 1e-6 * MERGED_PLAIN
    assert np.isfinite(out).all() and np.isfinite(resid).all() and (resid >= 0).all() and resid.max() > 0
    # a pixel the filter leaves alone because it is a constant in both halves gives exactly 0
    const = (D.variance(r0) == 0) & (D.variance(r1) == 0)
    assert const.sum() > 100 and not resid[const].any()


# ---- the CLI
def test_cli_flags_and_refusals():
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--denoise-cross", "--resid-out"):
        assert flag in r.stdout, flag
    for bad in (["--denoise-cross", "--gpus", "2"], ["--denoise-cross", "--noise", "0.1"], ["--denoise-cross", "--layers-out", "l"],
                ["--denoise-cross", "--over", "0", "0", "0"], ["--denoise-cross", "--groups-out", "g"], ["--denoise-cross", "--sun-gain", "1", "1", "1"],
                ["--denoise-cross", "--planes-out", "p"], ["--denoise-cross", "--groups-out", "g", "--groups-denoise"],
                ["--denoise-cross", "--layers-out", "l", "--layers-denoise"], ["--denoise-cross", "--planes-out", "p", "--planes-denoise"],
                ["--denoise-cross", "--denoise-features", "--aa", "2"], ["--resid-out", "r.hdr"], ["--denoise", "--resid-out", "r.hdr"],
                ["--denoise-cross", "--resid-out"], ["--denoise-cross", "--denoise-k", "0"]):
        r = subprocess.run([EXE] + bad, capture_output=True, text=True)
        assert r.returncode == 2, (bad, r.stdout, r.stderr)
    r = subprocess.run([EXE, "--denoise-cross", "--noise", "0.1"], capture_output=True, text=True)
    assert "--denoise-cross" in r.stderr and "--noise" in r.stderr
    r = subprocess.run([EXE, "--resid-out", "r.hdr"], capture_output=True, text=True)
    assert "--resid-out" in r.stderr and "--denoise-cross" in r.stderr
    # --denoise-cross implies --denoise; --aa above 1 is refused only together with --denoise-features
    src = open(os.path.join(ROOT, "cuda-volpath_amd", "host", "main.cpp")).read()
    assert re.search(r'a == "--denoise-cross"\)\s*denoise_cross\s*=\s*denoise\s*=\s*true', src)
