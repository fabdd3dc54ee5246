"""Per-pixel filter selection (include/volpath.h vp_cross_error, vp_select) without a GPU: the ABI, the refusals
that come before the device, known answers of the numpy restatement (tests/select_lib.py), the quality rows on the oracle's frames,
and the CLI flags."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import adaptive_lib as A
import denoise_lib as D
import halves_lib as HL
import scenes
import select_lib as S
import variance_lib as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cuda-volpath_amd", "volpath_render")
E_ARG = -3
F32 = np.float32
CANDIDATES = ((5, 1, 0.45), (10, 3, 0.45))
VAR = (1, 3, 0.45)
# DESIGN.md section 2.18, relative L2 of frames 0..N-1 against the mean of frames 1000..1255, 64 x 48, global majorant, Philox2x32-7,
# key (1, 2): (scene, frames) -> (candidate (5, 1), candidate (10, 3), selected), the values as measured with the restatement
RECORDED = {
    ("julia", 16): (0.111479317, 0.106946995, 0.103512406),
    ("julia", 64): (0.076228325, 0.072448188, 0.073168515),
    ("cloud", 16): (0.109393701, 0.116852910, 0.103159903),
    ("cloud", 64): (0.093093711, 0.101040864, 0.089916671),
}
BEATS_BOTH = {("julia", 16): True, ("julia", 64): False, ("cloud", 16): True, ("cloud", 64): True}


# ---- the C ABI without a device
def test_symbols_and_mirrors():
    import volpath
    text = open(os.path.join(ROOT, "include", "volpath.h")).read()
    stub = open(os.path.join(ROOT, "scripts", "cli_trace_stub.c")).read()
    for sym in ("vp_cross_error", "vp_select"):
        assert sym in volpath.PART2_SYMBOLS and hasattr(volpath.lib(), sym), sym
        assert re.search(r"\bint\s+%s\s*\(" % sym, text), sym
        assert re.search(r"\bint\s+%s\s*\(" % sym, stub), sym
    assert re.search(r"typedef struct \{ int smooth_radius, blend_radius; \} vp_select_params;", text)
    assert re.search(r"#define VP_SELECT_MAX_CANDIDATES 4\b", text) and re.search(r"#define VP_SELECT_MAX_RADIUS 3\b", text)
    assert C.sizeof(volpath.SelectParams) == 8
    assert [f[0] for f in volpath.SelectParams._fields_] == ["smooth_radius", "blend_radius"]
    assert volpath.SelectParams.blend_radius.offset == 4
    assert (volpath.SELECT_MAX_CANDIDATES, volpath.SELECT_MAX_RADIUS) == (4, 3) == (S.MAX_CANDIDATES, S.MAX_RADIUS)
    for name in ("cross_error", "select", "denoise_select"):
        assert callable(getattr(volpath, name)), name
    par = inspect.signature(volpath.denoise_select).parameters
    assert par["candidates"].default == CANDIDATES and par["smooth"].default == 1 and par["blend"].default == 1 and par["variance"].default == VAR
    assert par["features"].default is None


def test_argument_refusals_come_before_the_device():
    """every refusal of the header returns VP_E_ARG; no pointer is followed and no device is asked for"""
    import volpath
    L = volpath.lib()
    err, fa, fb, h0, s0, h1, s1, dst, idx = (C.c_void_p(a) for a in (0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000, 0x8000, 0x9000))   # never dereferenced

    def cross(e=err, a=fa, b=fb, x0=h0, r0=s0, x1=h1, r1=s1, size=192):
        return L.vp_cross_error(e, a, b, x0, r0, x1, r1, size)

    for name in ("e", "a", "b", "x0", "r0", "x1", "r1"):
        assert cross(**{name: None}) == E_ARG, name
    for same in (fa, fb, h0, s0, h1, s1):
        assert cross(e=same) == E_ARG
    assert cross(size=-1) == E_ARG
    assert "vp_cross_error" in L.vp_last_error().decode()

    imgs = [0xA000, 0xB000, 0xC000, 0xD000, 0xE000]
    errs = [0x1A000, 0x1B000, 0x1C000, 0x1D000, 0x1E000]

    def sel(d=dst, ix=idx, im=imgs[:2], er=errs[:2], n=None, w=16, h=12, rs=1, rb=1, sp="default", null_im=False, null_er=False):
        ia = (C.c_void_p * max(len(im), 1))(*im)
        ea = (C.c_void_p * max(len(er), 1))(*er)
        arg = C.byref(volpath.SelectParams(rs, rb)) if sp == "default" else sp
        return L.vp_select(d, ix, None if null_im else ia, None if null_er else ea, len(im) if n is None else n, w, h, arg)

    assert sel(d=None) == E_ARG and sel(null_im=True) == E_ARG and sel(null_er=True) == E_ARG and sel(sp=None) == E_ARG
    assert sel(im=[], er=[], n=0) == E_ARG and sel(n=-1) == E_ARG and sel(im=imgs, er=errs, n=5) == E_ARG
    assert sel(im=[imgs[0], None]) == E_ARG and sel(er=[errs[0], None]) == E_ARG and sel(im=[None], er=errs[:1]) == E_ARG
    assert sel(er=[errs[0], dst.value]) == E_ARG and sel(er=[dst.value], im=imgs[:1]) == E_ARG and sel(ix=dst) == E_ARG
    assert sel(w=0) == E_ARG and sel(h=0) == E_ARG and sel(w=-3) == E_ARG and sel(h=-1) == E_ARG
    for r in (-1, 4):
        assert sel(rs=r) == E_ARG and sel(rb=r) == E_ARG
    assert "vp_select" in L.vp_last_error().decode()
    with pytest.raises(volpath.VolpathError, match="blend_radius"):
        volpath.select(dst, None, imgs[:2], errs[:2], 16, 12, 1, 4)
    with pytest.raises(volpath.VolpathError, match="d_err is one of the inputs"):
        volpath.cross_error(fa, fa, fb, h0, s0, h1, s1, 192)
    with pytest.raises(ValueError, match="error planes"):
        volpath.select(dst, None, imgs[:2], errs[:1], 16, 12)
    # the helper asks for every buffer before it queues anything
    with pytest.raises(ValueError, match="var_ptrs"):
        volpath.denoise_select(dst, None, h0, s0, h1, s1, 16, 12, tmp=(fa, fb, imgs[:2], errs[:2]))
    with pytest.raises(ValueError, match="tmp="):
        volpath.denoise_select(dst, None, h0, s0, h1, s1, 16, 12, var_ptrs=(err, fa, fb))
    with pytest.raises(ValueError, match="tmp="):
        volpath.denoise_select(dst, None, h0, s0, h1, s1, 16, 12, var_ptrs=(err, fa, fb), tmp=(fa, fb, imgs[:1], errs[:2]))
    assert L.vp_set_denoise_form(1) == 0 and L.vp_set_denoise_form(0) == 0 and L.vp_last_denoise_form() == 0


# ---- known answers of the restatement
def test_select_one_candidate_and_equal_planes():
    imgs = S.images_for(23, 13, 3, 1)
    errs = S.error_planes(23, 13, 3, 2, "noise")
    for Rs, Rb in ((0, 0), (1, 1), (3, 3)):
        # n = 1 is a copy
        dst, k = S.select(imgs[:1], errs[:1], Rs, Rb)
        assert dst.tobytes() == imgs[0].tobytes() and not k.any()
        # equal planes: images[0], index 0 -- the order of the candidates is a preference
        dst, k = S.select(imgs, [errs[1]] * 3, Rs, Rb)
        assert dst.tobytes() == imgs[0].tobytes() and not k.any()


def test_select_radius_zero_is_the_hard_pick_and_negative_errors_count():
    imgs = S.images_for(23, 13, 3, 1)
    errs = S.error_planes(23, 13, 3, 2, "noise")
    assert all((e < 0).sum() > 50 for e in errs)
    dst, k = S.select(imgs, errs, 0, 0)
    want_k = np.argmin(np.stack(errs), 0)                       # (the noise has no ties; argmin's first index would settle one alike)
    assert (k == want_k).all() and set(np.unique(k)) == {0, 1, 2}
    assert dst.tobytes() == np.take_along_axis(np.stack(imgs), want_k[None, ..., None], 0)[0].tobytes()
    assert (S.smooth_error(errs[0], 0) == errs[0]).all()        # (x / 1.0f)
    # the most negative plane wins everywhere, whatever the radii
    low = [errs[0], errs[1], np.full((13, 23), -50.0, F32)]
    for Rs, Rb in ((0, 0), (2, 1), (3, 3)):
        dst, k = S.select(imgs, low, Rs, Rb)
        assert (k == 2).all() and dst.tobytes() == imgs[2].tobytes()


def test_select_border_counts_on_a_hand_made_case():
    """5 x 3, Rs = 1: the window of a corner holds 4 positions, of an edge 6, of the middle row's interior 9; an all-ones plane smooths to
    exactly 1 everywhere only if every count is the in-image count"""
    ones = np.ones((3, 5), F32)
    assert (S.window_count(3, 5, 1) == np.array([[4, 6, 6, 6, 4], [6, 9, 9, 9, 6], [4, 6, 6, 6, 4]])).all()
    assert (S.smooth_error(ones, 1) == 1).all() and (S.smooth_error(ones, 3) == 1).all()
    assert (S.window_count(3, 5, 3) == np.array([[12, 15, 15, 15, 12]] * 3)).all()
    # a single spike: its share in each window that holds it is 9 / count
    e = np.zeros((3, 5), F32)
    e[0, 0] = 9
    E = S.smooth_error(e, 1)
    assert E.tolist() == [[2.25, 1.5, 0, 0, 0], [1.5, 1, 0, 0, 0], [0, 0, 0, 0, 0]]
    # the blend: candidate 1 wins the left column only (Rs = 0); W_1 counts the in-image window positions in column 0
    e0, e1 = np.zeros((3, 5), F32), np.ones((3, 5), F32)
    e1[:, 0] = -1
    a, b = np.full((3, 5, 4), 2.0, F32), np.full((3, 5, 4), 4.0, F32)
    a[..., 3], b[..., 3] = 7, 9
    dst, k = S.select([a, b], [e0, e1], 0, 1)
    assert k.tolist() == [[1, 0, 0, 0, 0]] * 3
    # column 0: T = 4, 6, 4 and W_1 = 2, 3, 2: (2 * 2 + 2 * 4) / 4 = 3; column 1: T = 6, 9, 6, W_1 = 2, 3, 2: (4 * 2 + 2 * 4) / 6 = 16 / 6
    assert (dst[:, 0, :3] == 3).all() and (dst[:, 1, :3] == F32(16) / F32(6)).all() and (dst[1, 1, :3] == F32(24) / F32(9)).all()
    assert (dst[:, 2:, :3] == 2).all()
    # w is the pick's and is never blended
    assert (dst[:, 0, 3] == 9).all() and (dst[:, 1:, 3] == 7).all()


def test_select_unmixed_windows_carry_the_candidates_bits():
    W, H, n = 70, 37, 4
    imgs = S.images_for(W, H, n, 5)
    errs = S.error_planes(W, H, n, 6, "block")
    agree = np.ones((H, W), bool)
    for c in range(1, n):
        agree &= (imgs[c].view(np.uint32) == imgs[0].view(np.uint32)).all(-1)
    assert agree.sum() > 100
    for Rs, Rb in ((1, 1), (3, 3)):
        dst, k = S.select(imgs, errs, Rs, Rb)
        # the block's interior: the last candidate wins throughout and the window is its own
        assert (k[0:30 - Rs, 26 + Rs:70] == n - 1).all()
        inner = (slice(0, 30 - Rs - Rb), slice(26 + Rs + Rb, 70))
        assert dst[inner].tobytes() == imgs[n - 1][inner].tobytes() and dst[inner].size > 4 * 32 * 8
        # w everywhere is the pick's
        own = np.take_along_axis(np.stack(imgs), k[None, ..., None].astype(np.int64), 0)[0]
        assert dst[..., 3].tobytes() == own[..., 3].tobytes()
        # elsewhere the picks mix and the blend differs from every candidate
        assert all((dst[..., :3] != i[..., :3]).any() for i in imgs)
        # where all candidates agree bit for bit the value stays: exactly where one candidate holds the window, and otherwise up to the
        # roundings of the blend -- n products, n sums and one divide, each half an ulp: (2 n + 1) 2^-24 relative
        same = dst[agree][:, :3]
        ref = imgs[0][agree][:, :3]
        assert (np.abs(same.astype(np.float64) - ref) <= (2 * n + 1) * 2.0 ** -24 * np.abs(ref)).all()
        assert (same == ref).mean() > 0.5


def test_cross_error_rules():
    W, H = 23, 13
    h0, r0 = D.synthetic(W, H, 5)
    h1, r1 = D.synthetic(W, H, 6)
    fa, fb = A.scale_by_count(h0, r0["n"], 1.0), A.scale_by_count(h1, r1["n"], 1.0)
    err = S.cross_error(fa, fb, h0, r0, h1, r1)
    few = (r0["n"] < 2) | (r1["n"] < 2)
    assert few.sum() >= 5 and not err[few].any() and (err[~few] != 0).sum() > 100 and np.isfinite(err).all()
    assert (err < 0).any() and (err > 0).any()                              # not clamped
    # of the unfiltered halves: (y0 - y1)^2 - 0.5 (v0 + v1), in the definition's operation order
    y0, y1 = A.luminance(D.mean_image(h0, r0["n"])[0]), A.luminance(D.mean_image(h1, r1["n"])[0])
    v0, v1 = D.variance(r0), D.variance(r1)
    assert A.luminance(fa).tobytes() == y0.tobytes()                        # lum of the mean image is y: the same three products
    da, db = y0 - y1, y1 - y0
    want = F32(0.5) * ((da * da - v1) + (db * db - v0))
    assert err[~few].tobytes() == want[~few].tobytes()
    d = (y0 - y1).astype(np.float64)
    exact = d * d - 0.5 * (v0.astype(np.float64) + v1)
    assert np.allclose(err[~few], exact[~few], rtol=1e-5, atol=1e-6 * np.abs(d * d)[~few].max())
    # flags are never read; w of the filtered images is never read
    rf = r0.copy()
    rf["flags"] ^= 1
    fw = fa.copy()
    fw[..., 3] = -1
    assert S.cross_error(fw, fb, h0, rf, h1, r1).tobytes() == err.tobytes()
    # a perfect filter (both halves at the truth) on halves that differ by their noise alone: the estimate scatters round 0
    rng = np.random.default_rng(7)
    n = 64
    smp = rng.normal(2.0, 0.5, (2, n, 40, 40))
    recs = []
    for h in range(2):
        r = np.zeros((40, 40), r0.dtype)
        r["n"], r["sum_y"], r["sum_y2"] = n, smp[h].sum(0), (smp[h] ** 2).sum(0)
        recs.append(r)
    acc = [np.repeat(smp[h].sum(0)[..., None], 4, -1).astype(F32) for h in range(2)]
    truth = np.full((40, 40, 4), 2.0, F32)
    e = S.cross_error(truth, truth, acc[0], recs[0], acc[1], recs[1])
    # per pixel d ~ N(0, v), v = 0.25 / n: d^2 - v has mean 0 and sd sqrt(2) v, the mean of two independent ones sd v; 1600 pixels
    assert abs(e.mean()) < 5 * (0.25 / n) / 40 and (e < 0).mean() > 0.3


# ---- the quality rows
def _scene(oracle, name):
    if name == "julia":
        return A.anchor_oracle(oracle, scenes, dict(est="global", rng="philox7", key=(1, 2)))
    osc = oracle.OracleScene(oracle.cloud(32), scenes.synthetic_env(), scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER, estimator=oracle.EST_GLOBAL,
                             rng_mode=oracle.RNG_PHILOX7, seed=(1, 2))
    return osc, oracle.default_param(A.ANCHOR_W, A.ANCHOR_H, density=100.0, sigma_t=(1, 0.8, 0.6))


@pytest.fixture(scope="module", params=["julia", "cloud"])
def quality_scene(request, oracle):
    osc, oP = _scene(oracle, request.param)
    frames = A.oracle_frames(osc, oP)
    ref = None
    for f in range(1000, 1256):
        ref, _ = osc.render_frame(oP, f, ref)
    return request.param, frames, ref / F32(256)


@pytest.mark.parametrize("nframes", [16, 64])
def test_quality_rows_are_the_recorded_table(quality_scene, nframes):
    """frames 0..N-1 against the mean of frames 1000..1255: the cross-filter with the variance stage at (5, 1, 0.45) and (10, 3, 0.45), and
    the per-pixel selection between them (smooth 1, blend 1).  The values are pinned as measured with the restatement, which rows beat
    the better candidate is pinned, and ONE order is asserted on every row: the selection's error is at most the worse candidate's"""
    name, frames, ref = quality_scene
    h0, h1 = HL.render_halves(A.Stats(A.ANCHOR_W, A.ANCHOR_H), A.Stats(A.ANCHOR_W, A.ANCHOR_H), frames, 0, nframes)
    r0, r1 = h0.records(), h1.records()
    out = S.denoise_select(h0.acc, r0, h1.acc, r1, CANDIDATES, 1, 1, VAR)
    assert np.isfinite(out["dst"]).all() and all(np.isfinite(e).all() for e in out["errors"])
    c0, c1, sel = (D.rel_l2(x, ref) for x in (out["images"][0], out["images"][1], out["dst"]))
    share = [(out["index"] == c).mean() for c in range(2)]
    const = (D.variance(r0) == 0) & (D.variance(r1) == 0)
    best = np.where((((out["images"][0] - ref)[..., :3].astype(np.float64) ** 2).sum(-1) <= ((out["images"][1] - ref)[..., :3].astype(np.float64) ** 2).sum(-1))[..., None],
                    out["images"][0], out["images"][1])
    print("%s %d frames: (5, 1) %.9f  (10, 3) %.9f  selected %.9f  per-pixel best %.9f  share of candidate 0 %.3f, 1 %.3f  constant pixels %.3f  negative estimates %.3f"
          % (name, nframes, c0, c1, sel, D.rel_l2(best, ref), share[0], share[1], const.mean(), (out["errors"][0] < 0).mean()))
    want = RECORDED[(name, nframes)]
    for got, w, what in zip((c0, c1, sel), want, ("(5, 1)", "(10, 3)", "selected")):
        assert abs(got - w) <= 1e-6 * w, (name, nframes, what, got, w)
    assert sel <= max(c0, c1), (name, nframes, sel, c0, c1)
    assert (sel < min(c0, c1)) == BEATS_BOTH[(name, nframes)], (name, nframes, sel, c0, c1)
    # a pixel that is a constant in both halves is left alone by both candidates, its error estimate is exactly 0 in both, and the
    # selection hands it on: candidate 0's value where the tie holds the whole window
    assert const.sum() > 100
    for c in range(2):
        assert not out["errors"][c][const].any()
    mean = HL.merge_halves(A.scale_by_count(h0.acc, r0["n"], 1.0), r0, A.scale_by_count(h1.acc, r1["n"], 1.0), r1, want_resid=False)[0]
    assert out["images"][0][const].tobytes() == mean[const].tobytes() and out["images"][1][const].tobytes() == mean[const].tobytes()
    assert out["dst"][const][:, 3].tobytes() == mean[const][:, 3].tobytes()
    assert (np.abs(out["dst"][const].astype(np.float64) - mean[const]) <= 5 * 2.0 ** -24 * np.abs(mean[const])).all()      # (2 n + 1 roundings of half an ulp)


# ---- the CLI
def test_cli_flags_and_refusals():
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--denoise-select", "--denoise-select-radius", "--denoise-select-patch", "--denoise-select-smooth", "--denoise-select-blend", "--select-out"):
        assert flag in r.stdout, flag
    for bad in (["--denoise-select", "--gpus", "2"], ["--denoise-select", "--noise", "0.1"], ["--denoise-select", "--layers-out", "l"],
                ["--denoise-select", "--over", "0", "0", "0"], ["--denoise-select", "--groups-out", "g"], ["--denoise-select", "--sun-gain", "1", "1", "1"],
                ["--denoise-select", "--planes-out", "p"], ["--denoise-select", "--denoise-features", "--aa", "2"],
                ["--denoise-select", "--resid-out", "r.hdr"], ["--select-out", "s.hdr"], ["--denoise", "--select-out", "s.hdr"],
                ["--denoise-cross", "--select-out", "s.hdr"], ["--denoise-var", "--select-out", "s.hdr"], ["--denoise-select", "--select-out"],
                ["--denoise-select", "--denoise-select-radius", "11"], ["--denoise-select", "--denoise-select-radius", "-1"],
                ["--denoise-select", "--denoise-select-patch", "4"], ["--denoise-select", "--denoise-select-patch"],
                ["--denoise-select", "--denoise-select-smooth", "4"], ["--denoise-select", "--denoise-select-smooth", "x"],
                ["--denoise-select", "--denoise-select-blend", "-1"], ["--denoise-select", "--denoise-select-blend"],
                ["--denoise-select", "--denoise-k", "0"], ["--denoise-select", "--denoise-var-k", "0"]):
        r = subprocess.run([EXE] + bad, capture_output=True, text=True)
        assert r.returncode == 2, (bad, r.stdout, r.stderr)
    r = subprocess.run([EXE, "--denoise-select", "--noise", "0.1"], capture_output=True, text=True)
    assert "--denoise-cross" in r.stderr and "--noise" in r.stderr                      # the refusal it inherits
    r = subprocess.run([EXE, "--denoise-var", "--select-out", "s.hdr"], capture_output=True, text=True)
    assert "--select-out" in r.stderr and "--denoise-select" in r.stderr
    r = subprocess.run([EXE, "--denoise-select", "--resid-out", "r.hdr"], capture_output=True, text=True)
    assert "--resid-out" in r.stderr and "--denoise-select" in r.stderr
    # --denoise-select implies --denoise-var, which implies --denoise-cross, which implies --denoise; candidate 1's window and the radii
    src = open(os.path.join(ROOT, "cuda-volpath_amd", "host", "main.cpp")).read()
    assert re.search(r'a == "--denoise-select"\)\s*denoise_select\s*=\s*denoise_var\s*=\s*denoise_cross\s*=\s*denoise\s*=\s*true', src)
    assert re.search(r"vp_denoise_params\s+dns\s*=\s*\{10,\s*3,\s*0\.45f\}", src) and re.search(r"vp_select_params\s+sel\s*=\s*\{1,\s*1\}", src)
    assert re.search(r"cand\[1\]\.k\s*=\s*o\.dn\.k", src)                                # --denoise-k is shared
