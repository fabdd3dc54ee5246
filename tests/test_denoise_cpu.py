"""The NL-means filter of the output stage (include/volpath.h vp_denoise) without a GPU: known answers of the numpy restatement
(tests/denoise_lib.py), the restatement on the oracle's frames of the scene the defaults were chosen on, the argument refusals that
come before the device, and the CLI flags."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import adaptive_lib as A
import denoise_lib as D
import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cuda-volpath_amd", "volpath_render")
NEW_SYMBOLS = ("vp_denoise", "vp_set_denoise_form", "vp_last_denoise_form")
E_ARG = -3
F32 = np.float32
# the scene of the issue's table: Julia-32, 64 x 48, global majorant, Philox2x32-7, key (1, 2), synthetic environment, default sun
SCENE = dict(est="global", rng="philox7", key=(1, 2))


def records(W, H, n, mean_y, var_of_mean):
    """records whose mean luminance and variance of the mean are the given (exactly representable) numbers"""
    rec = np.zeros((H, W), A.Stats(1, 1).records().dtype)
    nd = np.float64(n)
    rec["n"] = n
    rec["sum_y"] = nd * mean_y
    rec["sum_y2"] = (var_of_mean * nd * nd * (nd - 1.0) + rec["sum_y"] * rec["sum_y"]) / nd
    return rec


# ---- known answers of the restatement
def test_constant_image_with_equal_variances_is_the_clipped_box_mean():
    """y the same everywhere and v the same everywhere: e = -2v / (eps + 2 k2 v) < 0, D = 0, every weight exactly 1: each pixel is
    the mean of the colours in its search window clipped to the image, summed in raster order and divided once"""
    W, H, R, n = 9, 7, 2, 4
    rng = np.random.default_rng(3)
    # red = green = 1 and a blue channel too small to move y (0.0722f * blue is far below half an ulp of 0.9278): y is ONE number,
    # and blue -- small integers times 2^-30, so that every sum below is exact -- carries the picture
    c = np.ones((H, W, 3), F32)
    c[..., 2] = rng.integers(0, 4, (H, W)).astype(F32) * F32(2.0 ** -30)
    assert np.unique(A.luminance(c)).size == 1
    acc = np.zeros((H, W, 4), F32)
    acc[..., :3] = c * F32(n)             # n = 4: the scaling is exact both ways
    acc[..., 3] = 8.0
    rec = records(W, H, n, 0.5, 0.25)
    assert (D.variance(rec) == F32(0.25)).all()
    out = D.denoise(acc, rec, R, 1, 0.45)
    for y in range(H):
        for x in range(W):
            num, den = np.zeros(3, F32), F32(0)
            for oy in range(-R, R + 1):
                for ox in range(-R, R + 1):
                    if 0 <= y + oy < H and 0 <= x + ox < W:
                        den = den + F32(1)
                        num = num + c[y + oy, x + ox]
            assert out[y, x, :3].tobytes() == (num / den).tobytes(), (x, y)
    assert (out[..., 3] == 2.0).all()
    # the corner's window is 3 x 3, the centre's 5 x 5
    assert out[0, 0, 2] == c[:3, :3, 2].sum(dtype=F32) / F32(9) and out[3, 4, 2] == c[1:6, 2:7, 2].sum(dtype=F32) / F32(25)


def test_zero_variance_and_zero_radius_return_the_mean_image():
    acc, rec = D.synthetic(17, 9, 11)
    c, s = D.mean_image(acc, rec["n"])
    want = np.concatenate([c, (acc[..., 3] * s)[..., None]], axis=-1)
    with np.errstate(invalid="ignore"):
        assert want.tobytes() == A.scale_by_count(acc, rec["n"], 1.0).tobytes()
    # R = 0: one offset, weight exactly 1, x / 1
    assert D.denoise(acc, rec, 0, 2, 0.45).tobytes() == want.tobytes()
    # v == 0 everywhere: identical samples (sum_y2 = sum_y^2 / n with dyadic numbers), and n < 2
    flat = records(17, 9, 4, 0.5, 0.0)
    flat["n"][2, 3], flat["n"][4, 5] = 0, 1
    assert not D.variance(flat).any()
    c2, s2 = D.mean_image(acc, flat["n"])
    got = D.denoise(acc, flat, 5, 1, 0.45)
    assert got[..., :3].tobytes() == c2.tobytes() and got[..., 3].tobytes() == (acc[..., 3] * s2).tobytes()
    assert not got[2, 3].any()
    # ... and a guide with v == 0 switches the filter off whatever src's own records say
    assert D.denoise(acc, rec, 5, 1, 0.45, guide=acc, guide_rec=flat)[..., :3].tobytes() == c.tobytes()


def test_weights_come_from_the_guide_and_colours_from_src():
    a1, r1 = D.synthetic(16, 16, 21)
    a2, r2 = D.synthetic(16, 16, 22)
    own = D.denoise(a1, r1, 2, 1, 0.45)
    cross = D.denoise(a1, r1, 2, 1, 0.45, guide=a2, guide_rec=r2)
    assert D.denoise(a1, r1, 2, 1, 0.45, guide=a1, guide_rec=r1).tobytes() == own.tobytes()
    assert cross.tobytes() != own.tobytes()
    assert cross[..., 3].tobytes() == own[..., 3].tobytes()            # heat: src's, unfiltered
    # flags are never read
    r3 = r1.copy(); r3["flags"] ^= 1
    assert D.denoise(a1, r3, 2, 1, 0.45).tobytes() == own.tobytes()


# ---- the scene the CLI defaults were chosen on
@pytest.fixture(scope="module")
def table_scene(oracle):
    osc, oP = A.anchor_oracle(oracle, scenes, SCENE)
    st = A.render_uniform(A.Stats(A.ANCHOR_W, A.ANCHOR_H), A.oracle_frames(osc, oP), 0, 16)
    ref = None
    for f in range(1000, 1256):
        ref, _ = osc.render_frame(oP, f, ref)
    return st, ref / F32(256)


def test_denoising_sixteen_frames_reduces_the_error(table_scene):
    """frames 0..15 against the mean of frames 1000..1255: noisy 0.1453; (5, 1, 0.7) 0.1030 = 0.709 of it, (3, 1, 0.45) 0.1141 = 0.785"""
    st, ref = table_scene
    rec = st.records()
    noisy = D.rel_l2(A.scale_by_count(st.acc, st.n, 1.0), ref)
    c, _ = D.mean_image(st.acc, st.n)
    flat = D.lhs_of(rec) <= 0
    print("noisy %.4f, pixels with lhs <= 0: %d" % (noisy, int(flat.sum())))
    assert int(flat.sum()) == 2690
    for R, Fp, k in ((5, 1, 0.7), (3, 1, 0.45)):
        out = D.denoise(st.acc, rec, R, Fp, k)
        err = D.rel_l2(out, ref)
        print("(%d, %d, %.2f): %.4f = %.3f of the noisy image" % (R, Fp, k, err, err / noisy))
        assert err <= 0.9 * noisy
        same = (out[..., :3].view(np.uint32) == c.view(np.uint32)).all(axis=-1)
        print("    bit-equal to the plain mean: %d pixels, %d of them with lhs > 0" % (int(same.sum()), int((same & ~flat).sum())))
        assert same[flat].all()                    # every per-pixel-constant pixel is the plain mean, bit for bit
        if k == 0.7:
            assert np.array_equal(same, flat)      # ... and no other pixel is
        else:
            # At (3, 1, 0.45) ONE measured pixel, (22, 22), comes out as its own mean as well: its sixteen samples nearly agree
            # (v = 2.6e-16), every neighbour's weight is below half an ulp of the centre's 1, and the sums round to c * 1 / 1.
            # That is the definition's answer, not a skipped pixel: the pixel's v is not 0.
            extra = same & ~flat
            assert int(extra.sum()) <= 1 and (D.variance(rec)[extra] < 1e-12).all()
        assert out[..., 3].tobytes() == A.scale_by_count(st.acc, st.n, 1.0)[..., 3].tobytes()


# ---- the C ABI without a device
def test_new_symbols_are_declared_and_exported():
    import volpath
    text = open(os.path.join(ROOT, "include", "volpath.h")).read()
    for n in NEW_SYMBOLS:
        assert n in volpath.PART2_SYMBOLS
        assert re.search(r"\bint\s+%s\s*\(" % n, text), n
        assert hasattr(volpath.lib(), n)
    assert re.search(r"#define\s+VP_DENOISE_MAX_RADIUS\s+10\b", text) and re.search(r"#define\s+VP_DENOISE_MAX_PATCH\s+3\b", text)
    assert (volpath.DENOISE_MAX_RADIUS, volpath.DENOISE_MAX_PATCH) == (D.MAX_RADIUS, D.MAX_PATCH) == (10, 3)
    assert C.sizeof(volpath.DenoiseParams) == 12


def test_argument_refusals_come_before_the_device():
    """every refusal of the header returns VP_E_ARG; the pointers are never followed (and no device is asked for)"""
    import volpath
    L = volpath.lib()
    dst, src, st, gd, gst = (C.c_void_p(a) for a in (0x1000, 0x2000, 0x3000, 0x4000, 0x5000))   # never dereferenced

    def call(d=dst, s=src, t=st, g=None, gt=None, w=16, h=8, radius=5, patch=1, k=0.45, dp="default"):
        arg = C.byref(volpath.DenoiseParams(radius, patch, k)) if dp == "default" else dp
        return L.vp_denoise(d, s, t, g, gt, w, h, arg)

    assert call(d=None) == E_ARG and call(s=None) == E_ARG and call(t=None) == E_ARG and call(dp=None) == E_ARG
    assert call(g=gd) == E_ARG and call(gt=gst) == E_ARG                       # exactly one of the guide pair
    assert call(d=src) == E_ARG                                                # in place
    assert call(d=gd, g=gd, gt=gst) == E_ARG
    assert call(w=0) == E_ARG and call(h=0) == E_ARG and call(w=-3) == E_ARG and call(h=-1) == E_ARG
    assert call(radius=-1) == E_ARG and call(radius=volpath.DENOISE_MAX_RADIUS + 1) == E_ARG
    assert call(patch=-1) == E_ARG and call(patch=volpath.DENOISE_MAX_PATCH + 1) == E_ARG
    for k in (0.0, -0.45, float("nan"), float("inf"), -float("inf")):
        assert call(k=k) == E_ARG, k
    assert "vp_denoise" in L.vp_last_error().decode()
    with pytest.raises(volpath.VolpathError, match="radius"):
        volpath.denoise(dst, src, st, 16, 8, radius=11)
    with pytest.raises(volpath.VolpathError, match="guide"):
        volpath.denoise(dst, src, st, 16, 8, guide_ptr=gd)
    # the form hook: 0 and 1, nothing else; the context stays usable
    assert L.vp_set_denoise_form(2) == E_ARG and L.vp_set_denoise_form(-1) == E_ARG
    assert L.vp_set_denoise_form(1) == 0 and L.vp_set_denoise_form(0) == 0
    assert L.vp_last_denoise_form() == 0
    assert L.vp_set_bound_brick(8) == 0 and L.vp_set_bound_brick(1) == 0


def test_cli_denoise_flags():
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--denoise", "--denoise-radius", "--denoise-patch", "--denoise-k"):
        assert flag in r.stdout, flag
    for bad in (["--denoise-radius"], ["--denoise", "--denoise-radius", "11"], ["--denoise", "--denoise-radius", "-1"],
                ["--denoise", "--denoise-patch", "4"], ["--denoise", "--denoise-k", "0"], ["--denoise", "--denoise-k", "abc"],
                ["--denoise", "--denoise-k", "nan"]):
        r = subprocess.run([EXE] + bad, capture_output=True, text=True)
        assert r.returncode == 2, (bad, r.stdout, r.stderr)
    # records are not reduced across ranks: refused with a message, before anything is rendered
    r = subprocess.run([EXE, "--denoise", "--gpus", "2"], capture_output=True, text=True)
    assert r.returncode == 2 and "--denoise" in r.stderr and "--gpus" in r.stderr
