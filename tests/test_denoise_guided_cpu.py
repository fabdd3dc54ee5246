"""The feature-guided NL-means filter (include/volpath.h vp_denoise_guided) without a GPU: the ABI, the argument
refusals that come before the device, known answers of the numpy restatement (tests/denoise_guided_lib.py), the conditions the GPU
cases rest on, the quality table's chosen cell on the oracle's frames, and the CLI flags."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import adaptive_lib as A
import denoise_guided_lib as G
import denoise_lib as D
import features_lib as FL
import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cuda-volpath_amd", "volpath_render")
E_ARG = -3
F32 = np.float32
INF = F32(np.inf)
# the scene of DESIGN.md 2.4's table: Julia-32, 64 x 48, global majorant, Philox2x32-7, key (1, 2), synthetic environment, default sun
SCENE = dict(est="global", rng="philox7", key=(1, 2))
# DESIGN.md section 2.13, relative L2 against the mean of frames 1000..1255: the recorded values
NOISY, PLAIN_5_1 = 0.145320349, 0.107198333
CLI_SIGMA_ALPHA, CLI_SIGMA_DEPTH, GUIDED_5_1 = 0.2, 0.2, 0.112379203    # the best cell of the 3 x 3 grid: it does NOT beat vp_denoise here


# ---- the C ABI without a device
def test_symbol_struct_and_constant():
    import volpath
    text = open(os.path.join(ROOT, "include", "volpath.h")).read()
    assert "vp_denoise_guided" in volpath.PART2_SYMBOLS and hasattr(volpath.lib(), "vp_denoise_guided")
    assert re.search(r"\bint\s+vp_denoise_guided\s*\(", text)
    assert re.search(r"typedef\s+struct\s*\{\s*const\s+vp_float4\*\s*plane;\s*int\s+channel;\s*float\s+sigma;\s*\}\s*vp_denoise_feature;", text)
    assert re.search(r"#define\s+VP_DENOISE_MAX_FEATURES\s+4\b", text)
    assert volpath.DENOISE_MAX_FEATURES == G.MAX_FEATURES == 4
    assert C.sizeof(volpath.DenoiseFeature) == 16
    assert (volpath.DenoiseFeature.plane.offset, volpath.DenoiseFeature.channel.offset, volpath.DenoiseFeature.sigma.offset) == (0, 8, 12)


def test_argument_refusals_come_before_the_device():
    """every refusal of the header returns VP_E_ARG; no pointer is followed and no device is asked for"""
    import volpath
    L = volpath.lib()
    dst, src, st, gd, gst, pl, pl2 = (C.c_void_p(a) for a in (0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000))   # never dereferenced
    good = [(pl, 1, 0.1)]

    def call(d=dst, s=src, t=st, g=None, gt=None, feats=good, n=None, w=16, h=8, radius=5, patch=1, k=0.45, dp="default", null_array=False):
        arg = C.byref(volpath.DenoiseParams(radius, patch, k)) if dp == "default" else dp
        arr = (volpath.DenoiseFeature * max(len(feats), 1))(*[volpath.DenoiseFeature(getattr(p, "value", p), c, s_) for p, c, s_ in feats])
        return L.vp_denoise_guided(d, s, t, g, gt, None if null_array else arr, len(feats) if n is None else n, w, h, arg)

    # everything vp_denoise refuses, with one feature and with none
    for feats in (good, []):
        assert call(d=None, feats=feats) == E_ARG and call(s=None, feats=feats) == E_ARG and call(t=None, feats=feats) == E_ARG
        assert call(dp=None, feats=feats) == E_ARG
        assert call(g=gd, feats=feats) == E_ARG and call(gt=gst, feats=feats) == E_ARG
        assert call(d=src, feats=feats) == E_ARG and call(d=gd, g=gd, gt=gst, feats=feats) == E_ARG
        assert call(w=0, feats=feats) == E_ARG and call(h=0, feats=feats) == E_ARG and call(w=-3, feats=feats) == E_ARG and call(h=-1, feats=feats) == E_ARG
        assert call(radius=-1, feats=feats) == E_ARG and call(radius=volpath.DENOISE_MAX_RADIUS + 1, feats=feats) == E_ARG
        assert call(patch=-1, feats=feats) == E_ARG and call(patch=volpath.DENOISE_MAX_PATCH + 1, feats=feats) == E_ARG
        for k in (0.0, -0.45, float("nan"), float("inf"), -float("inf")):
            assert call(k=k, feats=feats) == E_ARG, k
    # the feature list
    assert call(n=-1) == E_ARG and call(feats=good * 4, n=5) == E_ARG
    assert call(null_array=True) == E_ARG                                           # features == NULL with n_features > 0
    assert call(feats=[(None, 0, 0.1)]) == E_ARG                                    # a NULL plane
    assert call(feats=[(pl, 0, 0.1), (None, 0, 0.1)]) == E_ARG
    assert call(feats=[(dst, 0, 0.1)]) == E_ARG and call(feats=[(pl, 0, 0.1), (pl2, 3, 0.1), (dst, 2, 0.1)]) == E_ARG   # a plane equal to dst
    assert call(feats=[(pl, -1, 0.1)]) == E_ARG and call(feats=[(pl, 4, 0.1)]) == E_ARG
    for sigma in (0.0, -0.1, float("nan"), float("inf"), -float("inf")):
        assert call(feats=[(pl, 0, sigma)]) == E_ARG, sigma
    # sigma fine, g = 1 / (2 sigma^2) not: 2 sigma^2 underflows to 0 or to a denormal whose reciprocal is inf, or overflows
    for sigma in (1e-30, 1e-20, 1e20, 3e38):
        assert np.isfinite(F32(sigma)) and F32(sigma) > 0 and not (np.isfinite(G.g_of(sigma)) and G.g_of(sigma) > 0), sigma
        assert call(feats=[(pl, 0, sigma)]) == E_ARG, sigma
        assert call(feats=[(pl, 0, 0.1), (pl, 1, sigma)]) == E_ARG, sigma
    assert "vp_denoise_guided" in L.vp_last_error().decode()
    with pytest.raises(volpath.VolpathError, match="channel"):
        volpath.denoise_guided(dst, src, st, 16, 8, features=[(pl, 7, 0.1)])
    with pytest.raises(volpath.VolpathError, match="sigma"):
        volpath.denoise_guided(dst, src, st, 16, 8, features=[(pl, 0, 0.1), (pl2, 1, 0.0)])
    with pytest.raises(volpath.VolpathError, match="radius"):
        volpath.denoise_guided(dst, src, st, 16, 8, radius=11)
    # the context stays usable
    assert L.vp_set_denoise_form(1) == 0 and L.vp_set_denoise_form(0) == 0 and L.vp_last_denoise_form() == 0


# ---- known answers of the restatement
def _plane(values, channel=0):
    p = np.zeros(values.shape + (4,), F32)
    p[..., channel] = values
    return p


def test_no_feature_and_a_constant_feature_change_nothing():
    acc, rec = D.synthetic(23, 13, 5)
    ga, gr = D.synthetic(23, 13, 6)
    for R, Fp in ((2, 1), (3, 0)):
        want = D.denoise(acc, rec, R, Fp, 0.45)
        assert G.denoise_guided(acc, rec, [], R, Fp, 0.45).tobytes() == want.tobytes()
        for const in (0.0, 0.37, 1e30, np.inf, -np.inf):       # fa == fb everywhere: t = 0, two equal infinities included
            f = _plane(np.full((13, 23), const, F32), 2)
            assert G.denoise_guided(acc, rec, [(f, 2, 0.01)], R, Fp, 0.45).tobytes() == want.tobytes(), const
            assert G.denoise_guided(acc, rec, [(f, 2, 0.01), (f, 2, 5.0)], R, Fp, 0.45).tobytes() == want.tobytes(), const
    want = D.denoise(acc, rec, 2, 1, 0.45, guide=ga, guide_rec=gr)
    assert G.denoise_guided(acc, rec, [], 2, 1, 0.45, guide=ga, guide_rec=gr).tobytes() == want.tobytes()
    # a feature that varies does change the output
    f = _plane(np.random.default_rng(1).uniform(0, 1, (13, 23)).astype(F32))
    assert G.denoise_guided(acc, rec, [(f, 0, 0.05)], 2, 1, 0.45).tobytes() != D.denoise(acc, rec, 2, 1, 0.45).tobytes()


def test_a_mask_with_a_tiny_sigma_splits_the_image_into_two_filters():
    """mask 0 left of column m, 1 from it on; sigma 1e-3: g = 5e5, a pair across the mask has w = expf_(-5e5) = 0 exactly, and adding
    an exact 0 changes neither sum.  With patch 0 the distance of a pair involves no third pixel, so each side is the filter run on
    that side alone, byte for byte -- in particular wherever the window crosses the mask"""
    W, H, m, R = 21, 11, 9, 4
    acc, rec = D.synthetic(W, H, 12)
    mask = _plane((np.arange(W)[None, :] >= m).astype(F32).repeat(H, axis=0), 3)
    assert G.g_of(1e-3) > 4e5
    got = G.denoise_guided(acc, rec, [(mask, 3, 1e-3)], R, 0, 0.45)
    left, right = D.denoise(acc[:, :m], rec[:, :m], R, 0, 0.45), D.denoise(acc[:, m:], rec[:, m:], R, 0, 0.45)
    assert got[:, :m].tobytes() == left.tobytes() and got[:, m:].tobytes() == right.tobytes()
    # ... and that is not what the unguided filter gives next to the mask
    plain = D.denoise(acc, rec, R, 0, 0.45)
    near = (D.variance(rec) != 0) & (np.abs(np.arange(W)[None, :] - m + 0.5) < R)
    assert near.sum() > 20 and (got[near] != plain[near]).any(axis=-1).mean() > 0.9


def test_no_finite_pixel_receives_colour_from_an_infinite_region():
    """a depth-like feature with a +inf region: change src's colours inside the region (the guide pair, which alone makes the patch
    distances, stays) and the output outside keeps its bytes; inside, it changes"""
    W, H = 33, 17
    acc, rec = D.synthetic(W, H, 31, flat_block=False)
    ga, gr = D.synthetic(W, H, 32, flat_block=False)
    _, depth = G.synthetic_features(W, H, 1)
    hole = np.isinf(depth[..., 1])
    assert 0.2 < hole.mean() < 0.4 and hole[0, 0] and hole[:, 0].any() and hole[0, :].any() and not hole[-1, -1]
    acc2 = acc.copy()
    acc2[hole, :3] = acc[hole, :3] * F32(3.0) + F32(1.0)
    f = [(depth, 1, 0.2)]
    a = G.denoise_guided(acc, rec, f, 4, 1, 0.45, guide=ga, guide_rec=gr)
    b = G.denoise_guided(acc2, rec, f, 4, 1, 0.45, guide=ga, guide_rec=gr)
    assert a[~hole].tobytes() == b[~hole].tobytes()
    assert (a[hole] != b[hole]).any()
    # without the feature the colours do leak
    pa, pb = D.denoise(acc, rec, 4, 1, 0.45, guide=ga, guide_rec=gr), D.denoise(acc2, rec, 4, 1, 0.45, guide=ga, guide_rec=gr)
    assert pa[~hole].tobytes() != pb[~hole].tobytes()
    assert np.isfinite(a).all() and np.isfinite(b).all()


def test_conditions_of_the_gpu_cases():
    """what keeps the GPU comparison at 70 x 37 from passing on nothing: the features change at least half of the filtered pixels, and
    some window holds a pair with both features +inf and a pair with +inf against a finite value"""
    W, H, R = 70, 37, 5
    acc, rec = D.synthetic(W, H, 100 + W)
    alpha, depth = G.synthetic_features(W, H, 100 + W)
    hole = np.isinf(depth[..., 1])
    assert 0.25 < hole.mean() < 0.35 and hole[:, 0].any() and hole[0, :].any()
    assert set(np.unique(depth[..., 3])) == {0.0, 1.0} and alpha[..., 1].min() >= 0 and alpha[..., 1].max() <= 1
    assert np.abs(np.diff(alpha[..., 1], axis=1)).max() > 0.3                      # the step edge
    noisy = D.variance(rec) != 0
    plain = D.denoise(acc, rec, R, 1, 0.45)
    for feats in ([(alpha, 1, 0.1)], [(alpha, 1, 0.1), (depth, 1, 0.2), (depth, 3, 0.1)]):
        got = G.denoise_guided(acc, rec, feats, R, 1, 0.45)
        changed = (got.view(np.uint32) != plain.view(np.uint32)).any(axis=-1)
        print("pixels with v != 0: %d, changed by %d features: %d" % (noisy.sum(), len(feats), changed[noisy].sum()))
        assert changed[noisy].mean() >= 0.5 and not changed[~noisy].any()
    both = inf_fin = False
    for oy in range(-R, R + 1):
        for ox in range(-R, R + 1):
            a = hole[max(0, -oy):H - max(0, oy), max(0, -ox):W - max(0, ox)]
            b = hole[max(0, oy):H - max(0, -oy), max(0, ox):W - max(0, -ox)]
            n = noisy[max(0, -oy):H - max(0, oy), max(0, -ox):W - max(0, ox)]
            both |= bool((a & b & n).any()) and (oy, ox) != (0, 0)
            inf_fin |= bool((a & ~b & n).any()) and bool((~a & b & n).any())
    assert both and inf_fin


# ---- the quality table's scene
@pytest.fixture(scope="module")
def table_scene(oracle):
    osc, oP = A.anchor_oracle(oracle, scenes, SCENE)
    st = A.render_uniform(A.Stats(A.ANCHOR_W, A.ANCHOR_H), A.oracle_frames(osc, oP), 0, 16)
    ref = None
    for f in range(1000, 1256):
        ref, _ = osc.render_frame(oP, f, ref)
    alpha, depth, _ = FL.features(oracle, osc, A.ANCHOR_W, A.ANCHOR_H, 0.01, oP.density, tuple(oP.sigma_t))
    return st, ref / F32(256), alpha, depth


def test_quality_on_sixteen_frames_is_the_recorded_table(table_scene):
    """frames 0..15 against the mean of frames 1000..1255, filters at (5, 1, 0.45): noisy 0.145320, vp_denoise 0.107198, guided with
    (alpha.y, SA), (depth.y, SZ), (depth.w, SA) at the best cell of SA, SZ in {0.05, 0.1, 0.2}, SA = SZ = 0.2: 0.112379.  No cell of the
    grid beats vp_denoise on this scene (the full grid is in DESIGN.md section 2.13), so the values are pinned and no order is asserted"""
    st, ref, alpha, depth = table_scene
    rec = st.records()
    noisy = D.rel_l2(A.scale_by_count(st.acc, st.n, 1.0), ref)
    plain = D.rel_l2(D.denoise(st.acc, rec, 5, 1, 0.45), ref)
    feats = [(alpha, 1, CLI_SIGMA_ALPHA), (depth, 1, CLI_SIGMA_DEPTH), (depth, 3, CLI_SIGMA_ALPHA)]
    out = G.denoise_guided(st.acc, rec, feats, 5, 1, 0.45)
    guided = D.rel_l2(out, ref)
    print("noisy %.9f  vp_denoise %.9f  guided %.9f" % (noisy, plain, guided))
    assert abs(noisy - NOISY) <= 1e-6 * NOISY
    assert abs(plain - PLAIN_5_1) <= 1e-6 * PLAIN_5_1
    assert abs(guided - GUIDED_5_1) <= 1e-6 * GUIDED_5_1
    if GUIDED_5_1 < PLAIN_5_1:
        assert guided <= plain
    assert np.isfinite(out).all()
    assert out[..., 3].tobytes() == A.scale_by_count(st.acc, st.n, 1.0)[..., 3].tobytes()
    # the features of this scene carry what the definition's special cases are for
    zt = depth[..., 1]
    assert np.isinf(zt).any() and np.isfinite(zt).any() and set(np.unique(depth[..., 3])) == {0.0, 1.0}


# ---- the CLI
def test_cli_flags_and_defaults():
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--denoise-features", "--denoise-sigma-alpha", "--denoise-sigma-depth"):
        assert flag in r.stdout, flag
    src = open(os.path.join(ROOT, "cuda-volpath_amd", "host", "main.cpp")).read()
    m = re.search(r"dn_sigma_alpha\s*=\s*([0-9.eE+-]+)f\s*,\s*dn_sigma_depth\s*=\s*([0-9.eE+-]+)f", src)
    assert m and (float(m.group(1)), float(m.group(2))) == (CLI_SIGMA_ALPHA, CLI_SIGMA_DEPTH)       # the defaults are the table's best cell
    for bad in (["--denoise-features"], ["--denoise", "--denoise-features", "--aa", "2"], ["--denoise", "--denoise-features", "--gpus", "2"],
                ["--denoise", "--denoise-features", "--denoise-sigma-alpha", "0"], ["--denoise", "--denoise-features", "--denoise-sigma-depth", "nan"],
                ["--denoise", "--denoise-features", "--denoise-sigma-depth"], ["--groups-out", "g", "--groups-denoise", "--denoise-features"]):
        r = subprocess.run([EXE] + bad, capture_output=True, text=True)
        assert r.returncode == 2, (bad, r.stdout, r.stderr)
    r = subprocess.run([EXE, "--denoise-features"], capture_output=True, text=True)
    assert "--denoise-features" in r.stderr and "--denoise" in r.stderr
