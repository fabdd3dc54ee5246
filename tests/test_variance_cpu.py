"""The variance stage of the cross-filter (include/volpath.h vp_halves_variance, vp_filter_variance, vp_denoise_var; DESIGN.md section
2.17) without a GPU: the ABI, the refusals that come before the device, known answers of the numpy restatement
(tests/variance_lib.py), the quality rows on the oracle's frames, and the CLI flags."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import adaptive_lib as A
import denoise_guided_lib as G
import denoise_lib as D
import halves_lib as HL
import scenes
import variance_lib as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cuda-volpath_amd", "volpath_render")
E_ARG = -3
F32 = np.float32
# the scene of DESIGN.md 2.4's and 2.15's tables: Julia-32, 64 x 48, global majorant, Philox2x32-7, key (1, 2)
SCENE = dict(est="global", rng="philox7", key=(1, 2))
VAR = (1, 3, 0.45)
# DESIGN.md section 2.17, relative L2 of frames 0..15 against the mean of frames 1000..1255: the recorded values
CROSS_10_3 = 0.117482218                                 # the cross-filter without the stage at (10, 3, 0.45)
STAGE_5_1, STAGE_10_3 = 0.111479317, 0.106946995         # with the stage at (1, 3, 0.45)
POOLED_5_1, POOLED_10_3 = 0.110579392, 0.107570251       # pooled only: the variance pass at radius 0


# ---- the C ABI without a device
def test_symbols_and_mirrors():
    import volpath
    text = open(os.path.join(ROOT, "include", "volpath.h")).read()
    for sym in ("vp_halves_variance", "vp_filter_variance", "vp_denoise_var"):
        assert sym in volpath.PART2_SYMBOLS and hasattr(volpath.lib(), sym), sym
        assert re.search(r"\bint\s+%s\s*\(" % sym, text), sym
    for name in ("halves_variance", "filter_variance", "denoise_var", "denoise_cross"):
        assert callable(getattr(volpath, name)), name
    import inspect
    assert inspect.signature(volpath.denoise_cross).parameters["variance"].default is None
    stub = open(os.path.join(ROOT, "scripts", "cli_trace_stub.c")).read()
    for sym in ("vp_halves_variance", "vp_filter_variance", "vp_denoise_var"):
        assert re.search(r"\bint\s+%s\s*\(" % sym, stub), sym


def test_argument_refusals_come_before_the_device():
    """every refusal of the header returns VP_E_ARG; no pointer is followed and no device is asked for"""
    import volpath
    L = volpath.lib()
    u, q, s0, s1, dst, src, gd, pl, var = (C.c_void_p(a) for a in (0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000, 0x8000, 0x9000))   # never dereferenced

    def pooled(a=u, b=q, ra=s0, rb=s1, size=192):
        return L.vp_halves_variance(a, b, ra, rb, size)

    assert pooled(a=None) == E_ARG and pooled(ra=None) == E_ARG and pooled(rb=None) == E_ARG and pooled(size=-1) == E_ARG
    assert "vp_halves_variance" in L.vp_last_error().decode()

    def filt(d=dst, a=u, b=q, w=16, h=12, radius=1, patch=3, k=0.45, dp="default"):
        return L.vp_filter_variance(d, a, b, w, h, C.byref(volpath.DenoiseParams(radius, patch, k)) if dp == "default" else dp)

    assert filt(d=None) == E_ARG and filt(a=None) == E_ARG and filt(b=None) == E_ARG and filt(dp=None) == E_ARG
    assert filt(d=u) == E_ARG and filt(d=q) == E_ARG
    assert filt(w=0) == E_ARG and filt(h=0) == E_ARG and filt(w=-2) == E_ARG and filt(h=-1) == E_ARG
    assert filt(radius=-1) == E_ARG and filt(radius=volpath.DENOISE_MAX_RADIUS + 1) == E_ARG
    assert filt(patch=-1) == E_ARG and filt(patch=volpath.DENOISE_MAX_PATCH + 1) == E_ARG
    for k in (0.0, -0.45, float("nan"), float("inf"), -float("inf")):
        assert filt(k=k) == E_ARG, k
    assert "vp_filter_variance" in L.vp_last_error().decode()

    def dvar(d=dst, s=src, t=s0, g=None, gt=None, v=var, feats=(), n=None, w=16, h=12, radius=5, patch=1, k=0.45, dp="default"):
        arg = C.byref(volpath.DenoiseParams(radius, patch, k)) if dp == "default" else dp
        arr = (volpath.DenoiseFeature * max(len(feats), 1))(*[volpath.DenoiseFeature(getattr(p, "value", p), c, sg) for p, c, sg in feats])
        return L.vp_denoise_var(d, s, t, g, gt, v, arr, len(feats) if n is None else n, w, h, arg)

    # everything vp_denoise_guided refuses, with a plane and without one, with a feature and with none
    for v in (var, None):
        for feats in ([(pl, 1, 0.1)], []):
            kw = dict(v=v, feats=feats)
            assert dvar(d=None, **kw) == E_ARG and dvar(s=None, **kw) == E_ARG and dvar(t=None, **kw) == E_ARG and dvar(dp=None, **kw) == E_ARG
            assert dvar(g=gd, **kw) == E_ARG and dvar(gt=s1, **kw) == E_ARG
            assert dvar(d=src, **kw) == E_ARG and dvar(d=gd, g=gd, gt=s1, **kw) == E_ARG
            assert dvar(w=0, **kw) == E_ARG and dvar(h=0, **kw) == E_ARG
            assert dvar(radius=-1, **kw) == E_ARG and dvar(radius=volpath.DENOISE_MAX_RADIUS + 1, **kw) == E_ARG
            assert dvar(patch=-1, **kw) == E_ARG and dvar(patch=volpath.DENOISE_MAX_PATCH + 1, **kw) == E_ARG
            for k in (0.0, float("nan"), float("inf")):
                assert dvar(k=k, **kw) == E_ARG, k
        assert dvar(v=v, n=-1) == E_ARG and dvar(v=v, feats=[(pl, 1, 0.1)] * 4, n=5) == E_ARG
        assert dvar(v=v, feats=[(None, 0, 0.1)]) == E_ARG and dvar(v=v, feats=[(dst, 0, 0.1)]) == E_ARG
        assert dvar(v=v, feats=[(pl, 4, 0.1)]) == E_ARG and dvar(v=v, feats=[(pl, 0, 0.0)]) == E_ARG
    # its own: a plane that is dst
    assert dvar(v=dst) == E_ARG and dvar(v=dst, feats=[(pl, 1, 0.1)]) == E_ARG
    assert "vp_denoise_var" in L.vp_last_error().decode()
    with pytest.raises(volpath.VolpathError, match="d_sample_var is dst"):
        volpath.denoise_var(dst, src, s0, 16, 12, dst)
    with pytest.raises(volpath.VolpathError, match="radius"):
        volpath.filter_variance(dst, u, q, 16, 12, radius=11)
    with pytest.raises(ValueError, match="var_ptrs"):
        volpath.denoise_cross(dst, None, src, s0, gd, s1, u, q, 16, 12, 5, 1, 0.45, variance=VAR)
    assert L.vp_set_denoise_form(1) == 0 and L.vp_set_denoise_form(0) == 0 and L.vp_last_denoise_form() == 0


# ---- known answers of the restatement
def test_pooled_variance_rules():
    a, ra = D.synthetic(23, 13, 5)
    b, rb = D.synthetic(23, 13, 6)
    # equal halves: q = 0 and u the half's value (0.5 * (x + x) is exact)
    u, q = V.halves_variance(ra, ra)
    ua, ma = V.sample_variance(ra)
    assert u.tobytes() == ua.tobytes() and not q[ma].any()
    assert not q.any()                                              # (not measured: u = 0, q = u * u = 0)
    assert not ua[~ma].any() and (~ma).sum() >= 3 and (ua[ma] > 0).sum() > 100
    # the per-sample variance is vp_denoise's variance of the mean times n, up to the rounding of the two
    vm = D.variance(ra)
    assert np.allclose(ua[ma], vm[ma].astype(np.float64) * ra["n"][ma], rtol=3e-7, atol=0)
    # two different halves
    u, q = V.halves_variance(ra, rb)
    ub, mb = V.sample_variance(rb)
    both, only_a, only_b, none = ma & mb, ma & ~mb, ~ma & mb, ~ma & ~mb
    assert both.sum() > 100 and only_a.sum() >= 3 and only_b.sum() >= 3 and none.sum() >= 1
    assert (u[both] == F32(0.5) * (ua[both] + ub[both])).all()
    d = ua - ub
    assert (q[both] == F32(0.25) * (d * d)[both]).all() and (q[both] > 0).mean() > 0.8
    assert u[only_a].tobytes() == ua[only_a].tobytes() and u[only_b].tobytes() == ub[only_b].tobytes()
    assert (q[only_a] == u[only_a] * u[only_a]).all() and (q[only_b] == u[only_b] * u[only_b]).all()
    assert not u[none].any() and not q[none].any()
    assert np.isfinite(u).all() and np.isfinite(q).all()
    # flags are never read
    rf = ra.copy()
    rf["flags"] ^= 1
    assert V.halves_variance(rf, rb)[0].tobytes() == u.tobytes()


def test_filter_variance_identity_fixed_point_zeros_and_centre_weight():
    u, q = V.planes(23, 13, 3, "isolated")
    zero = u == 0
    assert zero.sum() >= 10 and (~zero).sum() > 200
    # radius 0 is the identity, whatever the patch
    for Fp in (0, 3):
        assert V.filter_variance(u, q, 0, Fp, 0.45).tobytes() == u.tobytes()
    # a constant plane is a fixed point: every weight is 1 and (n c) / n == c for a dyadic c
    const = np.full((13, 23), 0.375, F32)
    out = V.filter_variance(const, np.full((13, 23), 0.01, F32), 2, 1, 0.45)
    assert out.tobytes() == const.tobytes()
    # u == 0 next to noisy pixels stays exactly 0, and the others are finite and changed by the filter
    out, den = V.filter_variance(u, q, 2, 2, 0.45, want_den=True)
    assert not out[zero].any() and np.isfinite(out).all() and (out[~zero] > 0).all()
    assert (out != u)[~zero].mean() > 0.5
    # the centre weight is 1: the denominator is at least 1, and exactly the centre's where nothing else resembles the pixel
    assert (den >= 1).all()
    lone = np.full((9, 9), 1.0, F32)
    lone[4, 4] = 1000.0
    out, den = V.filter_variance(lone, np.full((9, 9), 1e-6, F32), 2, 0, 0.45, want_den=True)
    assert den[4, 4] == 1 and out[4, 4] == 1000.0


def _pow2_pair(W, H, seed, n=8):
    """a synthetic pair whose every measured pixel has n samples, n a power of two: x * n and x / n are exact"""
    acc, rec = D.synthetic(W, H, seed)
    old = np.maximum(rec["n"], 1).astype(np.float64)
    r = rec.copy()
    seen = rec["n"] > 0
    r["n"] = np.where(seen, n, 0)
    r["sum_y"] = rec["sum_y"] / old * n
    r["sum_y2"] = rec["sum_y2"] / old * n
    a = (acc * (n / old)[..., None]).astype(F32)
    return a, r


def test_denoise_var_against_the_two_older_restatements():
    a, ra = D.synthetic(23, 13, 5)
    b, rb = D.synthetic(23, 13, 6)
    alpha, depth = G.synthetic_features(23, 13, 5)
    feats = [(alpha, 1, 0.1), (depth, 1, 0.2)]
    # no plane: vp_denoise_guided, and nlm() is its loop -- with the records' variance as v it gives that call's filtered pixels
    for f in ([], feats):
        want = G.denoise_guided(a, ra, f, 3, 1, 0.45, guide=b, guide_rec=rb)
        assert V.denoise_var(a, ra, None, 3, 1, 0.45, f, guide=b, guide_rec=rb).tobytes() == want.tobytes()
        c, _ = D.mean_image(a, ra["n"])
        gc, _ = D.mean_image(b, rb["n"])
        v = D.variance(rb)
        rgb, _ = V.nlm(A.luminance(gc), v, c, 3, 1, 0.45, f)
        assert rgb[v != 0].tobytes() == want[v != 0][:, :3].tobytes() and (v != 0).sum() > 100
    # handed variance(rec) * n as the plane, n a power of two: the product round-trips and the call is vp_denoise
    a8, r8 = _pow2_pair(23, 13, 5)
    b8, r8b = _pow2_pair(23, 13, 6)
    for (src, rec, g, grec) in ((a8, r8, None, None), (a8, r8, b8, r8b)):
        gr = rec if grec is None else grec
        vm = D.variance(gr)
        plane = vm * gr["n"].astype(F32)
        _, s = D.mean_image(src, gr["n"])
        assert (plane * s).tobytes() == vm.tobytes() and (vm != 0).sum() > 100 and (vm == 0).sum() >= 10
        want = D.denoise(src, rec, 3, 1, 0.45, guide=g, guide_rec=grec)
        assert V.denoise_var(src, rec, plane, 3, 1, 0.45, guide=g, guide_rec=grec).tobytes() == want.tobytes()
    # a zero plane: every pixel comes back as the plain mean, w as always
    out = V.denoise_var(a, ra, np.zeros((13, 23), F32), 3, 1, 0.45, feats)
    assert out.tobytes() == A.scale_by_count(a, ra["n"], 1.0).tobytes()
    # a plane matters, and an unmeasured guide pixel (n == 0: s = 0) is left alone whatever the plane says
    plane = np.full((13, 23), 4.0, F32)
    out = V.denoise_var(a, ra, plane, 3, 1, 0.45)
    assert out.tobytes() != D.denoise(a, ra, 3, 1, 0.45).tobytes()
    unseen = ra["n"] == 0
    assert unseen.sum() >= 3 and not out[unseen].any() and np.isfinite(out).all()


# ---- the quality rows
@pytest.fixture(scope="module")
def table_scene(oracle):
    osc, oP = A.anchor_oracle(oracle, scenes, SCENE)
    frames = A.oracle_frames(osc, oP)
    h0, h1 = HL.render_halves(A.Stats(A.ANCHOR_W, A.ANCHOR_H), A.Stats(A.ANCHOR_W, A.ANCHOR_H), frames, 0, 16)
    ref = None
    for f in range(1000, 1256):
        ref, _ = osc.render_frame(oP, f, ref)
    return h0, h1, ref / F32(256)


def test_quality_on_sixteen_frames_is_the_recorded_table(table_scene):
    """frames 0..15 against the mean of frames 1000..1255: the cross-filter with the variance stage at (1, 3, 0.45) and with the pooled
    variance alone (the variance pass at radius 0: the identity), for the colour filters (5, 1, 0.45) and (10, 3, 0.45).  The values are
    pinned as measured.  One order is asserted: at (10, 3) the stage's error is at most the plain cross-filter's"""
    h0, h1, ref = table_scene
    r0, r1 = h0.records(), h1.records()
    assert (h0.n == 8).all() and (h1.n == 8).all()
    got = {}
    for name, (R, Fp), var in (("stage 5 1", (5, 1), VAR), ("stage 10 3", (10, 3), VAR), ("pooled 5 1", (5, 1), (0, 3, 0.45)), ("pooled 10 3", (10, 3), (0, 3, 0.45))):
        out, resid, _, _, uf = V.denoise_cross_var(h0.acc, r0, h1.acc, r1, R, Fp, 0.45, variance=var)
        assert np.isfinite(out).all() and np.isfinite(resid).all() and (resid >= 0).all()
        got[name] = D.rel_l2(out, ref)
    got["cross 10 3"] = D.rel_l2(HL.denoise_cross(h0.acc, r0, h1.acc, r1, 10, 3, 0.45)[0], ref)
    print("  ".join("%s %.9f" % kv for kv in got.items()))
    for name, want in (("stage 5 1", STAGE_5_1), ("stage 10 3", STAGE_10_3), ("pooled 5 1", POOLED_5_1), ("pooled 10 3", POOLED_10_3), ("cross 10 3", CROSS_10_3)):
        assert abs(got[name] - want) <= 1e-6 * want, (name, got[name], want)
    assert got["stage 10 3"] <= got["cross 10 3"]
    # a pixel that is a constant in both halves has u == 0, stays 0 through the variance pass and is left unfiltered: resid exactly 0
    u, q = V.halves_variance(r0, r1)
    const = (D.variance(r0) == 0) & (D.variance(r1) == 0)
    assert const.sum() > 100 and not u[const].any() and not uf[const].any() and not resid[const].any()
    assert (uf[~const] > 0).all()


# ---- the CLI
def test_cli_flags_and_refusals():
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--denoise-var", "--denoise-var-radius", "--denoise-var-patch", "--denoise-var-k", "--var-out", "--denoise-cross", "--resid-out"):
        assert flag in r.stdout, flag
    for bad in (["--denoise-var", "--gpus", "2"], ["--denoise-var", "--noise", "0.1"], ["--denoise-var", "--layers-out", "l"], ["--denoise-var", "--over", "0", "0", "0"],
                ["--denoise-var", "--groups-out", "g"], ["--denoise-var", "--sun-gain", "1", "1", "1"], ["--denoise-var", "--planes-out", "p"],
                ["--denoise-var", "--planes-out", "p", "--planes-denoise"], ["--denoise-var", "--denoise-features", "--aa", "2"],
                ["--var-out", "v.hdr"], ["--denoise", "--var-out", "v.hdr"], ["--denoise-cross", "--var-out", "v.hdr"], ["--denoise-var", "--var-out"],
                ["--denoise-var", "--denoise-var-k", "0"], ["--denoise-var", "--denoise-var-k", "x"], ["--denoise-var", "--denoise-var-radius", "11"],
                ["--denoise-var", "--denoise-var-radius", "-1"], ["--denoise-var", "--denoise-var-patch", "4"], ["--denoise-var", "--denoise-var-patch"],
                ["--denoise-var", "--denoise-k", "0"]):
        r = subprocess.run([EXE] + bad, capture_output=True, text=True)
        assert r.returncode == 2, (bad, r.stdout, r.stderr)
    r = subprocess.run([EXE, "--denoise-var", "--noise", "0.1"], capture_output=True, text=True)
    assert "--denoise-cross" in r.stderr and "--noise" in r.stderr
    r = subprocess.run([EXE, "--denoise-cross", "--var-out", "v.hdr"], capture_output=True, text=True)
    assert "--var-out" in r.stderr and "--denoise-var" in r.stderr
    # --denoise-var implies --denoise-cross, which implies --denoise; the variance pass has its own three parameters
    src = open(os.path.join(ROOT, "cuda-volpath_amd", "host", "main.cpp")).read()
    assert re.search(r'a == "--denoise-var"\)\s*denoise_var\s*=\s*denoise_cross\s*=\s*denoise\s*=\s*true', src)
    assert re.search(r"vp_denoise_params\s+dnv\s*=\s*\{1,\s*3,\s*0\.45f\}", src)
