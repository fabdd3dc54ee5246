"""GPU suite: the variance stage of the cross-filter (include/volpath.h vp_halves_variance, vp_filter_variance, vp_denoise_var; DESIGN.md
section 2.17).

The three calls are DEFINED to the bit; tests/variance_lib.py restates the definitions in numpy, and every comparison here is
tobytes() equality against it: on uploaded synthetic records and planes, in both forms of the kernels, and behind a half-buffer render
queued on the same stream.  tests/test_variance_cpu.py checks the restatement's own known answers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import adaptive_lib as A
import denoise_guided_lib as G
import denoise_lib as D
import halves_lib as HL
import layers_lib as LL
import scenes
import variance_lib as V

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cuda-volpath_amd", "volpath_render")
F32 = np.float32
NAN_PATTERN = np.uint32(0x7FC12345)
K = 0.45
VAR = (1, 3, 0.45)


@pytest.fixture(autouse=True)
def _restore(vp):
    yield
    vp.set_denoise_form(0)


class Floats:
    """a device plane of one float per pixel"""

    def __init__(self, vp, shape, fill=None):
        self.vp, self.shape = vp, tuple(shape)
        self.n = int(np.prod(self.shape))
        self.ptr = vp.lib().vp_malloc(max(self.n, 1) * 4)
        assert self.ptr
        self.upload(np.full(self.shape, NAN_PATTERN, np.uint32).view(F32) if fill is None else fill)

    def upload(self, arr):
        arr = np.ascontiguousarray(arr, F32)
        assert arr.shape == self.shape
        if arr.nbytes:
            assert self.vp.lib().vp_upload(self.ptr, arr.ctypes.data_as(C.c_void_p), arr.nbytes) == 0

    def poison(self):
        self.upload(np.full(self.shape, NAN_PATTERN, np.uint32).view(F32))

    def download(self):
        out = np.empty(self.shape, F32)
        if out.nbytes:
            assert self.vp.lib().vp_download(out.ctypes.data_as(C.c_void_p), self.ptr, out.nbytes) == 0
        return out

    def free(self):
        self.vp.lib().vp_free(self.ptr)


def _is_poison(arr):
    return (arr.view(np.uint32) == NAN_PATTERN).all()


# ---- 1. vp_halves_variance
@pytest.mark.parametrize("W,H", [(1, 1), (7, 5), (70, 37)])
def test_halves_variance_equals_the_restatement(vp, W, H):
    _, ra = D.synthetic(W, H, 100 + W)
    _, rb = D.synthetic(W, H, 200 + W)
    ra, rb = np.ascontiguousarray(ra, vp.PIXEL_STATS_DTYPE), np.ascontiguousarray(rb, vp.PIXEL_STATS_DTYPE)
    want_u, want_q = V.halves_variance(ra, rb)
    if W > 1:
        assert (ra["n"] < 2).any() and ra["flags"].any() and (want_u == 0).any() and (want_q > 0).any()
    sa, sb = vp.StatsBuffer(W, H), vp.StatsBuffer(W, H)
    du, dq = Floats(vp, (H, W)), Floats(vp, (H, W))
    try:
        sa.upload(ra); sb.upload(rb)
        vp.halves_variance(du.ptr, dq.ptr, sa.ptr, sb.ptr, W * H)
        assert du.download().tobytes() == want_u.tobytes() and dq.download().tobytes() == want_q.tobytes()
        # without d_q: u alone, q's buffer untouched
        du.poison(); dq.poison()
        vp.halves_variance(du.ptr, None, sa.ptr, sb.ptr, W * H)
        assert du.download().tobytes() == want_u.tobytes() and _is_poison(dq.download())
        # the roles swapped: the same plane (0.5 * (a + b) and (a - b)^2 are symmetric)
        vp.halves_variance(du.ptr, dq.ptr, sb.ptr, sa.ptr, W * H)
        assert du.download().tobytes() == want_u.tobytes() and dq.download().tobytes() == want_q.tobytes()
        # size 0: nothing is written
        du.poison(); dq.poison()
        vp.halves_variance(du.ptr, dq.ptr, sa.ptr, sb.ptr, 0)
        assert _is_poison(du.download()) and _is_poison(dq.download())
        assert sa.download().tobytes() == ra.tobytes() and sb.download().tobytes() == rb.tobytes()
    finally:
        for b in (sa, sb, du, dq):
            b.free()


# ---- 2. vp_filter_variance
_memo = {}


def _planes(W, H, kind):
    key = (W, H, kind)
    if key not in _memo:
        _memo[key] = V.planes(W, H, 300 + W, kind)
    return _memo[key]


def _want_filtered(W, H, kind, R, Fp):
    """the restatement's answer, computed once and never changed"""
    key = (W, H, kind, R, Fp)
    if key not in _memo:
        u, q = _planes(W, H, kind)
        out = V.filter_variance(u, q, R, Fp, K)
        out.setflags(write=False)
        _memo[key] = out
    return _memo[key]


@pytest.mark.parametrize("R,Fp", [(0, 0), (1, 3), (2, 2), (10, 3)])
@pytest.mark.parametrize("W,H", [(1, 1), (7, 5), (33, 9), (70, 37)])
def test_filter_variance_equals_the_restatement_in_both_forms(vp, W, H, R, Fp):
    du, dq, dst = Floats(vp, (H, W)), Floats(vp, (H, W)), Floats(vp, (H, W))
    try:
        for kind in ("block", "isolated"):
            u, q = _planes(W, H, kind)
            want = _want_filtered(W, H, kind, R, Fp)
            if (W, H) == (70, 37):
                assert not u[8:24, 32:64].any() if kind == "block" else ((u == 0).sum() > 100 and (u[8:16, 32:64] != 0).any())
                assert (u != 0).sum() > 1000 and (R == 0 or (want != u).sum() > 1000)
            du.upload(u); dq.upload(q)
            out = {}
            for form in (1, 0):
                vp.set_denoise_form(form)
                dst.poison()
                vp.filter_variance(dst.ptr, du.ptr, dq.ptr, W, H, R, Fp, K)
                assert vp.last_denoise_form() == form
                out[form] = dst.download()
                assert not np.isnan(out[form]).any()                    # a NaN-filled dst is fully overwritten
            assert out[0].tobytes() == out[1].tobytes(), (kind, "form 1 == form 0")
            assert out[0].tobytes() == want.tobytes(), kind
            assert not out[0][u == 0].any()
            if R == 0:
                assert out[0].tobytes() == u.tobytes()
            assert du.download().tobytes() == u.tobytes() and dq.download().tobytes() == q.tobytes()
    finally:
        for b in (du, dq, dst):
            b.free()


# ---- 3. vp_denoise_var
class Pair:
    """a synthetic (accumulator, records) pair on the device"""

    def __init__(self, vp, W, H, seed):
        self.acc, rec = D.synthetic(W, H, seed)
        self.rec = np.ascontiguousarray(rec, vp.PIXEL_STATS_DTYPE)
        self.buf, self.stats = vp.DeviceBuffer(W, H), vp.StatsBuffer(W, H)
        self.buf.upload(self.acc)
        self.stats.upload(self.rec)

    def free(self):
        self.buf.free(); self.stats.free()


def test_denoise_var_equals_the_restatement(vp):
    W, H = 70, 37
    s, g = Pair(vp, W, H, 170), Pair(vp, W, H, 8)
    alpha, depth = G.synthetic_features(W, H, 170)
    feats2 = [(alpha, 1, 0.1), (depth, 1, 0.2)]
    # a per-sample variance plane of the size of what the records say, with a zero block over a whole tile and isolated zeros
    plane, _ = V.halves_variance(s.rec, g.rec)
    plane[8:24, 32:64] = 0
    assert (plane != 0).sum() > 1000 and (plane == 0).sum() > 512
    da, dd, dst = vp.DeviceBuffer(W, H), vp.DeviceBuffer(W, H), vp.DeviceBuffer(W, H)
    dplane = Floats(vp, (H, W), plane)
    nan = np.full((H, W, 4), NAN_PATTERN, np.uint32).view(F32)
    try:
        da.upload(alpha); dd.upload(depth)
        dev_feats2 = [(da.ptr, 1, 0.1), (dd.ptr, 1, 0.2)]
        for form in (0, 1):
            vp.set_denoise_form(form)
            # a NULL plane: vp_denoise_guided's bytes, with features and without
            for hf, df in (([], []), (feats2, dev_feats2)):
                dst.upload(nan)
                vp.denoise_var(dst.ptr, s.buf.ptr, s.stats.ptr, W, H, None, df, 5, 1, K, guide_ptr=g.buf.ptr, guide_stats_ptr=g.stats.ptr)
                got = dst.download()
                dst.upload(nan)
                vp.denoise_guided(dst.ptr, s.buf.ptr, s.stats.ptr, W, H, df, 5, 1, K, guide_ptr=g.buf.ptr, guide_stats_ptr=g.stats.ptr)
                assert got.tobytes() == dst.download().tobytes(), (form, len(hf))
            # a plane, a separate guide pair and guide == src, no feature and two, the CLI's window and the paper's
            for (R, Fp) in ((5, 1), (10, 3)):
                for hf, df in (([], []), (feats2, dev_feats2)):
                    for guide in (g, None):
                        kw = dict(guide_ptr=guide.buf.ptr, guide_stats_ptr=guide.stats.ptr) if guide else {}
                        hkw = dict(guide=guide.acc, guide_rec=guide.rec) if guide else {}
                        key = ("var", R, Fp, len(hf), guide is not None)
                        if key not in _memo:
                            _memo[key] = V.denoise_var(s.acc, s.rec, plane, R, Fp, K, hf, **hkw)
                        want = _memo[key]
                        dst.upload(nan)
                        vp.denoise_var(dst.ptr, s.buf.ptr, s.stats.ptr, W, H, dplane.ptr, df, R, Fp, K, **kw)
                        assert vp.last_denoise_form() == form
                        got = dst.download()
                        assert not np.isnan(got).any()
                        assert got.tobytes() == want.tobytes(), (form, R, Fp, len(hf), guide is not None)
                        # the zero block comes back as the plain mean
                        mean = A.scale_by_count(s.acc, s.rec["n"], 1.0)
                        assert got[8:24, 32:64].tobytes() == mean[8:24, 32:64].tobytes()
            assert _memo[("var", 5, 1, 0, True)].tobytes() != _memo[("var", 5, 1, 0, False)].tobytes()
            assert _memo[("var", 5, 1, 0, True)].tobytes() != _memo[("var", 5, 1, 2, True)].tobytes()
        assert s.buf.download().tobytes() == s.acc.tobytes() and g.stats.download().tobytes() == g.rec.tobytes()
        assert dplane.download().tobytes() == plane.tobytes()
    finally:
        for b in (s, g, da, dd, dst, dplane):
            b.free()


# ---- 4. the pipeline behind a render, on one stream
@pytest.fixture
def ctx(vp):
    c = vp.Context(0)
    try:
        with c:
            yield c
    finally:
        c.destroy()


def _scene(vp, oracle, est=0, rng_mode=2):
    vp.init_volume(LL.grid_of("julia", oracle), brick=1, linear=True)
    vp.init_envmap(LL.ENV)
    vp.set_sun(scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER)
    vp.set_camera()
    vp.set_estimator(est)
    vp.set_rng(rng_mode, LL.KEY)
    vp.set_shard(0, 1)
    return vp.make_param(LL.W, LL.H, **LL.param_kw("julia"))


def test_the_pipeline_equals_the_restatement(vp, oracle, ctx):
    """vp_render_frames_halves_stats and the five calls of the stage queued back to back on the 16 x 12 Julia-32 view of layers_lib,
    against the restatement fed with the oracle's frames"""
    W, H, R, Fp = LL.W, LL.H, 3, 1
    osc = oracle.OracleScene(LL.grid_of("julia", oracle), LL.ENV, scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER, estimator=0, rng_mode=2, seed=LL.KEY)
    oP = oracle.default_param(W, H, **LL.JULIA_KW)
    h0, h1 = HL.render_halves(A.Stats(W, H), A.Stats(W, H), lambda f: osc.render_samples(oP, f)[0], 0, 16)
    r0, r1 = h0.records(), h1.records()
    want, want_resid, wa, wb, wuf = V.denoise_cross_var(h0.acc, r0, h1.acc, r1, R, Fp, K, variance=VAR)
    assert (wuf != 0).sum() > 20 and want_resid.max() > 0
    assert want.tobytes() != HL.denoise_cross(h0.acc, r0, h1.acc, r1, R, Fp, K)[0].tobytes()          # the stage matters on this render
    P = _scene(vp, oracle)
    acc = (vp.DeviceBuffer(W, H), vp.DeviceBuffer(W, H))
    rec = (vp.StatsBuffer(W, H), vp.StatsBuffer(W, H))
    ta, tb, dst, plain = (vp.DeviceBuffer(W, H) for _ in range(4))
    du, dq, duf, res = (Floats(vp, (H, W)) for _ in range(4))
    try:
        vp.render_frames(plain.ptr, 0, 2, P)
        frames_before = plain.download()
        # queued back to back: nothing waits in between
        vp.render_frames_halves_stats(acc[0].ptr, acc[1].ptr, rec[0].ptr, rec[1].ptr, 0, 16, P)
        vp.halves_variance(du.ptr, dq.ptr, rec[0].ptr, rec[1].ptr, W * H)
        vp.filter_variance(duf.ptr, du.ptr, dq.ptr, W, H, *VAR)
        vp.denoise_var(ta.ptr, acc[0].ptr, rec[0].ptr, W, H, duf.ptr, (), R, Fp, K, guide_ptr=acc[1].ptr, guide_stats_ptr=rec[1].ptr)
        vp.denoise_var(tb.ptr, acc[1].ptr, rec[1].ptr, W, H, duf.ptr, (), R, Fp, K, guide_ptr=acc[0].ptr, guide_stats_ptr=rec[0].ptr)
        vp.merge_halves(dst.ptr, res.ptr, ta.ptr, rec[0].ptr, tb.ptr, rec[1].ptr, W * H, 1e-3)
        got = dst.download()
        assert acc[0].download().tobytes() == h0.acc.tobytes() and acc[1].download().tobytes() == h1.acc.tobytes()
        assert rec[0].download().tobytes() == np.ascontiguousarray(r0, vp.PIXEL_STATS_DTYPE).tobytes()
        wu, wq = V.halves_variance(r0, r1)
        assert du.download().tobytes() == wu.tobytes() and dq.download().tobytes() == wq.tobytes() and duf.download().tobytes() == wuf.tobytes()
        assert ta.download().tobytes() == wa.tobytes() and tb.download().tobytes() == wb.tobytes()
        assert got.tobytes() == want.tobytes() and res.download().tobytes() == want_resid.tobytes()
        # the helper: the same calls
        for form in (0, 1):
            vp.set_denoise_form(form)
            for b in (ta, tb, dst):
                b.reset()
            for b in (du, dq, duf, res):
                b.poison()
            vp.denoise_cross(dst.ptr, res.ptr, acc[0].ptr, rec[0].ptr, acc[1].ptr, rec[1].ptr, ta.ptr, tb.ptr, W, H, R, Fp, K, variance=VAR,
                             var_ptrs=(du.ptr, dq.ptr, duf.ptr))
            assert dst.download().tobytes() == want.tobytes() and res.download().tobytes() == want_resid.tobytes(), form
            assert duf.download().tobytes() == wuf.tobytes()
        vp.set_denoise_form(0)
        # vp_render_frames afterwards: the bytes it gave before
        plain.reset()
        vp.render_frames(plain.ptr, 0, 2, P)
        assert plain.download().tobytes() == frames_before.tobytes()
    finally:
        for b in acc + rec + (ta, tb, dst, plain, du, dq, duf, res):
            b.free()


# ---- 5. the CLI
def test_cli_denoise_var_equals_the_library_calls(vp, tmp_path):
    """volpath_render --denoise-var --var-out against the same calls made here in the driver's scene: --out and the filtered variance
    plane, each written by volpath.host.write_image (the driver's Image::dump_hdr), byte for byte"""
    from volpath import host
    W, H, spp = 64, 48, 8
    got_dir, want_dir = tmp_path / "cli", tmp_path / "want"
    got_dir.mkdir()
    want_dir.mkdir()
    r = subprocess.run([EXE, "--julia", "32", "--size", str(W), str(H), "--spp", str(spp), "--batch", "8", "--denoise-var", "--var-out", "v.hdr", "--out", "x.hdr"],
                       cwd=str(got_dir), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "  cross-filtered: two half-buffers" in r.stdout and "  variance: pooled from both halves, filtered at radius 1, patch 3, k 0.45" in r.stdout
    env, sun_dir, sun_power = host.bake_sunsky(0.5, 0.2)
    c = vp.Context(0)
    try:
        with c:
            vp.init_volume(vp.julia_volume(32), brick=1, linear=True)
            vp.init_envmap(env)
            vp.set_sun(sun_dir, sun_power)
            vp.set_camera(host.camera_matrix())
            vp.set_estimator(vp.EST_DECOMP)
            vp.set_rng(vp.RNG_SAMPLERH, (0x9E3779B9, 0x85EBCA6B))
            vp.set_shard(0, 1)
            P = vp.make_param(W, H)
            acc = (vp.DeviceBuffer(W, H), vp.DeviceBuffer(W, H))
            rec = (vp.StatsBuffer(W, H), vp.StatsBuffer(W, H))
            ta, tb, dst = (vp.DeviceBuffer(W, H) for _ in range(3))
            du, dq, duf = (Floats(vp, (H, W)) for _ in range(3))
            try:
                vp.render_frames_halves_stats(acc[0].ptr, acc[1].ptr, rec[0].ptr, rec[1].ptr, 0, spp, P)
                vp.denoise_cross(dst.ptr, None, acc[0].ptr, rec[0].ptr, acc[1].ptr, rec[1].ptr, ta.ptr, tb.ptr, W, H, 5, 1, K, floor_y=1e-3, variance=VAR,
                                 var_ptrs=(du.ptr, dq.ptr, duf.ptr))
                img, uf = dst.download(), duf.download()
            finally:
                for b in acc + rec + (ta, tb, dst, du, dq, duf):
                    b.free()
    finally:
        c.destroy()
    assert (uf > 0).sum() > 100 and np.isfinite(uf).all()
    grey = np.ones((H, W, 4), F32)
    grey[..., :3] = uf[..., None]
    host.write_image(img, str(want_dir / "x.hdr"), hdr=True)
    host.write_image(grey, str(want_dir / "v.hdr"), hdr=True)
    assert sorted(os.listdir(str(got_dir))) == ["v.hdr", "x.hdr"]
    for n in ("x.hdr", "v.hdr"):
        assert open(str(got_dir / n), "rb").read() == open(str(want_dir / n), "rb").read(), n
