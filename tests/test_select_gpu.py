"""GPU suite: per-pixel filter selection from cross-buffer error estimates (include/volpath.h vp_cross_error, vp_select; DESIGN.md
section 2.18).

Both calls are DEFINED to the bit; tests/select_lib.py restates the definitions in numpy, and every comparison here is tobytes()
equality against it: on uploaded synthetic halves, images and error planes, in both forms of the selection kernel, and behind a
half-buffer render queued on the same stream.  tests/test_select_cpu.py checks the restatement's own known answers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import adaptive_lib as A
import denoise_lib as D
import halves_lib as HL
import layers_lib as LL
import scenes
import select_lib as S

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


class Plane:
    """a device array of one dtype: float planes (NaN-filled unless given), float4 images, index bytes (0xA5-filled)"""

    def __init__(self, vp, shape, fill=None, dtype=F32):
        self.vp, self.shape, self.dtype = vp, tuple(shape), np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        self.ptr = vp.lib().vp_malloc(max(self.nbytes, 4))
        assert self.ptr
        if fill is None:
            self.poison()
        else:
            self.upload(fill)

    def poison_value(self):
        return np.full(self.shape, NAN_PATTERN, np.uint32).view(F32) if self.dtype == F32 else np.full(self.shape, 0xA5, self.dtype)

    def poison(self):
        self.upload(self.poison_value())

    def upload(self, arr):
        arr = np.ascontiguousarray(arr, self.dtype)
        assert arr.shape == self.shape
        if arr.nbytes:
            assert self.vp.lib().vp_upload(self.ptr, arr.ctypes.data_as(C.c_void_p), arr.nbytes) == 0

    def download(self):
        out = np.empty(self.shape, self.dtype)
        if out.nbytes:
            assert self.vp.lib().vp_download(out.ctypes.data_as(C.c_void_p), self.ptr, out.nbytes) == 0
        return out

    def is_poison(self):
        return self.download().tobytes() == self.poison_value().tobytes()

    def free(self):
        self.vp.lib().vp_free(self.ptr)


# ---- 1. vp_cross_error
@pytest.mark.parametrize("W,H", [(1, 1), (7, 5), (70, 37)])
def test_cross_error_equals_the_restatement(vp, W, H):
    h0, r0 = D.synthetic(W, H, 100 + W)
    h1, r1 = D.synthetic(W, H, 200 + W)
    r0, r1 = np.ascontiguousarray(r0, vp.PIXEL_STATS_DTYPE), np.ascontiguousarray(r1, vp.PIXEL_STATS_DTYPE)
    # "filtered" halves: the means, moved a little, with a w that must not matter
    rng = np.random.default_rng(W)
    fa = (A.scale_by_count(h0, r0["n"], 1.0) * rng.uniform(0.8, 1.2, (H, W, 1))).astype(F32)
    fb = (A.scale_by_count(h1, r1["n"], 1.0) * rng.uniform(0.8, 1.2, (H, W, 1))).astype(F32)
    want = S.cross_error(fa, fb, h0, r0, h1, r1)
    if W == 70:
        few = (r0["n"] < 2) | (r1["n"] < 2)
        assert (r0["n"] == 0).any() and r0["flags"].any() and few.any() and not want[few].any() and (D.variance(r0) == 0).sum() >= 2
        assert (want < 0).any() and (want > 0).any()
    bufs = [vp.DeviceBuffer(W, H) for _ in range(4)]
    stats = [vp.StatsBuffer(W, H), vp.StatsBuffer(W, H)]
    err = Plane(vp, (H, W))
    try:
        for b, a in zip(bufs, (fa, fb, h0, h1)):
            b.upload(a)
        stats[0].upload(r0); stats[1].upload(r1)
        vp.cross_error(err.ptr, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, stats[0].ptr, bufs[3].ptr, stats[1].ptr, W * H)
        got = err.download()
        assert not np.isnan(got).any() and got.tobytes() == want.tobytes()
        # the roles of the halves swapped: 0.5f * (ea + eb) is symmetric
        err.poison()
        vp.cross_error(err.ptr, bufs[1].ptr, bufs[0].ptr, bufs[3].ptr, stats[1].ptr, bufs[2].ptr, stats[0].ptr, W * H)
        assert err.download().tobytes() == want.tobytes()
        # size 0: nothing is written
        err.poison()
        vp.cross_error(err.ptr, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, stats[0].ptr, bufs[3].ptr, stats[1].ptr, 0)
        assert err.is_poison()
        for b, a in zip(bufs, (fa, fb, h0, h1)):
            assert b.download().tobytes() == a.tobytes()
        assert stats[0].download().tobytes() == r0.tobytes() and stats[1].download().tobytes() == r1.tobytes()
    finally:
        for b in bufs + stats + [err]:
            b.free()


# ---- 2. vp_select
_memo = {}


def _inputs(W, H, kind):
    key = (W, H, kind)
    if key not in _memo:
        imgs = S.images_for(W, H, 4, 400 + W)
        errs = S.error_planes(W, H, 4, 500 + W, kind)
        for a in imgs + errs:
            a.setflags(write=False)
        _memo[key] = (imgs, errs)
    return _memo[key]


def _want(W, H, kind, n, Rs, Rb):
    """the restatement's answer, computed once and never changed; candidates n of the four, the LAST n so that the block's winner is among them"""
    key = (W, H, kind, n, Rs, Rb)
    if key not in _memo:
        imgs, errs = _inputs(W, H, kind)
        dst, k = S.select(imgs[4 - n:], errs[4 - n:], Rs, Rb)
        dst.setflags(write=False); k.setflags(write=False)
        _memo[key] = (dst, k)
    return _memo[key]


@pytest.mark.parametrize("Rs,Rb", [(0, 0), (1, 1), (3, 0), (0, 3), (3, 3)])
@pytest.mark.parametrize("W,H", [(1, 1), (7, 5), (33, 9), (70, 37)])
def test_select_equals_the_restatement_in_both_forms(vp, W, H, Rs, Rb):
    dimg = [vp.DeviceBuffer(W, H) for _ in range(4)]
    derr = [Plane(vp, (H, W)) for _ in range(4)]
    dst, idx = vp.DeviceBuffer(W, H), Plane(vp, (H, W), dtype=np.uint8)
    nan = np.full((H, W, 4), NAN_PATTERN, np.uint32).view(F32)
    try:
        for kind in ("noise", "ties", "block"):
            imgs, errs = _inputs(W, H, kind)
            for b, a in zip(dimg + derr, imgs + errs):
                b.upload(a)
            for n in (1, 2, 4):
                want, want_k = _want(W, H, kind, n, Rs, Rb)
                ip, ep = [b.ptr for b in dimg[4 - n:]], [b.ptr for b in derr[4 - n:]]
                if (W, H) == (70, 37) and n > 1:
                    if kind == "block":     # one candidate wins whole tiles (rows 0..23, columns 32..63 are tiles of their own), and the picks mix elsewhere
                        assert (want_k[0:24, 32:64] == n - 1).all() and want[0:24 - Rb, 32 + Rb:64].tobytes() == imgs[3][0:24 - Rb, 32 + Rb:64].tobytes()
                        assert len(np.unique(want_k)) == n
                    if kind == "ties":      # exact ties of the smoothed errors go to the lowest index
                        E = [S.smooth_error(e, Rs) for e in errs[4 - n:]]
                        assert ((E[0] == E[1]) & (want_k == 0)).sum() > 100
                    if kind == "noise":
                        assert all((e < 0).sum() > 1000 for e in errs) and len(np.unique(want_k)) == n
                out = {}
                for form in (1, 0):
                    vp.set_denoise_form(form)
                    dst.upload(nan); idx.poison()
                    vp.select(dst.ptr, idx.ptr, ip, ep, W, H, Rs, Rb)
                    assert vp.last_denoise_form() == form
                    out[form] = (dst.download(), idx.download())
                    assert not np.isnan(out[form][0]).any()                     # a NaN-filled dst is fully overwritten
                assert out[0][1].tobytes() == out[1][1].tobytes() and out[0][0].tobytes() == out[1][0].tobytes(), (kind, n, "form 1 == form 0")
                assert out[0][1].tobytes() == want_k.tobytes(), (kind, n)
                assert out[0][0].tobytes() == want.tobytes(), (kind, n)
                if n == 1:
                    assert out[0][0].tobytes() == imgs[3].tobytes()
            # without d_index: the same image, the index buffer untouched; dst == images[0]: the same image again
            want, _ = _want(W, H, kind, 2, Rs, Rb)
            ip, ep = [b.ptr for b in dimg[2:]], [b.ptr for b in derr[2:]]
            for form in (0, 1):
                vp.set_denoise_form(form)
                dst.upload(nan); idx.poison()
                vp.select(dst.ptr, None, ip, ep, W, H, Rs, Rb)
                assert dst.download().tobytes() == want.tobytes() and idx.is_poison()
                dimg[2].upload(imgs[2])
                vp.select(dimg[2].ptr, idx.ptr, ip, ep, W, H, Rs, Rb)
                assert dimg[2].download().tobytes() == want.tobytes(), (kind, form, "in place")
                dimg[2].upload(imgs[2])
            for b, a in zip(dimg + derr, imgs + errs):
                assert b.download().tobytes() == a.tobytes()
    finally:
        for b in dimg + derr + [dst, idx]:
            b.free()


# ---- 3. the pipeline behind a render, on one stream
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
    """vp_render_frames_halves_stats and volpath.denoise_select queued back to back on the 16 x 12 Julia-32 view of layers_lib, in both
    forms, against the restatement fed with the oracle's frames; vp_render_frames gives the same bytes before and after"""
    W, H = LL.W, LL.H
    cands = ((2, 1, K), (4, 2, K))
    osc = oracle.OracleScene(LL.grid_of("julia", oracle), LL.ENV, scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER, estimator=0, rng_mode=2, seed=LL.KEY)
    oP = oracle.default_param(W, H, **LL.JULIA_KW)
    h0, h1 = HL.render_halves(A.Stats(W, H), A.Stats(W, H), lambda f: osc.render_samples(oP, f)[0], 0, 16)
    r0, r1 = h0.records(), h1.records()
    want = S.denoise_select(h0.acc, r0, h1.acc, r1, cands, 1, 1, VAR)
    assert len(np.unique(want["index"])) == 2 and all((e != 0).sum() > 20 for e in want["errors"])      # both candidates win somewhere on this render
    assert all(want["dst"].tobytes() != i.tobytes() for i in want["images"])
    P = _scene(vp, oracle)
    acc = (vp.DeviceBuffer(W, H), vp.DeviceBuffer(W, H))
    rec = (vp.StatsBuffer(W, H), vp.StatsBuffer(W, H))
    ta, tb, dst, plain, i0, i1 = (vp.DeviceBuffer(W, H) for _ in range(6))
    du, dq, duf, e0, e1 = (Plane(vp, (H, W)) for _ in range(5))
    idx = Plane(vp, (H, W), dtype=np.uint8)
    try:
        vp.render_frames(plain.ptr, 0, 2, P)
        frames_before = plain.download()
        for form in (0, 1):
            vp.set_denoise_form(form)
            for b in acc + rec + (ta, tb, dst, i0, i1):
                b.reset()
            for b in (du, dq, duf, e0, e1, idx):
                b.poison()
            # queued back to back: nothing waits in between
            vp.render_frames_halves_stats(acc[0].ptr, acc[1].ptr, rec[0].ptr, rec[1].ptr, 0, 16, P)
            vp.denoise_select(dst.ptr, idx.ptr, acc[0].ptr, rec[0].ptr, acc[1].ptr, rec[1].ptr, W, H, candidates=cands, smooth=1, blend=1, variance=VAR,
                              var_ptrs=(du.ptr, dq.ptr, duf.ptr), tmp=(ta.ptr, tb.ptr, (i0.ptr, i1.ptr), (e0.ptr, e1.ptr)))
            got = dst.download()
            assert vp.last_denoise_form() == form
            assert acc[0].download().tobytes() == h0.acc.tobytes() and acc[1].download().tobytes() == h1.acc.tobytes()
            assert rec[0].download().tobytes() == np.ascontiguousarray(r0, vp.PIXEL_STATS_DTYPE).tobytes()
            assert duf.download().tobytes() == want["uf"].tobytes()
            for b, w in ((e0, want["errors"][0]), (e1, want["errors"][1]), (i0, want["images"][0]), (i1, want["images"][1])):
                assert b.download().tobytes() == w.tobytes(), form
            assert idx.download().tobytes() == want["index"].tobytes() and got.tobytes() == want["dst"].tobytes(), form
        vp.set_denoise_form(0)
        # vp_render_frames afterwards: the bytes it gave before
        plain.reset()
        vp.render_frames(plain.ptr, 0, 2, P)
        assert plain.download().tobytes() == frames_before.tobytes()
    finally:
        for b in acc + rec + (ta, tb, dst, plain, i0, i1, du, dq, duf, e0, e1, idx):
            b.free()


# ---- 4. the CLI
def test_cli_denoise_select_equals_the_library_calls(vp, tmp_path):
    """volpath_render --denoise-select --select-out against the same calls made here in the driver's scene: --out and the index map, each
    written by volpath.host.write_image (the driver's Image::dump_hdr), byte for byte"""
    from volpath import host
    W, H, spp = 64, 48, 8
    got_dir, want_dir = tmp_path / "cli", tmp_path / "want"
    got_dir.mkdir()
    want_dir.mkdir()
    r = subprocess.run([EXE, "--julia", "32", "--size", str(W), str(H), "--spp", str(spp), "--batch", "8", "--denoise-select", "--denoise-radius", "2",
                        "--denoise-select-radius", "5", "--denoise-select-patch", "2", "--select-out", "s.hdr", "--out", "x.hdr"],
                       cwd=str(got_dir), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "  variance: pooled from both halves, filtered at radius 1, patch 3, k 0.45" in r.stdout
    assert "  selected per pixel against radius 5, patch 2: errors smoothed at radius 1, picks blended at radius 1" in r.stdout
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
            ta, tb, dst, i0, i1 = (vp.DeviceBuffer(W, H) for _ in range(5))
            du, dq, duf, e0, e1 = (Plane(vp, (H, W)) for _ in range(5))
            idx = Plane(vp, (H, W), dtype=np.uint8)
            try:
                vp.render_frames_halves_stats(acc[0].ptr, acc[1].ptr, rec[0].ptr, rec[1].ptr, 0, spp, P)
                vp.denoise_select(dst.ptr, idx.ptr, acc[0].ptr, rec[0].ptr, acc[1].ptr, rec[1].ptr, W, H, candidates=((2, 1, K), (5, 2, K)),
                                  var_ptrs=(du.ptr, dq.ptr, duf.ptr), tmp=(ta.ptr, tb.ptr, (i0.ptr, i1.ptr), (e0.ptr, e1.ptr)))
                img, index = dst.download(), idx.download()
            finally:
                for b in acc + rec + (ta, tb, dst, i0, i1, du, dq, duf, e0, e1, idx):
                    b.free()
    finally:
        c.destroy()
    assert index.max() <= 1 and (index == 0).any()
    grey = np.repeat(index.astype(F32)[..., None], 4, -1)
    host.write_image(img, str(want_dir / "x.hdr"), hdr=True)
    host.write_image(grey, str(want_dir / "s.hdr"), hdr=True)
    assert sorted(os.listdir(str(got_dir))) == ["s.hdr", "x.hdr"]
    for n in ("x.hdr", "s.hdr"):
        assert open(str(got_dir / n), "rb").read() == open(str(want_dir / n), "rb").read(), n
