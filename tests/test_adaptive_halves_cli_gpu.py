"""Adaptive sampling on half-buffers in the volpath_render driver (--cross-noise, --cross-noise-out, --plane-cross-noise,
--planes-cross-noise, --plane-cross-noise-out) end to end, in the style of tests/test_cli_modes_gpu.py and with
its scene and its expectation helper: one volpath_render child per case on Julia-32 at 64 x 48, held byte for byte -- every file it
writes -- and line for line -- what it prints that does not depend on time -- to the library calls the flags are documented to make,
made here through the binding."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import test_cli_modes_gpu as CM

pytestmark = pytest.mark.gpu

scene = CM.scene          # the driver's scene, in a context of its own
W, H, NPIX = CM.W, CM.H, CM.NPIX
MODE = {"layers": 1, "groups": 2, "planes": 3}
FLAG = {"layers": "--plane-cross-noise", "groups": "--plane-cross-noise", "planes": "--planes-cross-noise"}
SPP = 16


def _pooled_noise_map(vp, e, name, rec0, rec1, floor):
    """the noise map of two halves' records together: a zeroed scratch copy, both added (vp_accumulate_stats), vp_stats_rel_error"""
    scratch = e.records()
    vp.accumulate_stats(scratch.ptr, rec0.ptr, NPIX)
    vp.accumulate_stats(scratch.ptr, rec1.ptr, NPIX)
    e.noise_map(name, scratch, floor)


def _counts_vary(e, recs, round_frames=4):
    """what keeps a case from passing vacuously: some pixels stop early, some do not, and the rounds were the driver's"""
    res = e.result
    assert 0 < res["samples"] < NPIX * SPP and res["frames_used"] == SPP and res["rounds"] == SPP // round_frames, res
    n = recs[0].download()["n"].astype(np.int64) + recs[1].download()["n"]
    assert len(set(n.ravel().tolist())) >= 2 and n.max() == SPP and int(n.sum()) == res["samples"]


def _beauty(vp, scene, d, out, tol, noise_out=None, resid_out=None, aa=1, round_frames=4):
    e = CM.Expect(vp, scene, d, aa=aa)
    P = e.P
    acc, rec = (e.image(), e.image()), (e.records(), e.records())
    tmp = (e.image(), e.image())
    e.opacity()
    res = vp.render_adaptive_halves(acc[0].ptr, acc[1].ptr, rec[0].ptr, rec[1].ptr, 0, SPP, P, tol, CM.FLOOR, 4, round_frames)
    e.adaptive_line(res, "--cross-noise %g" % tol, round_frames=round_frames)
    resid = vp.lib().vp_malloc(NPIX * 4) if resid_out else None
    vp.denoise_cross(e.disp.ptr, resid, acc[0].ptr, rec[0].ptr, acc[1].ptr, rec[1].ptr, tmp[0].ptr, tmp[1].ptr, W, H, floor_y=CM.FLOOR, **CM.DN)
    e.lines.append("denoised: radius 5, patch 1, k 0.45")
    e.lines.append("  cross-filtered: two half-buffers, each with the other's weights, merged by their counts")
    e.out(out)
    if resid_out:
        m = np.empty((H, W), np.float32)
        vp.lib().vp_download(m.ctypes.data_as(ctypes.c_void_p), resid, NPIX * 4)
        e.write_grey(resid_out, m)
        vp.synchronize()
        vp.lib().vp_free(resid)
    if noise_out:
        _pooled_noise_map(vp, e, noise_out, rec[0], rec[1], CM.FLOOR)
    _counts_vary(e, rec, round_frames)
    return e


def _planes(vp, scene, d, kind, out, tol, prefix, noise_prefix=None, over=None):
    e = CM.Expect(vp, scene, d)
    P, sfx, mode = e.P, CM.PLANES[kind], MODE[kind]
    half = [[(e.image(), e.records()) for _ in sfx] for _ in (0, 1)]
    ptrs = [[(a.ptr, r.ptr) for a, r in h] for h in half]
    e.opacity()
    res = vp.render_adaptive_planes_halves(mode, ptrs[0], ptrs[1], 0, SPP, P, tol, CM.FLOORS[kind], 4, 4)
    e.adaptive_line(res, FLAG[kind] + "".join(" %g" % t for t in tol))
    mean, tmp = [e.image() for _ in sfx], (e.image(), e.image())
    vp.denoise_cross_planes(mode, [m.ptr for m in mean], None, ptrs[0], ptrs[1], tmp[0].ptr, tmp[1].ptr, W, H, **CM.DN)
    for k, name in enumerate(sfx):
        e.write_buf(prefix + name, mean[k])
    m = [b.ptr for b in mean]
    if kind == "layers":
        vp.composite(e.disp.ptr, m[0], m[1], NPIX, 1.0, plate_rgb=over)
    elif kind == "groups":
        vp.relight(e.disp.ptr, m[0], m[1], NPIX, 1.0)
    else:
        vp.relight_composite(e.disp.ptr, m[0], m[1], m[2], NPIX, 1.0, plate_rgb=over or (0.0, 0.0, 0.0))
    e.lines.append("denoised per plane: radius 5, patch 1, k 0.45")
    e.lines.append("  cross-filtered: two halves of every plane, each with the other's weights, merged by their counts")
    e.out(out)
    for k, name in enumerate(sfx if noise_prefix else ()):
        _pooled_noise_map(vp, e, noise_prefix + name, half[0][k][1], half[1][k][1], CM.FLOORS[kind][k])
    _counts_vary(e, (half[0][0][1], half[1][0][1]))
    return e


ROUNDS = ["--min-spp", "4", "--round", "4", "--spp", str(SPP)]
CASES = {
    "cross_noise": (["--cross-noise", "0.3", "--cross-noise-out", "c.hdr", "--resid-out", "r.hdr", "--out", "x.hdr"] + ROUNDS,
                    _beauty, dict(out="x.hdr", tol=0.3, noise_out="c.hdr", resid_out="r.hdr")),
    "cross_noise_aa2": (["--cross-noise", "0.3", "--aa", "2", "--out", "x.ppm"] + ROUNDS,
                        _beauty, dict(out="x.ppm", tol=0.3, aa=2, round_frames=8)),
    "plane_cross_noise_layers": (["--layers-out", "L", "--over", *CM._f(CM.OVER), "--layers-denoise-cross", "--plane-cross-noise", "0.5", "0.2", "--plane-cross-noise-out", "N",
                                  "--out", "x.ppm"] + ROUNDS, _planes, dict(kind="layers", out="x.ppm", tol=(0.5, 0.2), prefix="L", noise_prefix="N", over=CM.OVER)),
    "plane_cross_noise_groups": (["--groups-out", "G", "--groups-denoise-cross", "--plane-cross-noise", "0.5", "0.2", "--out", "x.hdr"] + ROUNDS,
                                 _planes, dict(kind="groups", out="x.hdr", tol=(0.5, 0.2), prefix="G")),
    "planes_cross_noise": (["--planes-out", "P", "--over", *CM._f(CM.OVER), "--planes-denoise-cross", "--planes-cross-noise", "0.3", "0.2", "0.1", "--plane-cross-noise-out", "M",
                            "--out", "x.hdr"] + ROUNDS, _planes, dict(kind="planes", out="x.hdr", tol=(0.3, 0.2, 0.1), prefix="P", noise_prefix="M", over=CM.OVER)),
}


@pytest.mark.parametrize("case", list(CASES))
def test_cli_cross_noise(vp, scene, tmp_path, case):
    flags, expect, kw = CASES[case]
    got_dir, want_dir = tmp_path / "cli", tmp_path / "want"
    got_dir.mkdir()
    want_dir.mkdir()
    argv = [CM.EXE, "--julia", "32", "--size", str(W), str(H)] + flags
    r = subprocess.run(argv, cwd=str(got_dir), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    e = expect(vp, scene, want_dir, **kw)
    try:
        got, want = sorted(os.listdir(str(got_dir))), sorted(os.listdir(str(want_dir)))
        assert got == want, "the files the driver wrote"
        for n in want:
            assert open(os.path.join(str(got_dir), n), "rb").read() == open(os.path.join(str(want_dir), n), "rb").read(), n
        assert [ln for ln in r.stdout.splitlines() if ln.startswith(CM.TIMELESS)] == e.lines
        for n, m in e.maps.items():
            assert np.isfinite(m).all() and (m != 0).any(), n + ": an all-zero map"
        # with --aa 2 the driver says that it rounded --round 4 up to 2 S^2 = 8; otherwise it says nothing
        assert ("--round 4 rounded up to 8" in r.stderr) == (kw.get("aa") == 2), r.stderr
    finally:
        vp.set_subpixel(1)
        e.free()
