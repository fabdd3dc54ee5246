"""The cross-filter on planes in the volpath_render driver (--layers-denoise-cross, --groups-denoise-cross, --planes-denoise-cross,
--plane-denoise-var, --plane-resid-out) end to end, in the style of tests/test_cli_modes_gpu.py and with its
scene and its expectation helper: one volpath_render child per case on Julia-32 at 64 x 48, held byte for byte -- the plane files, --out
and the residual maps -- to the library calls the flag is documented to make, made here through the binding."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import test_cli_modes_gpu as CM

pytestmark = pytest.mark.gpu

scene = CM.scene          # the driver's scene, in a context of its own
W, H, NPIX = CM.W, CM.H, CM.NPIX
MODE = {"layers": 1, "groups": 2, "planes": 3}
TIMELESS = ("wrote ", "denoised", "  cross-filtered", "  variance")
VAR = (1, 3, 0.45)


def _cross(vp, scene, d, kind, out, prefix=None, over=None, sun_gain=(1.0, 1.0, 1.0), sky_gain=(1.0, 1.0, 1.0), variance=False, resid_prefix=None, spp=8):
    e = CM.Expect(vp, scene, d)
    P, sfx, mode = e.P, CM.PLANES[kind], MODE[kind]
    half = [[(e.image(), e.records()) for _ in sfx] for _ in (0, 1)]
    ptrs = [[(a.ptr, r.ptr) for a, r in h] for h in half]
    vp.render_frames_planes_halves_stats(mode, ptrs[0], ptrs[1], 0, spp, P)
    mean, tmp = [e.image() for _ in sfx], (e.image(), e.image())
    resid = [vp.lib().vp_malloc(NPIX * 4) for _ in sfx] if resid_prefix else None
    var = [vp.lib().vp_malloc(NPIX * 4) for _ in range(3)] if variance else None
    vp.denoise_cross_planes(mode, [m.ptr for m in mean], resid, ptrs[0], ptrs[1], tmp[0].ptr, tmp[1].ptr, W, H, variance=VAR if variance else None, var_ptrs=var, **CM.DN)
    assert [vp.PLANE_RESID_FLOOR[vp.PLANE_NAMES[mode][k]] for k in range(len(sfx))] == list(CM.FLOORS[kind])
    for k, name in enumerate(sfx if resid_prefix else ()):
        m = np.empty((H, W), np.float32)
        vp.lib().vp_download(m.ctypes.data_as(ctypes.c_void_p), resid[k], NPIX * 4)
        e.write_grey(resid_prefix + name, m)
    vp.synchronize()
    for p in (resid or []) + (var or []):
        vp.lib().vp_free(p)
    for k, name in enumerate(sfx if prefix else ()):
        e.write_buf(prefix + name, mean[k])
    m = [b.ptr for b in mean]
    if kind == "layers" and over is not None:
        vp.composite(e.disp.ptr, m[0], m[1], NPIX, 1.0, plate_rgb=over)
    elif kind == "groups":
        vp.relight(e.disp.ptr, m[0], m[1], NPIX, 1.0, sun_gain, sky_gain)
    elif kind == "planes":
        vp.relight_composite(e.disp.ptr, m[0], m[1], m[2], NPIX, 1.0, sun_gain, sky_gain, plate_rgb=over or (0.0, 0.0, 0.0))
    e.lines.append("denoised per plane: radius 5, patch 1, k 0.45")
    e.lines.append("  cross-filtered: two halves of every plane, each with the other's weights, merged by their counts")
    if variance:
        e.lines.append("  variance: pooled from both halves of a plane, filtered at radius 1, patch 3, k 0.45")
    if kind != "layers" or over is not None:
        e.out(out)
    # what the self-guided filter of the mode's -denoise flag gives is something else
    own = vp.DeviceBuffer(W, H)
    try:
        vp.denoise(own.ptr, half[0][0][0].ptr, half[0][0][1].ptr, W, H, **CM.DN)
        assert own.download().tobytes() != mean[0].download().tobytes()
    finally:
        own.free()
    e.halves = [[(a.download(), r.download()) for a, r in h] for h in half]
    return e


CASES = {
    "layers_cross": (["--layers-out", "L", "--over", *CM._f(CM.OVER), "--layers-denoise-cross", "--out", "x.ppm"],
                     dict(kind="layers", out="x.ppm", prefix="L", over=CM.OVER)),
    "groups_cross": (["--groups-out", "G", "--sun-gain", *CM._f(CM.GAINS["sun_gain"]), "--sky-gain", *CM._f(CM.GAINS["sky_gain"]), "--groups-denoise-cross", "--out", "x.hdr"],
                     dict(kind="groups", out="x.hdr", prefix="G", **CM.GAINS)),
    "planes_cross": (["--planes-out", "P", "--sun-gain", *CM._f(CM.GAINS["sun_gain"]), "--over", *CM._f(CM.OVER), "--out", "x.hdr", "--planes-denoise-cross"],
                     dict(kind="planes", out="x.hdr", prefix="P", over=CM.OVER, sun_gain=CM.GAINS["sun_gain"])),
    "planes_cross_var_resid": (["--planes-out", "P", "--over", *CM._f(CM.OVER), "--out", "x.hdr", "--planes-denoise-cross", "--plane-denoise-var", "--plane-resid-out", "R"],
                               dict(kind="planes", out="x.hdr", prefix="P", over=CM.OVER, variance=True, resid_prefix="R")),
}


@pytest.mark.parametrize("case", list(CASES))
def test_cli_plane_cross(vp, scene, tmp_path, case):
    flags, kw = CASES[case]
    got_dir, want_dir = tmp_path / "cli", tmp_path / "want"
    got_dir.mkdir()
    want_dir.mkdir()
    argv = [CM.EXE, "--julia", "32", "--size", str(W), str(H), "--spp", "8", "--batch", "8"] + flags
    r = subprocess.run(argv, cwd=str(got_dir), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    e = _cross(vp, scene, want_dir, **kw)
    try:
        got, want = sorted(os.listdir(str(got_dir))), sorted(os.listdir(str(want_dir)))
        assert got == want, "the files the driver wrote"
        data = {n: open(os.path.join(str(want_dir), n), "rb").read() for n in want}
        for n in want:
            assert open(os.path.join(str(got_dir), n), "rb").read() == data[n], n
        assert [ln for ln in r.stdout.splitlines() if ln.startswith(TIMELESS)] == e.lines
        # ---- what keeps the case from passing vacuously
        names = [n for n in want if re.match(r"[LGPR]_", n)]
        assert len(names) == len(CM.PLANES[kw["kind"]]) * (2 if kw.get("resid_prefix") else 1)
        assert len({data[n] for n in names}) == len(names), "two plane files of one run are equal"
        for n, m in e.maps.items():
            assert np.isfinite(m).all() and (m != 0).any(), n + ": an all-zero map"
        assert len(e.maps) == (len(CM.PLANES[kw["kind"]]) if kw.get("resid_prefix") else 0)
        for h in (0, 1):
            for a, rec in e.halves[h]:
                assert (rec["n"] == 4).all() and a[..., :3].max() > 0
        assert "adaptive:" not in r.stdout
    finally:
        e.free()
