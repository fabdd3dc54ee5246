"""Every documented mode of the volpath_render driver (cuda-volpath_amd/host/main.cpp, README, `usage()`) end to end: the files it writes
and the lines it prints that do not depend on time.

Each case is one volpath_render child on Julia-32 at 64 x 48.  Its expectation is the library calls the mode is documented to make, made
here through the binding on the same scene (host.bake_sunsky(0.5, 0.2), host.camera_matrix(), key (0x9E3779B9, 0x85EBCA6B), brick 1,
linear filter), each file written by volpath.host.write_image -- the Image::dump_hdr / dump_ppm of the driver.  Library and writer are
the same code on both sides and every call is defined to the bit, so every file is compared byte for byte.

The adaptive cases run --spp 16 --min-spp 4 --round 4 (16 is above 11: the decomposition estimator's optical-depth table is built before
the rounds).  Their tolerances were chosen on the CPU oracle on this scene with tests/adaptive_lib.py, adaptive_planes_lib.py and
adaptive_group_layers_lib.py; `ADAPTIVE` states them with the sample counts the oracle gives.  A case with all 64 * 48 * 16 = 49152
samples, or none, would say nothing about the per-pixel counts, so the count is asserted to lie strictly between."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cuda-volpath_amd", "volpath_render")
W, H, NPIX = 64, 48, 64 * 48
KEY = (0x9E3779B9, 0x85EBCA6B)
DN = dict(radius=5, patch=1, k=0.45)
FLOOR, FLOOR_TRANS = 1e-3, 1e-2
ROUNDS = ["--min-spp", "4", "--round", "4", "--spp", "16"]
# tolerances of the adaptive cases -> (samples of 49152, pixels left active after all four rounds) on the CPU oracle.  Of 3072 pixels 1414
# miss the box and about 2740 meet any tolerance with their first four frames; each tolerance below freezes pixels at 8 and at 12 frames
# too and leaves some active.  The planes' tolerances differ from each other, so that a swapped pair shows (layers at (0.5, 0.5): 13156
# samples, groups: 14216; the three planes at 0.3 everywhere: 15904)
ADAPTIVE = {
    "noise_philox7": (0.3, (14844, 81)),
    "noise": (0.3, (14920, 106)),
    "layers": ((0.5, 0.2), (13196, 18)),
    "groups": ((0.5, 0.2), (15760, 191)),
    "planes": ((0.3, 0.2, 0.1), (16136, 288)),
}
TIMELESS = ("wrote ", "denoised", "  cross-filtered", "  weights cut", "adaptive:")


@pytest.fixture(scope="module")
def scene(vp):
    """the driver's scene in a context of its own; the session's context keeps its state"""
    from volpath import host
    env, sun_dir, sun_power = host.bake_sunsky(0.5, 0.2)
    c = vp.Context(0)
    try:
        with c:
            vp.init_volume(vp.julia_volume(32), brick=1, linear=True)
            vp.init_envmap(env)
            vp.set_sun(sun_dir, sun_power)
            vp.set_camera(host.camera_matrix())
            vp.set_tracking(vp.TRACK_SPECTRAL)
            vp.set_envmap_sampling(vp.ENV_PASSIVE)
            vp.set_arithmetic(vp.ARITH_EXACT)
            yield dict(sun_dir=sun_dir, P=vp.make_param(W, H))
    finally:
        c.destroy()


class Expect:
    """the driver's buffers and its output stage, through the binding; files go to `out_dir` under the names the driver is given"""

    def __init__(self, vp, scene, out_dir, est="decomp", rng="samplerh", aa=1):
        self.vp, self.P, self.sun_dir, self.dir = vp, scene["P"], scene["sun_dir"], str(out_dir)
        self.lines, self.bufs, self.maps = [], [], {}
        vp.set_estimator({"decomp": vp.EST_DECOMP, "global": vp.EST_GLOBAL}[est])
        vp.set_rng({"samplerh": vp.RNG_SAMPLERH, "philox7": vp.RNG_PHILOX7}[rng], KEY)
        vp.set_shard(0, 1)
        vp.set_subpixel(aa)
        self.disp = self.image()

    def image(self):
        self.bufs.append(self.vp.DeviceBuffer(W, H))
        return self.bufs[-1]

    def records(self):
        self.bufs.append(self.vp.StatsBuffer(W, H))
        return self.bufs[-1]

    def free(self):
        for b in self.bufs:
            b.free()

    def opacity(self):
        self.vp.precompute_opacity(self.sun_dir)

    def adaptive_line(self, res, what, spp=16, round_frames=4):
        self.result = res
        full = float(NPIX * spp)
        self.lines.append("adaptive: %d of %.0f samples (%.1f %%), %d rounds of %d frames, %d pixels still above %s after %d frames"
                          % (res["samples"], full, 100.0 * res["samples"] / full, res["rounds"], round_frames, res["active_left"], what, res["frames_used"]))

    def write(self, name, rgba, hdr=None):
        from volpath import host
        hdr = name.endswith(".hdr") if hdr is None else hdr
        host.write_image(rgba, os.path.join(self.dir, name), hdr=hdr)
        self.lines.append("wrote " + name)

    def write_buf(self, name, buf):
        self.write(name, buf.download())

    def write_grey(self, name, values):
        """a float map as the driver writes it: grey, w = 1, HDR"""
        v = np.asarray(values, np.float32).reshape(H, W)
        self.maps[name] = v
        rgba = np.ones((H, W, 4), np.float32)
        rgba[..., :3] = v[..., None]
        self.write(name, rgba, hdr=True)

    def noise_map(self, name, rec, floor):
        self.write_grey(name, self.vp.stats_rel_error(rec.ptr, W, H, floor))

    def out(self, name, src=None, s=1.0):
        """--out: gamma unless the name is HDR; src None: disp already holds the scaled image"""
        vp, hdr = self.vp, name.endswith(".hdr")
        if src is not None and hdr:
            vp.scale(self.disp.ptr, src.ptr, NPIX, s)
        elif src is not None or not hdr:
            vp.gamma_correct(self.disp.ptr, (src or self.disp).ptr, NPIX, s, 2.2)
        self.write_buf(name, self.disp)

    def plane_means(self, prefix, suffixes, acc, rec, mode, spp):
        """per plane: the mean by filter, by count or by 1 / spp, written where a prefix is given; returns (planes to combine, scale)"""
        vp = self.vp
        if mode == "raw":
            for k, sfx in enumerate(suffixes if prefix else ()):
                vp.scale(self.disp.ptr, acc[k].ptr, NPIX, 1.0 / spp)
                self.write_buf(prefix + sfx, self.disp)
            return acc, 1.0 / spp
        mean = [self.image() for _ in acc]
        for k, sfx in enumerate(suffixes):
            if mode == "denoise":
                vp.denoise(mean[k].ptr, acc[k].ptr, rec[k].ptr, W, H, **DN)
            else:
                vp.scale_by_count(mean[k].ptr, acc[k].ptr, rec[k].ptr, NPIX, 1.0)
            if prefix:
                self.write_buf(prefix + sfx, mean[k])
        return mean, 1.0


def _beauty(vp, scene, d, out, est="decomp", rng="samplerh", aa=1, noise=None, noise_out=None, denoise=False, features=False, cross=False,
            resid_out=None, features_out=None, feature_step=0.001, spp=8):
    """cases a, b, c, d, e, k: the beauty image"""
    e = Expect(vp, scene, d, est, rng, aa)
    P, acc = e.P, e.image()
    rec = e.records() if noise is not None or denoise else None
    if noise is not None:
        e.opacity()
        e.adaptive_line(vp.render_adaptive(acc.ptr, rec.ptr, 0, spp, P, noise, FLOOR, 4, 4), "--noise %g" % noise)
    elif cross:
        half1, rec1, tmp = e.image(), e.records(), (e.image(), e.image())
        vp.render_frames_halves_stats(acc.ptr, half1.ptr, rec.ptr, rec1.ptr, 0, spp, P)
    elif denoise:
        vp.render_frames_stats(acc.ptr, rec.ptr, 0, spp, P)
    else:
        vp.render_frames(acc.ptr, 0, spp, P)
    if denoise:
        feats = ()
        if features:
            alpha, depth = e.image(), e.image()
            vp.render_features(P, 0.001, alpha_ptr=alpha.ptr, depth_ptr=depth.ptr)
            feats = ((alpha.ptr, 1, 0.2), (depth.ptr, 1, 0.2), (depth.ptr, 3, 0.2))
        if cross:
            resid = vp.lib().vp_malloc(NPIX * 4) if resid_out else None
            vp.denoise_cross(e.disp.ptr, resid, acc.ptr, rec.ptr, half1.ptr, rec1.ptr, tmp[0].ptr, tmp[1].ptr, W, H, features=feats, floor_y=FLOOR, **DN)
        else:
            vp.denoise_guided(e.disp.ptr, acc.ptr, rec.ptr, W, H, feats, **DN)
        e.lines.append("denoised: radius 5, patch 1, k 0.45")
        if cross:
            e.lines.append("  cross-filtered: two half-buffers, each with the other's weights, merged by their counts")
        if features:
            e.lines.append("  weights cut by features: sigma alpha 0.2, sigma depth 0.2")
        e.out(out)
    elif noise is not None:
        vp.scale_by_count(e.disp.ptr, acc.ptr, rec.ptr, NPIX, 1.0)
        e.out(out)
    else:
        e.out(out, acc, 1.0 / spp)
    if cross and resid_out:
        m = np.empty((H, W), np.float32)
        vp.lib().vp_download(m.ctypes.data_as(ctypes.c_void_p), resid, NPIX * 4)
        vp.lib().vp_free(resid)
        e.write_grey(resid_out, m)
    if noise_out:
        e.noise_map(noise_out, rec, FLOOR)
    if features_out:
        vp.set_shard(0, 1)
        vp.set_subpixel(1)
        alpha, depth = vp.render_features(P, feature_step)
        e.inf_depths = int(np.isinf(depth).sum())
        depth[np.isinf(depth)] = 0.0       # RGBE has no inf
        e.write(features_out + "_alpha.hdr", alpha)
        e.write(features_out + "_depth.hdr", depth)
    return e


PLANES = {"layers": ("_fg.hdr", "_trans.hdr"), "groups": ("_sun.hdr", "_sky.hdr"), "planes": ("_sun.hdr", "_sky.hdr", "_trans.hdr")}
FLOORS = {"layers": (FLOOR, FLOOR_TRANS), "groups": (FLOOR, FLOOR), "planes": (FLOOR, FLOOR, FLOOR_TRANS)}


def _planes(vp, scene, d, kind, out, prefix=None, over=None, sun_gain=(1.0, 1.0, 1.0), sky_gain=(1.0, 1.0, 1.0), denoise=False, tol=None,
            noise_prefix=None, spp=8):
    """cases f, g, h, i, j: layers, light groups, or the three planes of a group-layers render"""
    e = Expect(vp, scene, d)
    P, sfx = e.P, PLANES[kind]
    acc = [e.image() for _ in sfx]
    rec = [e.records() for _ in sfx] if denoise or tol else None
    a, r = [b.ptr for b in acc], [b.ptr for b in rec or ()]
    if tol:
        e.opacity()
        call = {"layers": vp.render_adaptive_layers, "groups": vp.render_adaptive_groups, "planes": vp.render_adaptive_group_layers}[kind]
        flag = "--planes-noise " if kind == "planes" else "--plane-noise "
        e.adaptive_line(call(*a, *r, 0, spp, P, tol, FLOORS[kind], 4, 4), flag + " ".join("%g" % t for t in tol))
    elif denoise:
        {"layers": vp.render_frames_layers_stats, "groups": vp.render_frames_groups_stats, "planes": vp.render_frames_group_layers_stats}[kind](*a, *r, 0, spp, P)
    else:
        {"layers": vp.render_frames_layers, "groups": vp.render_frames_groups, "planes": vp.render_frames_group_layers}[kind](*a, 0, spp, P)
    m, s = e.plane_means(prefix, sfx, acc, rec, "denoise" if denoise else "count" if tol else "raw", spp)
    m = [b.ptr for b in m]
    if kind == "layers" and over is not None:
        vp.composite(e.disp.ptr, m[0], m[1], NPIX, s, plate_rgb=over)
    elif kind == "groups":
        vp.relight(e.disp.ptr, m[0], m[1], NPIX, s, sun_gain, sky_gain)
    elif kind == "planes":
        vp.relight_composite(e.disp.ptr, m[0], m[1], m[2], NPIX, s, sun_gain, sky_gain, plate_rgb=over or (0.0, 0.0, 0.0))
    if denoise:
        e.lines.append("denoised per plane: radius 5, patch 1, k 0.45")
    if kind != "layers" or over is not None:
        e.out(out)
    for k, name in enumerate(sfx if noise_prefix else ()):
        e.noise_map(noise_prefix + name, rec[k], FLOORS[kind][k])
    return e


def _t(key):
    return ADAPTIVE[key][0]


def _f(values):
    return [repr(float(v)) for v in values]


GAINS = dict(sun_gain=(1.5, 1.2, 0.9), sky_gain=(0.5, 0.5, 0.5))
OVER = (0.2, 0.4, 0.9)
# case -> (driver flags, expectation, its arguments, the key of ADAPTIVE or None)
CASES = {
    "a_frames_hdr": (["--out", "x.hdr"], _beauty, dict(out="x.hdr"), None),
    "b_noise_ppm": (["--rng", "philox7", "--noise", repr(_t("noise_philox7")), *ROUNDS, "--noise-out", "n.hdr", "--out", "x.ppm"], _beauty,
                    dict(out="x.ppm", rng="philox7", noise=_t("noise_philox7"), noise_out="n.hdr", spp=16), "noise_philox7"),
    "c_denoise": (["--denoise", "--out", "x.hdr"], _beauty, dict(out="x.hdr", denoise=True), None),
    "c_denoise_noise": (["--denoise", "--noise", repr(_t("noise")), *ROUNDS, "--noise-out", "n.hdr", "--out", "x.hdr"], _beauty,
                        dict(out="x.hdr", denoise=True, noise=_t("noise"), noise_out="n.hdr", spp=16), "noise"),
    "d_denoise_features": (["--estimator", "global", "--denoise", "--denoise-features", "--out", "x.ppm"], _beauty,
                           dict(out="x.ppm", est="global", denoise=True, features=True), None),
    "e_denoise_cross": (["--denoise-cross", "--resid-out", "r.hdr", "--aa", "2", "--out", "x.hdr"], _beauty,
                        dict(out="x.hdr", aa=2, denoise=True, cross=True, resid_out="r.hdr"), None),
    "f_layers_over": (["--layers-out", "L", "--over", *_f(OVER), "--out", "x.ppm"], _planes, dict(kind="layers", out="x.ppm", prefix="L", over=OVER), None),
    "f_layers_alone": (["--layers-out", "L"], _planes, dict(kind="layers", out=None, prefix="L"), None),
    "g_groups_gains": (["--groups-out", "G", "--sun-gain", *_f(GAINS["sun_gain"]), "--sky-gain", *_f(GAINS["sky_gain"]), "--out", "x.hdr"], _planes,
                       dict(kind="groups", out="x.hdr", prefix="G", **GAINS), None),
    "h_groups_denoise": (["--groups-out", "G", "--groups-denoise"], _planes, dict(kind="groups", out="output0.ppm", prefix="G", denoise=True), None),
    "h_layers_denoise": (["--over", "0", "0", "0", "--layers-denoise"], _planes, dict(kind="layers", out="output0.ppm", over=(0.0, 0.0, 0.0), denoise=True), None),
    "i_layers_plane_noise": (["--layers-out", "L", "--over", *_f(OVER), "--plane-noise", *_f(_t("layers")), "--plane-noise-out", "N", *ROUNDS], _planes,
                             dict(kind="layers", out="output0.ppm", prefix="L", over=OVER, tol=_t("layers"), noise_prefix="N", spp=16), "layers"),
    "i_groups_plane_noise": (["--groups-out", "G", "--plane-noise", *_f(_t("groups")), "--plane-noise-out", "N", *ROUNDS], _planes,
                             dict(kind="groups", out="output0.ppm", prefix="G", tol=_t("groups"), noise_prefix="N", spp=16), "groups"),
    "j_planes": (["--planes-out", "P", "--sun-gain", *_f(GAINS["sun_gain"]), "--over", *_f(OVER), "--out", "x.hdr"], _planes,
                 dict(kind="planes", out="x.hdr", prefix="P", over=OVER, sun_gain=GAINS["sun_gain"]), None),
    "j_planes_denoise": (["--planes-out", "P", "--sun-gain", *_f(GAINS["sun_gain"]), "--over", *_f(OVER), "--out", "x.hdr", "--planes-denoise"], _planes,
                         dict(kind="planes", out="x.hdr", prefix="P", over=OVER, sun_gain=GAINS["sun_gain"], denoise=True), None),
    "j_planes_noise": (["--planes-out", "P", "--sun-gain", *_f(GAINS["sun_gain"]), "--over", *_f(OVER), "--out", "x.hdr", "--planes-noise", *_f(_t("planes")),
                        "--planes-noise-out", "N", *ROUNDS], _planes,
                       dict(kind="planes", out="x.hdr", prefix="P", over=OVER, sun_gain=GAINS["sun_gain"], tol=_t("planes"), noise_prefix="N", spp=16), "planes"),
    "k_features_aa": (["--aa", "2", "--features-out", "F", "--feature-step", "0.01", "--out", "x.ppm"], _beauty,
                      dict(out="x.ppm", aa=2, features_out="F", feature_step=0.01), None),
}


@pytest.mark.parametrize("case", list(CASES))
def test_cli_mode(vp, scene, tmp_path, case):
    flags, expect, kw, adaptive = CASES[case]
    got_dir, want_dir = tmp_path / "cli", tmp_path / "want"
    got_dir.mkdir()
    want_dir.mkdir()
    argv = [EXE, "--julia", "32", "--size", str(W), str(H)] + ([] if "--spp" in flags else ["--spp", "8"]) + ["--batch", "8"] + flags
    r = subprocess.run(argv, cwd=str(got_dir), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    e = expect(vp, scene, want_dir, **kw)
    try:
        got, want = sorted(os.listdir(str(got_dir))), sorted(os.listdir(str(want_dir)))
        assert got == want, "the files the driver wrote"       # (f_layers_alone: neither --out nor output0.ppm)
        data = {n: open(os.path.join(str(want_dir), n), "rb").read() for n in want}
        for n in want:
            assert open(os.path.join(str(got_dir), n), "rb").read() == data[n], n
        assert [ln for ln in r.stdout.splitlines() if ln.startswith(TIMELESS)] == e.lines
        # ---- what keeps the case from passing vacuously
        names = [n for n in want if re.match(r"[LGPN]_", n)]
        assert len({data[n] for n in names}) == len(names), "two plane files of one run are equal"
        for n, m in e.maps.items():
            assert np.isfinite(m).all() and (m != 0).any(), n + ": an all-zero map"
        assert len(e.maps) == sum(f in ("--resid-out", "--noise-out") for f in flags) + sum(len(PLANES[kw["kind"]]) for f in flags if f in ("--plane-noise-out", "--planes-noise-out"))
        if adaptive:
            samples = e.result["samples"]
            print(case, e.result)
            assert 0 < samples < NPIX * 16
            assert (samples, e.result["active_left"]) == ADAPTIVE[adaptive][1], "the oracle's counts for this tolerance"
            m = re.search(r"^adaptive: (\d+) of 49152 samples \(\S+ %\), (\d+) rounds of 4 frames, (\d+) pixels still above .* after (\d+) frames$", r.stdout, re.M)
            assert m and tuple(int(v) for v in m.groups()) == (samples, e.result["rounds"], e.result["active_left"], e.result["frames_used"])
        else:
            assert "adaptive:" not in r.stdout
        if case == "k_features_aa":
            assert e.inf_depths > 0, "no depth of this scene is +inf: the substitution by 0 is not reached"
    finally:
        e.free()
