"""Adaptive sampling on planes (include/volpath.h vp_render_adaptive_groups / vp_render_adaptive_layers) without a
GPU: the symbols and the struct's layout, every refusal that comes before the device, the CLI flags, and the restatement of the
definition (tests/adaptive_planes_lib.py) on the CPU oracle's plane samples -- the census of the eight anchors that the GPU tests
compare against, and the restatement against itself."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import adaptive_lib as AL
import adaptive_planes_lib as AP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cuda-volpath_amd", "volpath_render")
NEW = ("vp_render_adaptive_groups", "vp_render_adaptive_layers")
E_STATE, E_ARG = -2, -3


def test_struct_layout_in_c(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "volpath.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(vp_adaptive_planes), offsetof(vp_adaptive_planes, rel_tol),'
                   ' offsetof(vp_adaptive_planes, floor_y), offsetof(vp_adaptive_planes, min_frames), offsetof(vp_adaptive_planes, round_frames));'
                   ' return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["cc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    assert [int(v) for v in subprocess.check_output([str(exe)], text=True).split()] == [24, 0, 8, 16, 20]


def test_symbols_are_declared_exported_and_mirrored():
    import volpath
    text = open(os.path.join(ROOT, "include", "volpath.h")).read()
    L = volpath.lib()
    for n, (a, b) in zip(NEW, (("sun", "sky"), ("fg", "trans"))):
        assert n in volpath.PART2_SYMBOLS and hasattr(L, n)
        assert re.search(r"int\s+%s\(vp_float4\*\s*d_%s,\s*vp_float4\*\s*d_%s,\s*vp_pixel_stats\*\s*d_%s_stats,\s*vp_pixel_stats\*\s*d_%s_stats,"
                         r"\s*int first_frame,\s*int max_frames,\s*const Param\*\s*p,\s*const vp_adaptive_planes\*\s*a,\s*vp_adaptive_result\*\s*result\);"
                         % (n, a, b, a, b), text), n
        assert getattr(L, n).argtypes == [C.c_void_p] * 4 + [C.c_int, C.c_int, C.POINTER(volpath.Param), C.POINTER(volpath.AdaptivePlanes),
                                                              C.POINTER(volpath.AdaptiveResult)]
    S = volpath.AdaptivePlanes
    assert C.sizeof(S) == 24 and (S.rel_tol.offset, S.floor_y.offset, S.min_frames.offset, S.round_frames.offset) == (0, 8, 16, 20)
    assert callable(volpath.render_adaptive_groups) and callable(volpath.render_adaptive_layers)
    flat = " ".join(text.split()).replace(" * ", " ")
    section = flat[flat.index("Adaptive sampling on planes"):]
    for phrase in ("ACTIVE while the FROZEN bit is clear in BOTH", "takes plane k out of the decision", "groups combined with layers",
                   "across processes", "under VP_ARITH_FAST", "small bias"):
        assert phrase in section, phrase
    assert "which plane's record would freeze a pixel" not in flat             # the design question is settled


@pytest.mark.parametrize("name", NEW)
def test_refusals_come_before_the_device(name):
    """VP_E_ARG for the arguments, VP_E_STATE exactly where the underlying plane call gives it: the pointers are never followed and no
    device is asked for (this machine has none)"""
    import volpath
    L = volpath.lib()
    P = C.byref(volpath.make_param(16, 8))
    a, b, ra, rb = (C.c_void_p(v) for v in (0x1000, 0x2000, 0x3000, 0x4000))      # never dereferenced
    f = getattr(L, name)

    def call(d0=a, d1=b, r0=ra, r1=rb, first=0, maxf=8, p=P, arg="default", tol=(0.1, 0.2), fl=(1e-3, 1e-2), min_frames=2, round_frames=1, res=None):
        if arg == "default":
            arg = C.byref(volpath.AdaptivePlanes((C.c_float * 2)(*tol), (C.c_float * 2)(*fl), min_frames, round_frames))
        return f(d0, d1, r0, r1, first, maxf, p, arg, res)

    nan = float("nan")
    for kw in (dict(d0=None), dict(d1=None), dict(r0=None), dict(r1=None), dict(p=None), dict(arg=None), dict(d1=a), dict(r1=ra), dict(maxf=0),
               dict(maxf=-5), dict(first=-1), dict(min_frames=1), dict(min_frames=0), dict(min_frames=-3), dict(round_frames=0), dict(round_frames=-1),
               dict(tol=(-0.1, 0.2)), dict(tol=(0.1, -0.2)), dict(tol=(nan, 0.2)), dict(tol=(0.1, nan)), dict(fl=(-1e-3, 0.0)), dict(fl=(0.0, -1e-3)),
               dict(fl=(nan, 0.0)), dict(fl=(0.0, nan))):
        assert call(**kw) == E_ARG, kw
        assert name + ":" in L.vp_last_error().decode(), kw
    res = volpath.AdaptiveResult(7, 7, 7, 7)
    assert call(maxf=0, res=C.byref(res)) == E_ARG
    assert res.as_dict() == {"samples": 0, "rounds": 0, "active_left": 0, "frames_used": 0}
    try:
        for mode in (volpath.TRACK_SCALAR, volpath.TRACK_MULTI_CHANNEL):
            volpath.set_tracking(mode)
            assert call() == E_STATE
            assert "spectral" in L.vp_last_error().decode() and name + " " in L.vp_last_error().decode()
        volpath.set_tracking(volpath.TRACK_SPECTRAL)
        assert L.vp_enable_counters(1) == 0
        assert call() == E_STATE
        assert "counters" in L.vp_last_error().decode() and name + " " in L.vp_last_error().decode()
        L.vp_enable_counters(0)
        # (the setters of the environment mode and the arithmetic ask for the device themselves: where there is none they fail and the
        # mode stays; tests/test_adaptive_planes_gpu.py makes both refusals with the four buffers checked)
        if L.vp_set_envmap_sampling(volpath.ENV_MIS) == 0:
            assert call() == E_STATE and "passive" in L.vp_last_error().decode() and name + " " in L.vp_last_error().decode()
            assert L.vp_set_envmap_sampling(volpath.ENV_PASSIVE) == 0
        if L.vp_set_arithmetic(volpath.ARITH_FAST) == 0:
            assert call() == E_STATE and "exact" in L.vp_last_error().decode() and name + " " in L.vp_last_error().decode()
            assert L.vp_set_arithmetic(volpath.ARITH_EXACT) == 0
        # an argument error comes before a state error
        volpath.set_tracking(volpath.TRACK_SCALAR)
        assert call(min_frames=1) == E_ARG
    finally:
        volpath.set_tracking(volpath.TRACK_SPECTRAL)
        L.vp_enable_counters(0)
    wrapper = getattr(volpath, name[3:])
    with pytest.raises(volpath.VolpathError, match=name):
        wrapper(a, b, ra, ra, 0, 8, volpath.make_param(16, 8), (0.1, 0.1))


def test_cli_plane_noise_flags():
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--plane-noise TOL0 TOL1", "--plane-noise-out PREFIX", "vp_render_adaptive_groups", "vp_render_adaptive_layers"):
        assert flag in r.stdout, flag
    planes = (["--groups-out", "x"], ["--sun-gain", "2", "0.5", "0"], ["--sky-gain", "0", "1", "3"], ["--layers-out", "x"], ["--over", "0.5", "0.5", "0.5"])
    tol = ["--plane-noise", "0.05", "0.1"]
    r = subprocess.run([EXE] + tol, capture_output=True, text=True)                        # alone: it needs a plane flag
    assert r.returncode == 2 and "--plane-noise" in r.stderr and "--groups-out" in r.stderr and "--layers-out" in r.stderr, r.stderr
    for plane in planes:
        for other in (["--gpus", "2"], ["--noise", "0.05"], ["--denoise"]):
            r = subprocess.run([EXE] + tol + plane + other, capture_output=True, text=True)
            assert r.returncode == 2 and other[0] in r.stderr, (plane, other, r.stderr)
        for bad in (["--plane-noise", "0.05"], ["--plane-noise", "0.05", "abc"], ["--plane-noise", "-0.5", "0.1"], ["--plane-noise", "0.1", "-0.5"],
                    ["--plane-noise", "nan", "0.1"], ["--plane-noise", "0.1", "0.1x"]):
            r = subprocess.run([EXE] + plane + bad, capture_output=True, text=True)
            assert r.returncode == 2, (plane, bad, r.stdout, r.stderr)
        for bad in (["--min-spp", "1"], ["--round", "0"]):
            r = subprocess.run([EXE] + tol + plane + bad, capture_output=True, text=True)
            assert r.returncode == 2, (plane, bad, r.stderr)
    r = subprocess.run([EXE, "--groups-out", "x", "--plane-noise-out", "y"], capture_output=True, text=True)
    assert r.returncode == 2 and "--plane-noise-out" in r.stderr
    # the refusals that were there before stay: --noise with a plane flag or a per-plane filter
    for plane in planes:
        r = subprocess.run([EXE, "--noise", "0.05"] + plane, capture_output=True, text=True)
        assert r.returncode == 2 and "--noise" in r.stderr, (plane, r.stderr)
    for flag, plane in (("--groups-denoise", planes[0]), ("--layers-denoise", planes[3])):
        r = subprocess.run([EXE, "--noise", "0.05", flag] + plane, capture_output=True, text=True)
        assert r.returncode == 2 and flag in r.stderr and "--noise" in r.stderr, (flag, r.stderr)


# ---- the restatement on the oracle's plane samples
@pytest.mark.parametrize("kind,name,est,rng,first", AP.ANCHORS, ids=["%s-%s-est%d-rng%d-from%d" % a for a in AP.ANCHORS])
def test_anchor_census(oracle, kind, name, est, rng, first):
    """A condition on the INPUTS of the GPU comparison, from the oracle restatement alone: every anchor freezes pixels at exactly
    min_frames, freezes others strictly between, leaves some active, and has pixel-rounds in which only plane 0's half of the decision
    held and pixel-rounds in which only plane 1's did -- the AND is exercised from both sides."""
    st, res, tally = AP.anchor_expected(oracle, kind, name, est, rng, first)
    c = AP.census(st, AP.ANCHOR_ARGS["min_frames"], AP.ANCHOR_FRAMES)
    print(kind, name, est, rng, first, res, c, tally)
    assert c["at_min"] > 0 and c["between"] > 0 and c["active"] > 0, c
    assert tally["only0"] > 0 and tally["only1"] > 0, tally
    last = int((((st[0].flags & 1) != 0) & (st[0].n == AP.ANCHOR_FRAMES)).sum())           # frozen by the last round
    assert c["at_min"] + c["between"] + last + c["active"] == 16 * 12 and res["active_left"] == c["active"]
    assert res["samples"] == int(st[0].n.sum()) == int(st[1].n.sum()) and res["frames_used"] == AP.ANCHOR_FRAMES and res["rounds"] == 12
    # a frozen pixel stopped at a round boundary at or above min_frames, in both records at once; an active one has every frame
    frozen = (st[0].flags & 1) != 0
    assert (st[0].n[frozen] % 4 == 0).all() and (st[0].n[frozen] >= 8).all() and (st[0].n[~frozen] == AP.ANCHOR_FRAMES).all()
    # the ranges measured when the anchors were chosen (the issue's table)
    lo_hi = {"groups": dict(at_min=(159, 175), between=(14, 31), active=(1, 3), only0=(19, 77), only1=(20, 60)),
             "layers": dict(at_min=(160, 179), between=(10, 17), active=(3, 17), only0=(2, 21), only1=(65, 237))}[kind]
    for k, (lo, hi) in lo_hi.items():
        v = c[k] if k in c else tally[k]
        assert lo <= v <= hi, (k, v, lo, hi)


@pytest.mark.parametrize("kind,name,est,rng,first", (AP.ANCHORS[1], AP.ANCHORS[6]))
def test_one_call_equals_two_calls_at_a_round_boundary(oracle, kind, name, est, rng, first):
    """48 frames in one call equal 20 + 28 in two: 20 is a multiple of the round, so the boundaries are the same"""
    frames = AP.anchor_frames(oracle, kind, name, est, rng, first)
    one, res, _ = AP.anchor_expected(oracle, kind, name, est, rng, first)
    two = AP.new_pair(16, 12)
    r1 = AP.render_adaptive_planes(two, frames, first, 20, AP.ANCHOR_TOL[kind], **AP.ANCHOR_ARGS)
    r2 = AP.render_adaptive_planes(two, frames, first + 20, 28, AP.ANCHOR_TOL[kind], **AP.ANCHOR_ARGS)
    for k in (0, 1):
        assert AL.same_state(one[k], two[k].acc, two[k].records()) is None, k
    assert r1["samples"] + r2["samples"] == res["samples"] and r1["rounds"] + r2["rounds"] == res["rounds"] and r2["active_left"] == res["active_left"]
    # ... and not at any other place: a first call of 18 frames ends with a round of two
    odd = AP.new_pair(16, 12)
    AP.render_adaptive_planes(odd, frames, first, 18, AP.ANCHOR_TOL[kind], **AP.ANCHOR_ARGS)
    AP.render_adaptive_planes(odd, frames, first + 18, 30, AP.ANCHOR_TOL[kind], **AP.ANCHOR_ARGS)
    assert any(AL.same_state(one[k], odd[k].acc, odd[k].records()) is not None for k in (0, 1))


def test_a_large_floor_takes_a_plane_out_of_the_decision(oracle):
    """floor_y[k] = 1e30f with rel_tol[k] > 0: plane k's half holds from two samples on, so the frozen set is the other plane's own --
    adaptive_lib.render_adaptive on that plane alone"""
    kind, name, est, rng, first = AP.FLOOR_CASE
    frames = AP.anchor_frames(oracle, kind, name, est, rng, first)
    tol, fl = AP.FLOOR_TOL, AP.ANCHOR_ARGS["floor_y"]
    for out in (0, 1):
        keep = 1 - out
        st = AP.new_pair(16, 12)
        floors = tuple(AP.BIG_FLOOR if k == out else fl[k] for k in (0, 1))
        res = AP.render_adaptive_planes(st, frames, first, AP.ANCHOR_FRAMES, tol, floors, 8, 4)
        alone = AL.Stats(16, 12)
        want = AL.render_adaptive(alone, lambda f: frames(f)[keep], first, AP.ANCHOR_FRAMES, tol[keep], fl[keep], 8, 4)
        assert AL.same_state(alone, st[keep].acc, st[keep].records()) is None and res == want, out
        assert np.array_equal(st[out].flags, alone.flags) and np.array_equal(st[out].n, alone.n)
        assert 0 < int((alone.flags & 1).sum()) < 16 * 12
