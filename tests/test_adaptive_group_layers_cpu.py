"""Adaptive sampling on group layers (include/volpath.h vp_render_adaptive_group_layers) without a GPU: the
symbol and the struct's layout, every refusal that comes before the device, the CLI flags, and the restatement of the definition
(tests/adaptive_group_layers_lib.py) on the CPU oracle's plane samples -- the census of the four anchors that the GPU tests compare
against, the restatement against itself and against the two-plane restatement of tests/adaptive_planes_lib.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import adaptive_group_layers_lib as AG
import adaptive_lib as AL
import adaptive_planes_lib as AP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cuda-volpath_amd", "volpath_render")
NAME = "vp_render_adaptive_group_layers"
E_STATE, E_ARG = -2, -3
IDS = ["%s-est%d-rng%d-from%d" % a for a in AG.ANCHORS]


def test_struct_layout_in_c(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "volpath.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(vp_adaptive_planes3), offsetof(vp_adaptive_planes3, rel_tol),'
                   ' offsetof(vp_adaptive_planes3, floor_y), offsetof(vp_adaptive_planes3, min_frames), offsetof(vp_adaptive_planes3, round_frames));'
                   ' return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["cc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    assert [int(v) for v in subprocess.check_output([str(exe)], text=True).split()] == [32, 0, 12, 24, 28]


def test_symbol_is_declared_exported_mirrored_and_typed():
    import volpath
    text = open(os.path.join(ROOT, "include", "volpath.h")).read()
    L = volpath.lib()
    assert NAME in volpath.PART2_SYMBOLS and hasattr(L, NAME)
    assert re.search(r"int\s+%s\(vp_float4\*\s*d_sun,\s*vp_float4\*\s*d_sky,\s*vp_float4\*\s*d_trans,\s*vp_pixel_stats\*\s*d_sun_stats,"
                     r"\s*vp_pixel_stats\*\s*d_sky_stats,\s*vp_pixel_stats\*\s*d_trans_stats,\s*int first_frame,\s*int max_frames,\s*const Param\*\s*p,"
                     r"\s*const vp_adaptive_planes3\*\s*a,\s*vp_adaptive_result\*\s*result\);" % NAME, text)
    assert getattr(L, NAME).argtypes == [C.c_void_p] * 6 + [C.c_int, C.c_int, C.POINTER(volpath.Param), C.POINTER(volpath.AdaptivePlanes3),
                                                           C.POINTER(volpath.AdaptiveResult)]
    S = volpath.AdaptivePlanes3
    assert C.sizeof(S) == 32 and (S.rel_tol.offset, S.floor_y.offset, S.min_frames.offset, S.round_frames.offset) == (0, 12, 24, 28)
    assert callable(volpath.render_adaptive_group_layers)
    flat = " ".join(text.split()).replace(" * ", " ")
    section = flat[flat.index("Adaptive sampling on group layers (DESIGN.md section 2.11)"):]
    for phrase in ("ACTIVE while the FROZEN bit is clear in ALL THREE", "takes plane k out of the decision", "across processes", "under VP_ARITH_FAST",
                   "small bias", "vp_relight_composite with scale 1"):
        assert phrase in section, phrase
    # the call is no longer listed as unbuilt, in the header or in the documents
    for doc in ("include/volpath.h", "DESIGN.md", "README.md"):
        body = " ".join(open(os.path.join(ROOT, doc)).read().split()).replace(" * ", " ")
        assert NAME in body, doc
        assert not re.search(r"[Nn]ot built: adaptive rounds on three planes", body), doc


def test_refusals_come_before_the_device():
    """VP_E_ARG for the arguments, VP_E_STATE exactly where vp_render_frames_group_layers gives it: the pointers are never followed and
    no device is asked for"""
    import volpath
    L = volpath.lib()
    P = C.byref(volpath.make_param(16, 8))
    ptr = [C.c_void_p(v) for v in (0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000)]      # never dereferenced
    f = getattr(L, NAME)

    def call(swap=None, first=0, maxf=8, p=P, arg="default", tol=(0.1, 0.2, 0.3), fl=(1e-3, 1e-3, 1e-2), min_frames=2, round_frames=1, res=None):
        q = list(ptr)
        for i, v in (swap or {}).items():
            q[i] = v
        if arg == "default":
            arg = C.byref(volpath.AdaptivePlanes3((C.c_float * 3)(*tol), (C.c_float * 3)(*fl), min_frames, round_frames))
        return f(*q, first, maxf, p, arg, res)

    nan = float("nan")
    cases = [dict(swap={i: None}) for i in range(6)] + [dict(p=None), dict(arg=None)]
    cases += [dict(swap={j: ptr[i]}) for i, j in ((0, 1), (0, 2), (1, 2), (3, 4), (3, 5), (4, 5))]        # any two accumulators, any two record buffers
    cases += [dict(maxf=0), dict(maxf=-5), dict(first=-1), dict(min_frames=1), dict(min_frames=0), dict(min_frames=-3), dict(round_frames=0), dict(round_frames=-1)]
    for k in range(3):
        for bad in (-0.1, nan):
            cases.append(dict(tol=tuple(bad if j == k else 0.1 for j in range(3))))
            cases.append(dict(fl=tuple(bad if j == k else 0.0 for j in range(3))))
    for kw in cases:
        assert call(**kw) == E_ARG, kw
        assert NAME + ":" in L.vp_last_error().decode(), kw
    res = volpath.AdaptiveResult(7, 7, 7, 7)
    assert call(maxf=0, res=C.byref(res)) == E_ARG
    assert res.as_dict() == {"samples": 0, "rounds": 0, "active_left": 0, "frames_used": 0}
    try:
        for mode in (volpath.TRACK_SCALAR, volpath.TRACK_MULTI_CHANNEL):
            volpath.set_tracking(mode)
            res = volpath.AdaptiveResult(7, 7, 7, 7)
            assert call(res=C.byref(res)) == E_STATE
            assert "spectral" in L.vp_last_error().decode() and NAME + " " in L.vp_last_error().decode()
            assert res.as_dict() == {"samples": 0, "rounds": 0, "active_left": 0, "frames_used": 0}
        volpath.set_tracking(volpath.TRACK_SPECTRAL)
        assert L.vp_enable_counters(1) == 0
        assert call() == E_STATE
        assert "counters" in L.vp_last_error().decode() and NAME + " " in L.vp_last_error().decode()
        L.vp_enable_counters(0)
        # (the setters of the environment mode and the arithmetic ask for the device themselves: where there is none they fail and the
        # mode stays; tests/test_adaptive_group_layers_gpu.py makes both refusals with the six buffers checked)
        if L.vp_set_envmap_sampling(volpath.ENV_MIS) == 0:
            assert call() == E_STATE and "passive" in L.vp_last_error().decode() and NAME + " " in L.vp_last_error().decode()
            assert L.vp_set_envmap_sampling(volpath.ENV_PASSIVE) == 0
        if L.vp_set_arithmetic(volpath.ARITH_FAST) == 0:
            assert call() == E_STATE and "exact" in L.vp_last_error().decode() and NAME + " " in L.vp_last_error().decode()
            assert L.vp_set_arithmetic(volpath.ARITH_EXACT) == 0
        # an argument error comes before a state error
        volpath.set_tracking(volpath.TRACK_SCALAR)
        assert call(min_frames=1) == E_ARG
        assert call(swap={5: ptr[3]}) == E_ARG
    finally:
        volpath.set_tracking(volpath.TRACK_SPECTRAL)
        L.vp_enable_counters(0)
    with pytest.raises(volpath.VolpathError, match=NAME):
        volpath.render_adaptive_group_layers(*ptr[:4], ptr[3], ptr[5], 0, 8, volpath.make_param(16, 8), (0.1, 0.1, 0.1))


def test_cli_planes_noise_flags():
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--planes-noise TOL_SUN TOL_SKY TOL_TRANS", "--planes-noise-out PREFIX", NAME, "--plane-noise TOL0 TOL1"):
        assert flag in r.stdout, flag
    tol = ["--planes-noise", "0.05", "0.1", "0.2"]
    planes = ["--planes-out", "x"]
    r = subprocess.run([EXE] + tol, capture_output=True, text=True)                        # alone: it needs --planes-out
    assert r.returncode == 2 and "--planes-noise" in r.stderr and "--planes-out" in r.stderr, r.stderr
    for extra in ([], ["--groups-out", "y"], ["--layers-out", "y"], ["--over", "0.5", "0.5", "0.5"], ["--sun-gain", "2", "0.5", "0"]):
        r = subprocess.run([EXE] + tol + extra, capture_output=True, text=True)
        assert r.returncode == 2, (extra, r.stderr)
    for other in (["--gpus", "2"], ["--noise", "0.05"], ["--denoise"]):
        for extra in ([], ["--planes-denoise"], ["--planes-noise-out", "y"]):
            r = subprocess.run([EXE] + planes + tol + extra + other, capture_output=True, text=True)
            assert r.returncode == 2 and other[0] in r.stderr, (other, extra, r.stderr)
    for bad in (["--planes-noise"], ["--planes-noise", "0.05"], ["--planes-noise", "0.05", "0.1"], ["--planes-noise", "0.05", "0.1", "abc"],
                ["--planes-noise", "-0.5", "0.1", "0.1"], ["--planes-noise", "0.1", "-0.5", "0.1"], ["--planes-noise", "0.1", "0.1", "-0.5"],
                ["--planes-noise", "nan", "0.1", "0.1"], ["--planes-noise", "0.1", "0.1", "nan"], ["--planes-noise", "0.1", "0.1", "0.1x"]):
        r = subprocess.run([EXE] + planes + bad, capture_output=True, text=True)
        assert r.returncode == 2, (bad, r.stdout, r.stderr)
    r = subprocess.run([EXE] + tol[:3] + planes, capture_output=True, text=True)           # two values, then another flag
    assert r.returncode == 2, r.stderr
    for bad in (["--min-spp", "1"], ["--min-spp", "0"], ["--round", "0"], ["--round", "-2"]):
        r = subprocess.run([EXE] + planes + tol + bad, capture_output=True, text=True)
        assert r.returncode == 2 and "--planes-noise" in r.stderr, (bad, r.stderr)
    for extra in ([], ["--planes-denoise"]):
        r = subprocess.run([EXE] + planes + extra + ["--planes-noise-out", "y"], capture_output=True, text=True)
        assert r.returncode == 2 and "--planes-noise-out" in r.stderr and "--planes-noise" in r.stderr, r.stderr
    # the two-plane flag stays refused with --planes-out, and its refusal points to the new flag
    r = subprocess.run([EXE] + planes + ["--plane-noise", "0.1", "0.1"], capture_output=True, text=True)
    assert r.returncode == 2 and "--planes-out" in r.stderr and "--plane-noise" in r.stderr and "--planes-noise TOL_SUN TOL_SKY TOL_TRANS" in r.stderr, r.stderr


# ---- the restatement on the oracle's plane samples
@pytest.mark.parametrize("name,est,rng,first", AG.ANCHORS, ids=IDS)
def test_anchor_census(oracle, name, est, rng, first):
    """A condition on the INPUTS of the GPU comparison, from the oracle restatement alone: every anchor freezes pixels at exactly
    min_frames, freezes others strictly later, leaves some active, and has pixel-rounds in which each of the three planes alone held a
    pixel back -- the AND is exercised from all three sides.  The counts are those measured when the anchors were chosen ("between":
    frozen after more than min_frames and before the last round)."""
    st, res, tally = AG.anchor_expected(oracle, name, est, rng, first)
    c = AG.census(st, AG.ANCHOR_ARGS["min_frames"], AG.ANCHOR_FRAMES)
    last = int((((st[0].flags & 1) != 0) & (st[0].n == AG.ANCHOR_FRAMES)).sum())           # frozen by the last round
    print(name, est, rng, first, res, c, "last", last, tally)
    assert c["at_min"] > 0 and c["between"] > 0 and c["active"] > 0, c
    assert tally["held0"] > 0 and tally["held1"] > 0 and tally["held2"] > 0, tally
    assert c["at_min"] + c["between"] + last + c["active"] == 16 * 12 and res["active_left"] == c["active"]
    assert res["samples"] == int(st[0].n.sum()) == int(st[1].n.sum()) == int(st[2].n.sum()) and res["frames_used"] == AG.ANCHOR_FRAMES and res["rounds"] == 12
    # a frozen pixel stopped at a round boundary at or above min_frames, in all three records at once; an active one has every frame
    frozen = (st[0].flags & 1) != 0
    assert (st[0].n[frozen] % 4 == 0).all() and (st[0].n[frozen] >= 8).all() and (st[0].n[~frozen] == AG.ANCHOR_FRAMES).all()
    assert ((c["at_min"], c["between"], c["active"]), (tally["held0"], tally["held1"], tally["held2"])) == AG.ANCHOR_CENSUS[(name, est, rng, first)]


@pytest.mark.parametrize("name,est,rng,first", (AG.ANCHORS[0], AG.ANCHORS[3]), ids=(IDS[0], IDS[3]))
def test_one_call_equals_two_calls_at_a_round_boundary(oracle, name, est, rng, first):
    """48 frames in one call equal 20 + 28 in two: 20 is a multiple of the round, so the boundaries are the same"""
    frames = AG.anchor_frames(oracle, name, est, rng, first)
    tol = AG.ANCHOR_TOL[(name, est, rng, first)]
    one, res, _ = AG.anchor_expected(oracle, name, est, rng, first)
    two = AG.new_triple(16, 12)
    r1 = AG.render_adaptive_group_layers(two, frames, first, 20, tol, **AG.ANCHOR_ARGS)
    r2 = AG.render_adaptive_group_layers(two, frames, first + 20, 28, tol, **AG.ANCHOR_ARGS)
    for k in (0, 1, 2):
        assert AL.same_state(one[k], two[k].acc, two[k].records()) is None, k
    assert r1["samples"] + r2["samples"] == res["samples"] and r1["rounds"] + r2["rounds"] == res["rounds"] and r2["active_left"] == res["active_left"]
    # ... and not at any other place: a first call of 18 frames ends with a round of two
    odd = AG.new_triple(16, 12)
    AG.render_adaptive_group_layers(odd, frames, first, 18, tol, **AG.ANCHOR_ARGS)
    AG.render_adaptive_group_layers(odd, frames, first + 18, 30, tol, **AG.ANCHOR_ARGS)
    assert any(AL.same_state(one[k], odd[k].acc, odd[k].records()) is not None for k in (0, 1, 2))


@pytest.mark.parametrize("out", (0, 1, 2), ids=AG.PLANES)
def test_a_large_floor_leaves_the_two_plane_restatement(oracle, out):
    """floor_y[out] = 1e30f with rel_tol[out] > 0: plane `out`'s third of the decision holds from two samples on, so the call is
    adaptive_planes_lib.render_adaptive_planes on the other two planes' frames -- the merged two-plane restatement pins this one"""
    name, est, rng, first = key = AG.ANCHORS[0]
    frames = AG.anchor_frames(oracle, name, est, rng, first)
    tol, fl = AG.ANCHOR_TOL[key], AG.ANCHOR_ARGS["floor_y"]
    keep = [k for k in (0, 1, 2) if k != out]
    st = AG.new_triple(16, 12)
    floors = tuple(AG.BIG_FLOOR if k == out else fl[k] for k in (0, 1, 2))
    res = AG.render_adaptive_group_layers(st, frames, first, AG.ANCHOR_FRAMES, tol, floors, 8, 4)
    pair = AP.new_pair(16, 12)
    want = AP.render_adaptive_planes(pair, lambda f: tuple(frames(f)[k] for k in keep), first, AG.ANCHOR_FRAMES, tuple(tol[k] for k in keep),
                                     tuple(fl[k] for k in keep), 8, 4)
    assert res == want
    for j, k in enumerate(keep):
        assert AL.same_state(pair[j], st[k].acc, st[k].records()) is None, (out, k)
    assert np.array_equal(st[out].flags, pair[0].flags) and np.array_equal(st[out].n, pair[0].n)
    assert 0 < int((pair[0].flags & 1).sum()) < 16 * 12
