"""Adaptive sampling on half-buffers (include/volpath.h vp_render_adaptive_halves, vp_render_adaptive_planes_halves; DESIGN.md section
2.20) without a GPU: the ABI and its Python mirror, every refusal that comes before the device, the driver's flags and refusals, and the
numpy restatement (tests/adaptive_halves_lib.py) on the CPU oracle's frames -- the pooled rule, the round loop, resumption, shards and
the census that the GPU anchors rest on."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import adaptive_halves_lib as AH
import adaptive_lib as AL
import halves_lib as HL
import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cuda-volpath_amd", "volpath_render")
E_ARG = -3
W, H = AL.ANCHOR_W, AL.ANCHOR_H
BEAUTY, PLANES = "vp_render_adaptive_halves", "vp_render_adaptive_planes_halves"
MODES = {1: 2, 2: 2, 3: 3}       # mode: its planes
NAN = float("nan")


# ---- the C ABI without a device
def test_symbols_and_mirrors():
    import volpath
    text = open(os.path.join(ROOT, "include", "volpath.h")).read()
    for sym in (BEAUTY, PLANES):
        assert sym in volpath.PART2_SYMBOLS and hasattr(volpath.lib(), sym), sym
        assert re.search(r"\bint\s+%s\s*\(" % sym, text), sym
    for name in ("render_adaptive_halves", "render_adaptive_planes_halves"):
        assert callable(getattr(volpath, name)), name
    # the structs both calls reuse, as the header declares them on this ABI
    assert C.sizeof(volpath.Adaptive) == 16 and C.sizeof(volpath.AdaptivePlanes3) == 32 and C.sizeof(volpath.AdaptiveResult) == 24
    assert C.sizeof(volpath.PlaneBufs) == 6 * C.sizeof(C.c_void_p) == 48 and C.sizeof(volpath.PixelStats) == 24
    assert volpath.AdaptivePlanes3.floor_y.offset == 12 and volpath.AdaptivePlanes3.min_frames.offset == 24 and volpath.AdaptivePlanes3.round_frames.offset == 28
    flat = " ".join(text.split()).replace(" * ", " ")
    for phrase in ("ACTIVE while the FROZEN bit is clear in ALL 2N of its records", "r0.n >= 2 and r1.n >= 2", "conservative for noise", "across processes",
                   "FILTERED error estimate", "VP_ARITH_FAST on plane modes"):
        assert phrase in flat, phrase
    assert not re.search(r"[Nn]ot built: [^.]*adaptive rounds on halves", flat)


def test_the_beauty_call_refuses_its_arguments_before_the_device():
    """every VP_E_ARG refusal of the header, with pointers that must never be followed; *result is zeroed by each"""
    import volpath
    L = volpath.lib()
    h0, h1, s0, s1 = (C.c_void_p(a) for a in (0x1000, 0x2000, 0x3000, 0x4000))
    P = volpath.make_param(16, 12)

    def call(a=h0, b=h1, ra=s0, rb=s1, first=0, n=8, p=C.byref(P), tol=0.1, fl=1e-3, min_frames=4, round_frames=4, null_a=False):
        ad = volpath.Adaptive(tol, fl, min_frames, round_frames)
        res = volpath.AdaptiveResult(7, 7, 7, 7)
        rc = L.vp_render_adaptive_halves(a, b, ra, rb, first, n, p, None if null_a else C.byref(ad), C.byref(res))
        assert res.as_dict() == {"samples": 0, "rounds": 0, "active_left": 0, "frames_used": 0}
        return rc

    for kw in (dict(a=None), dict(b=None), dict(ra=None), dict(rb=None), dict(p=None), dict(null_a=True)):
        assert call(**kw) == E_ARG, kw
        assert BEAUTY in L.vp_last_error().decode() and "null" in L.vp_last_error().decode()
    assert call(b=h0) == E_ARG and "different buffers" in L.vp_last_error().decode()
    assert call(rb=s0) == E_ARG and "different buffers" in L.vp_last_error().decode()
    for kw, word in ((dict(n=0), "out of range"), (dict(n=-3), "out of range"), (dict(first=-1), "out of range"), (dict(min_frames=1), "min_frames"),
                     (dict(round_frames=0), "round_frames"), (dict(tol=-0.1), "rel_tol"), (dict(tol=NAN), "rel_tol"), (dict(fl=-1.0), "floor_y"), (dict(fl=NAN), "floor_y")):
        assert call(**kw) == E_ARG, kw
        msg = L.vp_last_error().decode()
        assert BEAUTY in msg and word in msg, (kw, msg)
    assert L.vp_render_adaptive_halves(h0, h1, s0, s1, 0, 0, C.byref(P), C.byref(volpath.Adaptive(0.1, 1e-3, 4, 4)), None) == E_ARG      # result may be NULL
    with pytest.raises(volpath.VolpathError, match=BEAUTY):
        volpath.render_adaptive_halves(h0, h0, s0, s1, 0, 8, P, 0.1)


def _bufs(volpath, base, n, garbage=True):
    """poisoned pointers, never dereferenced: plane k's accumulator at base + 0x100 k, its records 0x80 behind; beyond the mode's planes
    a non-NULL garbage entry"""
    b = volpath.PlaneBufs()
    for k in range(3):
        if k < n or garbage:
            b.acc[k] = base + 0x100 * k if k < n else 0xdead0
            b.rec[k] = base + 0x100 * k + 0x80 if k < n else 0xdead8
    return b


@pytest.mark.parametrize("mode", sorted(MODES))
def test_the_plane_call_refuses_its_arguments_before_the_device(mode):
    import volpath
    L = volpath.lib()
    n = MODES[mode]
    P = volpath.make_param(16, 12)

    def call(h0=None, h1=None, m=mode, first=0, frames=8, p=C.byref(P), tol=(0.1, 0.1, 0.1), fl=(1e-3, 1e-3, 1e-2), min_frames=4, round_frames=4, null=()):
        h0 = h0 if h0 is not None else _bufs(volpath, 0x10000, n)
        h1 = h1 if h1 is not None else _bufs(volpath, 0x20000, n)
        ad = volpath.AdaptivePlanes3((C.c_float * 3)(*tol), (C.c_float * 3)(*fl), min_frames, round_frames)
        res = volpath.AdaptiveResult(7, 7, 7, 7)
        rc = L.vp_render_adaptive_planes_halves(m, None if "h0" in null else C.byref(h0), None if "h1" in null else C.byref(h1), first, frames, p,
                                                None if "a" in null else C.byref(ad), C.byref(res))
        assert res.as_dict() == {"samples": 0, "rounds": 0, "active_left": 0, "frames_used": 0}
        return rc

    for null in ("h0", "h1", "a"):
        assert call(null=(null,)) == E_ARG and PLANES in L.vp_last_error().decode(), null
    assert call(p=None) == E_ARG and PLANES in L.vp_last_error().decode()
    for bad_mode in (0, 4, -1, 7):
        assert call(m=bad_mode) == E_ARG and "mode" in L.vp_last_error().decode(), bad_mode
    for h in (0, 1):
        for k in range(n):
            for field in ("acc", "rec"):
                b = [_bufs(volpath, 0x10000, n), _bufs(volpath, 0x20000, n)]
                getattr(b[h], field)[k] = None                                                      # a NULL used entry
                assert call(b[0], b[1]) == E_ARG and "null" in L.vp_last_error().decode(), (h, k, field)
                b = [_bufs(volpath, 0x10000, n), _bufs(volpath, 0x20000, n)]
                getattr(b[h], field)[k] = getattr(b[1 - h], field)[(k + 1) % n]                      # the same buffer across the halves
                assert call(b[0], b[1]) == E_ARG and "different buffers" in L.vp_last_error().decode(), (h, k, field)
                b = [_bufs(volpath, 0x10000, n), _bufs(volpath, 0x20000, n)]
                getattr(b[h], field)[k] = getattr(b[h], field)[(k + 1) % n]                          # ... and within a half
                assert call(b[0], b[1]) == E_ARG and "different buffers" in L.vp_last_error().decode(), (h, k, field)
    for kw, word in ((dict(frames=0), "out of range"), (dict(first=-1), "out of range"), (dict(min_frames=1), "min_frames"), (dict(round_frames=0), "round_frames")):
        assert call(**kw) == E_ARG and word in L.vp_last_error().decode(), kw
    for k in range(n):
        for field, bad in (("tol", -1.0), ("tol", NAN), ("fl", -1e-3), ("fl", NAN)):
            v = [0.1, 0.1, 0.1]
            v[k] = bad
            assert call(**{field: tuple(v)}) == E_ARG, (k, field, bad)
            assert "plane %d" % k in L.vp_last_error().decode()
    # entries of the vp_plane_bufs beyond the mode's planes are ignored -- garbage, the pointer of a used entry, NULL.  Shown without a
    # device: the frame range is checked after the buffers, so its message is the one that comes (a call that passed every check would
    # go on to the device with these pointers; unused tolerances and floors of NaN are given to the GPU cases instead)
    for k in range(n, 3):
        for fill in (0x10000, None):
            b = [_bufs(volpath, 0x10000, n), _bufs(volpath, 0x20000, n)]
            for h in (0, 1):
                b[h].acc[k] = fill
                b[h].rec[k] = fill + 0x80 if fill else None
            assert call(b[0], b[1], frames=0) == E_ARG and "out of range" in L.vp_last_error().decode(), (k, fill)
    with pytest.raises(volpath.VolpathError, match=PLANES):
        volpath.render_adaptive_planes_halves(mode, [(0x1000, 0x2000)] * n, [(0x3000, 0x4000)] * n, 0, 8, P, (0.1,) * n, (1e-3,) * n)


# ---- the driver
CROSS = {"--layers-denoise-cross": ["--layers-out", "l"], "--groups-denoise-cross": ["--groups-out", "g"], "--planes-denoise-cross": ["--planes-out", "p"]}
NOISE = {"--layers-denoise-cross": ["--plane-cross-noise", "0.1", "0.1"], "--groups-denoise-cross": ["--plane-cross-noise", "0.1", "0.1"],
         "--planes-denoise-cross": ["--planes-cross-noise", "0.1", "0.1", "0.1"]}


def _run(*args):
    return subprocess.run([EXE] + list(args), capture_output=True, text=True)


def test_cli_the_new_flags_are_in_the_usage_text():
    r = _run("--help")
    assert r.returncode == 0
    for flag in ("--cross-noise TOL", "--cross-noise-out", "--plane-cross-noise TOL0 TOL1", "--planes-cross-noise TOL_SUN TOL_SKY TOL_TRANS", "--plane-cross-noise-out",
                 BEAUTY, PLANES):
        assert flag in r.stdout, flag


def test_cli_the_new_flags_parse():
    """a bad operand is refused by name with the usage text; a good one passes the parser (what then refuses the line is a conflict)"""
    for bad in (["--cross-noise", "-1"], ["--cross-noise", "x"], ["--cross-noise", "nan"], ["--plane-cross-noise", "0.1", "-1"], ["--planes-cross-noise", "0.1", "0.1", "nan"]):
        r = _run(*bad)
        assert r.returncode == 2 and bad[0] + " " + bad[-1] in r.stderr and "volpath_render [" in r.stdout, (bad, r.stderr)
    for missing in (["--cross-noise"], ["--plane-cross-noise", "0.1"], ["--planes-cross-noise", "0.1", "0.1"], ["--cross-noise-out"], ["--plane-cross-noise-out"]):
        assert _run(*missing).returncode == 2, missing
    # --cross-noise implies --denoise-cross (and with it --denoise)
    src = open(os.path.join(ROOT, "cuda-volpath_amd", "host", "main.cpp")).read()
    assert re.search(r'a == "--cross-noise"\).*cross_adaptive\s*=\s*denoise_cross\s*=\s*denoise\s*=\s*true', src)
    r = _run("--cross-noise", "0.1", "--layers-out", "l")
    assert r.returncode == 2 and "--denoise-cross with --layers-out" in r.stderr                    # ... so --denoise-cross's refusals apply
    for extra in (["--min-spp", "1"], ["--round", "0"]):
        r = _run("--cross-noise", "0.1", *extra)
        assert r.returncode == 2 and "--cross-noise needs --min-spp >= 2 and --round >= 1" in r.stderr, r.stderr


def test_cli_the_new_refusals():
    for extra, named in ((["--gpus", "2"], "--gpus"), (["--noise", "0.1"], "--noise")):
        r = _run("--cross-noise", "0.1", *extra)
        assert r.returncode == 2 and r.stderr.startswith("--cross-noise with %s:" % named), (extra, r.stderr)
    for flag in sorted(CROSS):
        base = [flag] + CROSS[flag] + NOISE[flag]
        adaptive = ["--planes-noise", "0.1", "0.1", "0.1"] if flag == "--planes-denoise-cross" else ["--plane-noise", "0.1", "0.1"]
        for extra, named in ((["--gpus", "2"], "--gpus"), (["--noise", "0.1"], "--noise"), (adaptive, adaptive[0])):
            r = _run(*base, *extra)
            assert r.returncode == 2 and r.stderr.startswith("%s with %s:" % (NOISE[flag][0], named)), (flag, extra, r.stderr)
        # --cross-noise is the beauty image's
        r = _run(flag, *CROSS[flag], "--cross-noise", "0.1")
        assert r.returncode == 2 and r.stderr.startswith("--cross-noise with %s:" % flag), r.stderr
        # a flag of the wrong mode, and a flag without its cross-filter
        wrong = ["--plane-cross-noise", "0.1", "0.1"] if flag == "--planes-denoise-cross" else ["--planes-cross-noise", "0.1", "0.1", "0.1"]
        r = _run(flag, *CROSS[flag], *wrong)
        assert r.returncode == 2 and r.stderr.startswith(wrong[0] + " needs "), (flag, r.stderr)
        r = _run(*CROSS[flag], *NOISE[flag])
        assert r.returncode == 2 and r.stderr.startswith(NOISE[flag][0] + " needs "), (flag, r.stderr)
    for lone, needs in ((["--cross-noise-out", "c.hdr"], "--cross-noise"), (["--plane-cross-noise-out", "n"], "--plane-cross-noise")):
        r = _run(*lone)
        assert r.returncode == 2 and lone[0] + " needs " + needs in r.stderr, r.stderr


def test_cli_the_old_refusals_stand_word_for_word():
    """--noise, --plane-noise and --planes-noise with any -denoise-cross flag: the messages of the parent commit"""
    r = _run("--denoise-cross", "--noise", "0.1")
    assert r.returncode == 2 and r.stderr == (
        "--denoise-cross with --noise: the half-buffers' records are not reduced across ranks, adaptive rounds on halves are not built and the halves are "
        "the beauty image's, not a plane's; use one GPU without --noise and without plane outputs or plane filters\n")
    for flag in sorted(CROSS):
        adaptive = ["--planes-noise", "0.1", "0.1", "0.1"] if flag == "--planes-denoise-cross" else ["--plane-noise", "0.1", "0.1"]
        for extra, named in ((["--noise", "0.1"], "--noise"), (adaptive, adaptive[0])):
            r = _run(flag, *CROSS[flag], *extra)
            assert r.returncode == 2 and r.stderr == (
                "%s with %s: the halves' records are not reduced across ranks, adaptive rounds on halves are not built and the beauty image's halves are "
                "its own; use one GPU without --noise, --plane-noise, --planes-noise and --denoise-cross / -var / -select\n" % (flag, named)), (flag, extra, r.stderr)


# ---- the restatement on the oracle's frames
ANCHORS = [(AL.ANCHOR1, 0), (AL.ANCHOR1, 1), (AL.ANCHOR2, 0)]
_RUNS = {}


def _anchor_run(oracle, anchor, first):
    key = (anchor["est"], first)
    if key not in _RUNS:
        frames = AH.beauty(AH.anchor_frames(oracle, scenes, anchor))
        st = AH.new_halves(W, H)
        res = AH.render_adaptive_halves(st, frames, first, anchor["max_frames"], **AL.anchor_args(anchor))
        _RUNS[key] = (frames, st, res)
    return _RUNS[key]


@pytest.mark.parametrize("anchor,first", ANCHORS, ids=["anchor1-from0", "anchor1-from1", "anchor2"])
def test_the_anchors_exercise_every_path(oracle, anchor, first):
    """a condition on the inputs of the GPU anchors: pixels frozen at min_frames, frozen strictly between, pixels with all frames, pixels
    still active -- and both halves fed"""
    _, st, res = _anchor_run(oracle, anchor, first)
    c = AH.census(st, anchor["min_frames"], anchor["max_frames"])
    print(anchor["est"], first, c, res)
    assert c["at_min"] >= 1 and c["between"] >= 1 and c["all_frames"] >= 1 and c["active"] >= 1, c
    assert res["active_left"] == c["active"] and res["frames_used"] == anchor["max_frames"]
    n0, n1 = st[0][0].n.astype(np.int64), st[1][0].n.astype(np.int64)
    assert res["samples"] == int((n0 + n1).sum())
    assert (np.abs(n0 - n1) <= 1).all() and (n0 != n1).any() == (anchor["round_frames"] % 2 == 1)      # whole rounds of an even length feed the halves equally
    frozen = AH.frozen_mask(st)
    assert ((n0 + n1)[frozen] >= anchor["min_frames"]).all() and (n0[frozen] >= 2).all() and (n1[frozen] >= 2).all()


def test_the_pooled_rule_is_the_criterion_on_the_accumulated_records(oracle):
    a = AL.ANCHOR1
    frames, _, _ = _anchor_run(oracle, a, 0)
    st = AH.new_halves(W, H)
    AH.add_round(st, frames, 0, 24, AL.all_pixels(W, H))
    r0, r1 = st[0][0], st[1][0]
    both = HL.accumulate_stats(r0.records(), r1.records())
    for tol in (0.05, 0.1, 0.3):
        for min_frames in (2, 24, 25):
            want = (r0.n >= 2) & (r1.n >= 2) & (both["n"] >= min_frames) & AL.criterion(both["sum_y"], both["sum_y2"], both["n"], tol, a["floor_y"])
            got = AH.plane_ok(r0, r1, tol, a["floor_y"], min_frames)
            assert np.array_equal(got, want) and (got.any() and not got.all() or min_frames == 25 and not got.any()), (tol, min_frames)
    # a half with fewer than two samples holds the pixel back whatever the other half says
    one = AH.new_halves(W, H)
    AH.add_round(one, frames, 0, 1, AL.all_pixels(W, H))
    AH.add_round(one, frames, 1, 1, AL.all_pixels(W, H))
    AH.add_round(one, frames, 3, 1, AL.all_pixels(W, H))
    AH.add_round(one, frames, 5, 1, AL.all_pixels(W, H))
    assert (one[0][0].n == 1).all() and (one[1][0].n == 3).all()
    assert not AH.plane_ok(one[0][0], one[1][0], 1e30, 1e30, 2).any()


def test_rounds_by_hand_equal_the_loop(oracle):
    a = AL.ANCHOR2
    frames, want, res = _anchor_run(oracle, a, 0)
    st = AH.new_halves(W, H)
    owned = AL.all_pixels(W, H)
    samples = 0
    for k in range(a["max_frames"] // a["round_frames"]):
        active = AH.active_mask(st, owned)
        for f in range(k * a["round_frames"], (k + 1) * a["round_frames"]):
            st[f & 1][0].add_frame(frames(f)[0], active)
        samples += int(active.sum()) * a["round_frames"]
        r0, r1 = st[0][0], st[1][0]
        n = r0.n + r1.n
        ok = active & (r0.n >= 2) & (r1.n >= 2) & (n >= a["min_frames"]) & AL.criterion(r0.sum_y + r1.sum_y, r0.sum_y2 + r1.sum_y2, n, a["rel_tol"], a["floor_y"])
        r0.flags[ok] |= 1
        r1.flags[ok] |= 1
    for h in (0, 1):
        assert AL.same_state(want[h][0], st[h][0].acc, st[h][0].records()) is None
    assert samples == res["samples"] and res["rounds"] == a["max_frames"] // a["round_frames"]


@pytest.mark.parametrize("first", [0, 1])
def test_resuming_equals_one_call_when_the_round_divides_the_first_call(oracle, first):
    a = AL.ANCHOR1
    frames, want, res = _anchor_run(oracle, a, first)
    args = AL.anchor_args(a)
    st = AH.new_halves(W, H)
    r1 = AH.render_adaptive_halves(st, frames, first, 40, **args)
    r2 = AH.render_adaptive_halves(st, frames, first + 40, a["max_frames"] - 40, **args)
    assert 40 % a["round_frames"] == 0
    for h in (0, 1):
        assert AL.same_state(want[h][0], st[h][0].acc, st[h][0].records()) is None
    assert r1["samples"] + r2["samples"] == res["samples"] and r1["rounds"] + r2["rounds"] == res["rounds"] and r2["active_left"] == res["active_left"]
    # ... and not when it does not: a decision falls after 44 frames that the one call never takes
    st = AH.new_halves(W, H)
    AH.render_adaptive_halves(st, frames, first, 44, **args)
    AH.render_adaptive_halves(st, frames, first + 44, a["max_frames"] - 44, **args)
    assert any(AL.same_state(want[h][0], st[h][0].acc, st[h][0].records()) is not None for h in (0, 1))


def test_shards_partition_the_render(oracle):
    import volpath
    a = AL.ANCHOR2
    frames, want, res = _anchor_run(oracle, a, 0)
    st = AH.new_halves(W, H)
    samples = left = 0
    seen = np.zeros((H, W), int)
    for r in range(3):
        owned = AL.owned_pixels(volpath, W, H, r, 3)
        before = AH.copy_halves(st)
        out = AH.render_adaptive_halves(st, frames, 0, a["max_frames"], owned=owned, **AL.anchor_args(a))
        for h in (0, 1):
            assert st[h][0].acc[~owned].tobytes() == before[h][0].acc[~owned].tobytes() and np.array_equal(st[h][0].n[~owned], before[h][0].n[~owned])
        samples, left, seen = samples + out["samples"], left + out["active_left"], seen + owned
    assert (seen == 1).all()
    for h in (0, 1):
        assert AL.same_state(want[h][0], st[h][0].acc, st[h][0].records()) is None
    assert (samples, left) == (res["samples"], res["active_left"])


def test_plane_modes_pool_each_plane_and_and_the_planes(oracle):
    """the plane sample tables of the oracle at 16 x 12: with a large floor on all planes but one the frozen set is that plane's own
    pooled rule, and the call's frozen set is within every plane's own"""
    import adaptive_group_layers_lib as AGL
    name, est, rng, first = "soft", 0, 1, 0
    frames = AH.oracle_plane_frames(oracle, AH.GROUP_LAYERS, name, est, rng, range(first, first + AGL.ANCHOR_FRAMES))
    tol, floors = AGL.FLOOR_TOL, (1e-3, 1e-3, 1e-2)
    st = AH.new_halves(16, 12, 3)
    res = AH.render_adaptive_halves(st, frames, first, 32, tol, floors, 8, 4)
    frozen = AH.frozen_mask(st)
    assert 0 < frozen.sum() < 16 * 12 and res["rounds"] == 8
    for k in range(3):
        fl = tuple(floors[j] if j == k else AGL.BIG_FLOOR for j in range(3))
        one = AH.new_halves(16, 12, 3)
        AH.render_adaptive_halves(one, frames, first, 32, tol, fl, 8, 4)
        alone = AH.new_halves(16, 12, 1)
        AH.render_adaptive_halves(alone, lambda f, k=k: (frames(f)[k],), first, 32, tol[k], floors[k], 8, 4)
        assert np.array_equal(AH.frozen_mask(one), AH.frozen_mask(alone)) and 0 < AH.frozen_mask(alone).sum() < 16 * 12, k
        for h in (0, 1):
            assert AL.same_state(alone[h][0], one[h][k].acc, one[h][k].records()) is None
