"""Per-pixel statistics and adaptive sampling (include/volpath.h vp_pixel_stats / vp_render_adaptive) without a GPU: the record's
layout in C and in the ctypes mirror, the exported symbols, the argument refusals that come before the device, the CLI flags, and
the numpy restatement of the definition (tests/adaptive_lib.py) against the CPU oracle's per-frame renders."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import adaptive_lib as A
import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cuda-volpath_amd", "volpath_render")
NEW_SYMBOLS = ("vp_render_frames_stats", "vp_render_adaptive", "vp_scale_by_count", "vp_stats_rel_error")
E_ARG = -3


def test_record_layout_in_c(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "volpath.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %u %zu %zu\\n", sizeof(vp_pixel_stats), offsetof(vp_pixel_stats, sum_y),'
                   ' offsetof(vp_pixel_stats, sum_y2), offsetof(vp_pixel_stats, n), offsetof(vp_pixel_stats, flags), VP_STATS_FROZEN,'
                   ' sizeof(vp_adaptive), sizeof(vp_adaptive_result)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["cc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)], text=True).split()
    assert [int(v) for v in out] == [24, 0, 8, 16, 20, 1, 16, 24]


def test_record_layout_in_the_ctypes_mirror():
    import volpath
    S = volpath.PixelStats
    assert C.sizeof(S) == 24
    assert (S.sum_y.offset, S.sum_y2.offset, S.n.offset, S.flags.offset) == (0, 8, 16, 20)
    d = volpath.PIXEL_STATS_DTYPE
    assert d.itemsize == 24 and [d.fields[k][1] for k in ("sum_y", "sum_y2", "n", "flags")] == [0, 8, 16, 20]
    assert A.Stats(3, 2).records().dtype == d
    assert C.sizeof(volpath.Adaptive) == 16 and C.sizeof(volpath.AdaptiveResult) == 24
    assert volpath.STATS_FROZEN == A.FROZEN == 1


def test_new_symbols_are_declared_and_exported():
    import volpath
    text = open(os.path.join(ROOT, "include", "volpath.h")).read()
    for n in NEW_SYMBOLS:
        assert n in volpath.PART2_SYMBOLS
        assert re.search(r"\bint\s+%s\s*\(" % n, text), n
        assert hasattr(volpath.lib(), n)
    assert re.search(r"#define\s+VP_STATS_FROZEN\s+1u", text)


def test_argument_refusals_come_before_the_device():
    """every refusal of the header returns VP_E_ARG; the pointers are never followed (and no device is asked for)"""
    import volpath
    L = volpath.lib()
    P = volpath.make_param(16, 8)
    out, st = C.c_void_p(0x1000), C.c_void_p(0x2000)     # never dereferenced: each call is refused first

    def adaptive(o=out, s=st, first=0, maxf=8, p=C.byref(P), a="default", rel_tol=0.1, floor_y=1e-3, min_frames=2, round_frames=1, res=None):
        arg = C.byref(volpath.Adaptive(rel_tol, floor_y, min_frames, round_frames)) if a == "default" else a
        return L.vp_render_adaptive(o, s, first, maxf, p, arg, res)

    assert adaptive(o=None) == E_ARG
    assert adaptive(s=None) == E_ARG
    assert adaptive(p=None) == E_ARG
    assert adaptive(a=None) == E_ARG
    assert adaptive(maxf=0) == E_ARG and adaptive(maxf=-5) == E_ARG
    assert adaptive(first=-1) == E_ARG
    assert adaptive(min_frames=1) == E_ARG and adaptive(min_frames=0) == E_ARG and adaptive(min_frames=-3) == E_ARG
    assert adaptive(round_frames=0) == E_ARG and adaptive(round_frames=-1) == E_ARG
    assert adaptive(rel_tol=-0.1) == E_ARG and adaptive(rel_tol=float("nan")) == E_ARG
    assert adaptive(floor_y=-1e-3) == E_ARG and adaptive(floor_y=float("nan")) == E_ARG
    assert "vp_render_adaptive" in L.vp_last_error().decode()
    res = volpath.AdaptiveResult(7, 7, 7, 7)
    assert adaptive(maxf=0, res=C.byref(res)) == E_ARG
    assert res.as_dict() == {"samples": 0, "rounds": 0, "active_left": 0, "frames_used": 0}
    with pytest.raises(volpath.VolpathError, match="min_frames"):
        volpath.render_adaptive(out, st, 0, 8, P, 0.1, min_frames=1)
    # the uniform render and the output stage
    f = L.vp_render_frames_stats
    assert f(None, st, 0, 4, C.byref(P)) == E_ARG and f(out, None, 0, 4, C.byref(P)) == E_ARG and f(out, st, 0, 4, None) == E_ARG
    assert f(out, st, 0, 0, C.byref(P)) == E_ARG and f(out, st, -1, 4, C.byref(P)) == E_ARG
    g = L.vp_scale_by_count
    assert g(None, out, st, 4, 1.0) == E_ARG and g(out, None, st, 4, 1.0) == E_ARG and g(out, out, None, 4, 1.0) == E_ARG and g(out, out, st, -1, 1.0) == E_ARG
    h = L.vp_stats_rel_error
    assert h(None, st, 4, 1e-3) == E_ARG and h(out, None, 4, 1e-3) == E_ARG and h(out, st, -1, 1e-3) == E_ARG and h(out, st, 4, -1.0) == E_ARG


def test_cli_noise_flags():
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--noise TOL", "--min-spp", "--round", "--noise-out"):
        assert flag in r.stdout, flag
    for bad in (["--noise"], ["--noise", "-0.5"], ["--noise", "abc"], ["--noise", "0.05", "--min-spp", "1"], ["--noise", "0.05", "--round", "0"]):
        r = subprocess.run([EXE] + bad, capture_output=True, text=True)
        assert r.returncode == 2, (bad, r.stdout, r.stderr)
    # statistics are not reduced across ranks: refused with a message, before anything is rendered
    r = subprocess.run([EXE, "--noise", "0.05", "--gpus", "2"], capture_output=True, text=True)
    assert r.returncode == 2 and "--noise" in r.stderr and "--gpus" in r.stderr


# ---- the restatement against the oracle's per-frame renders
@pytest.fixture(scope="module")
def anchor1(oracle):
    osc, oP = A.anchor_oracle(oracle, scenes, A.ANCHOR1)
    return osc, oP, A.oracle_frames(osc, oP)


def test_luminance_and_criterion_are_the_written_operations():
    v = np.array([[0.3, 0.6, 0.1, 9.0], [1e-3, 2.5, 7.0, 0.0]], np.float32)
    want = [np.float32(np.float32(np.float32(0.2126) * a + np.float32(0.7152) * b) + np.float32(0.0722) * c) for a, b, c, _ in v]
    assert A.luminance(v).tolist() == [float(w) for w in want]
    # three samples 1, 2, 3: lhs = 3 * 14 - 36 = 6; m = 6; rhs = tol^2 * 2 * 36
    sy, sy2, n = np.array([6.0]), np.array([14.0]), np.array([3], np.uint32)
    t_edge = np.sqrt(6.0 / 72.0)
    assert not A.criterion(sy, sy2, n, np.float32(t_edge) * np.float32(0.999), 0.0)[0]
    assert A.criterion(sy, sy2, n, np.float32(t_edge) * np.float32(1.001), 0.0)[0]
    # the floor takes over where the mean is below it: m = n * floor
    assert A.criterion(sy, sy2, n, 0.1, 100.0)[0]          # rhs = 0.01 * 2 * 300^2 = 1800 >= 6
    # the arguments are the binary32 values widened, not the decimal literals
    tol = np.float64(np.float32(0.1))
    assert tol != 0.1
    # NaN on either side: not frozen
    assert not A.criterion(np.array([np.nan]), sy2, n, 0.1, 0.0)[0]
    assert not A.criterion(np.array([np.inf]), np.array([np.inf]), n, 0.1, 0.0)[0]


def test_uniform_restatement_is_the_oracle_accumulator(anchor1):
    osc, oP, frame = anchor1
    st = A.render_uniform(A.Stats(A.ANCHOR_W, A.ANCHOR_H), frame, 3, 9)
    ref = None
    for f in range(3, 12):
        ref, _ = osc.render_frame(oP, f, ref)
    assert st.acc.tobytes() == ref.tobytes()
    assert (st.n == 9).all() and not st.flags.any()
    # the sums are those of the nine luminances, one after the other, in float64
    y = [A.luminance(frame(f)).astype(np.float64) for f in range(3, 12)]
    s = np.zeros_like(y[0]); s2 = np.zeros_like(y[0])
    for v in y:
        s = s + v; s2 = s2 + v * v
    assert A.equal_bits(st.sum_y, s) and A.equal_bits(st.sum_y2, s2)
    assert (st.sum_y > 0).any()


def test_anchor_figures(anchor1, oracle):
    """the oracle's expectation for both anchors: what keeps the GPU comparison from passing trivially"""
    osc, oP, frame = anchor1
    st = A.Stats(A.ANCHOR_W, A.ANCHOR_H)
    r = A.render_adaptive(st, frame, 0, A.ANCHOR1["max_frames"], **A.anchor_args(A.ANCHOR1))
    c = A.census(st, A.ANCHOR1["min_frames"], A.ANCHOR1["max_frames"])
    print("anchor 1:", r, c)
    assert c["at_min"] >= 2000 and c["between"] >= 150 and c["active"] >= 40
    assert r["samples"] == c["samples"] == int(st.n.sum()) and r["active_left"] == c["active"]
    assert (c["at_min"], c["between"], c["all_frames"], c["active"], r["samples"]) == (2771, 238, 63, 51, 64088)
    assert set(c["per_boundary"]) == set(range(24, 96, 8)) and 15 <= min(c["per_boundary"].values()) and max(c["per_boundary"].values()) <= 41
    osc2, oP2 = A.anchor_oracle(oracle, scenes, A.ANCHOR2)
    st2 = A.Stats(A.ANCHOR_W, A.ANCHOR_H)
    r2 = A.render_adaptive(st2, A.oracle_frames(osc2, oP2), 0, A.ANCHOR2["max_frames"], **A.anchor_args(A.ANCHOR2))
    c2 = A.census(st2, A.ANCHOR2["min_frames"], A.ANCHOR2["max_frames"])
    print("anchor 2:", r2, c2)
    assert c2["at_min"] >= 2000 and c2["between"] >= 100 and c2["active"] >= 8
    assert (c2["at_min"], c2["between"], c2["all_frames"], c2["active"], r2["samples"]) == (2883, 174, 15, 12, 26500)


def test_rounds_by_hand_equal_the_loop(anchor1):
    _, _, frame = anchor1
    a = A.ANCHOR1
    st = A.Stats(A.ANCHOR_W, A.ANCHOR_H)
    r = A.render_adaptive(st, frame, 0, 40, **A.anchor_args(a))
    hand = A.Stats(A.ANCHOR_W, A.ANCHOR_H)
    samples = 0
    for k in range(5):
        active = (hand.flags & A.FROZEN) == 0
        for f in range(8 * k, 8 * k + 8):
            hand.add_frame(frame(f), active)
        samples += 8 * int(active.sum())
        A.freeze_round(hand, active, a["rel_tol"], a["floor_y"], a["min_frames"])
    assert A.same_state(st, hand.acc, hand.records()) is None
    assert r == {"samples": samples, "rounds": 5, "active_left": int(((hand.flags & 1) == 0).sum()), "frames_used": 40}
    # a frozen pixel has received nothing since: n is a round boundary at or above min_frames, and every record says so
    frozen = (st.flags & 1) != 0
    assert frozen.any() and (st.n[frozen] % 8 == 0).all() and (st.n[frozen] >= 16).all() and (st.n[~frozen] == 40).all()


def test_huge_tolerance_freezes_everything_at_the_first_boundary_at_or_above_min_frames(anchor1):
    _, _, frame = anchor1
    for min_frames, B, want in ((16, 8, 16), (10, 4, 12), (2, 5, 5), (7, 7, 7)):
        st = A.Stats(A.ANCHOR_W, A.ANCHOR_H)
        r = A.render_adaptive(st, frame, 0, 30, 1e18, 1e-3, min_frames, B)
        assert (st.n == want).all() and (st.flags == 1).all(), (min_frames, B)
        assert r == {"samples": want * A.ANCHOR_W * A.ANCHOR_H, "rounds": want // B, "active_left": 0, "frames_used": want}
        # everything frozen: a further call renders nothing
        before = st.copy()
        assert A.render_adaptive(st, frame, want, 30, 1e18, 1e-3, min_frames, B) == {"samples": 0, "rounds": 0, "active_left": 0, "frames_used": 0}
        assert A.same_state(before, st.acc, st.records()) is None


def test_resuming_equals_one_call_when_the_round_divides_the_first_call(anchor1):
    _, _, frame = anchor1
    args = A.anchor_args(A.ANCHOR1)
    one = A.Stats(A.ANCHOR_W, A.ANCHOR_H)
    r = A.render_adaptive(one, frame, 0, 64, **args)
    two = A.Stats(A.ANCHOR_W, A.ANCHOR_H)
    r1 = A.render_adaptive(two, frame, 0, 24, **args)
    r2 = A.render_adaptive(two, frame, 24, 40, **args)
    assert A.same_state(one, two.acc, two.records()) is None
    assert r1["samples"] + r2["samples"] == r["samples"] and r1["rounds"] + r2["rounds"] == r["rounds"] and r2["active_left"] == r["active_left"]
    # ... and not otherwise: a first call of 20 frames ends with a round of four, whose boundary the single call does not have
    odd = A.Stats(A.ANCHOR_W, A.ANCHOR_H)
    A.render_adaptive(odd, frame, 0, 20, **args)
    A.render_adaptive(odd, frame, 20, 44, **args)
    assert A.same_state(one, odd.acc, odd.records()) is not None


def test_shards_partition_the_adaptive_render(anchor1):
    import volpath
    _, _, frame = anchor1
    args = A.anchor_args(A.ANCHOR1)
    whole = A.Stats(A.ANCHOR_W, A.ANCHOR_H)
    r = A.render_adaptive(whole, frame, 0, 48, **args)
    parts = A.Stats(A.ANCHOR_W, A.ANCHOR_H)
    total = 0
    for rank in range(3):
        total += A.render_adaptive(parts, frame, 0, 48, owned=A.owned_pixels(volpath, A.ANCHOR_W, A.ANCHOR_H, rank, 3), **args)["samples"]
    assert A.same_state(whole, parts.acc, parts.records()) is None and total == r["samples"]


def test_output_stage_restatement():
    rng = np.random.default_rng(5)
    src = rng.random((4, 6, 4), np.float32) * 100
    n = rng.integers(0, 50, (4, 6)).astype(np.uint32)
    n[0, 0] = 0; n[1, 1] = 1
    out = A.scale_by_count(src, n, 1.0)
    assert not out[0, 0].any() and np.array_equal(out[1, 1], src[1, 1])
    k = (2, 3)
    assert out[k][2] == src[k][2] * (np.float32(1.0) / np.float32(n[k]))
    # the noise map of a pixel with samples 1, 2, 3: variance of the mean = 1 / 3, mean 2
    e = A.rel_error(np.array([6.0, 6.0, 0.5]), np.array([14.0, 14.0, 0.25]), np.array([3, 1, 1], np.uint32), 1e-3)
    assert e[1] == 0 and e[2] == 0 and abs(e[0] - np.sqrt(1.0 / 3.0) / 2.0) < 1e-15
