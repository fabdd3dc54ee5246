"""Half-buffer renders of plane calls (include/volpath.h vp_render_frames_planes_halves_stats) without a GPU: the
ABI and its Python mirror, every refusal that comes before the device, and the driver's flags and refusals."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cuda-volpath_amd", "volpath_render")
E_ARG = -3
SYM = "vp_render_frames_planes_halves_stats"
MODES = {1: 2, 2: 2, 3: 3}       # mode: its planes
CROSS_FLAGS = {"--layers-denoise-cross": ["--layers-out", "l"], "--groups-denoise-cross": ["--groups-out", "g"], "--planes-denoise-cross": ["--planes-out", "p"]}


def test_symbol_and_mirror():
    import volpath
    text = open(os.path.join(ROOT, "include", "volpath.h")).read()
    assert SYM in volpath.PART2_SYMBOLS and hasattr(volpath.lib(), SYM)
    assert re.search(r"\bint\s+%s\s*\(" % SYM, text)
    for name, value in (("VP_PLANES_LAYERS", 1), ("VP_PLANES_GROUPS", 2), ("VP_PLANES_GROUP_LAYERS", 3)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), text), name
        assert getattr(volpath, name[3:]) == value
    assert re.search(r"typedef struct \{ vp_float4\* acc\[3\]; vp_pixel_stats\* rec\[3\]; \} vp_plane_bufs;", text)
    # two arrays of three pointers: the struct of the header on this ABI
    assert C.sizeof(volpath.PlaneBufs) == 6 * C.sizeof(C.c_void_p) == 48
    assert volpath.PlaneBufs.acc.offset == 0 and volpath.PlaneBufs.rec.offset == 3 * C.sizeof(C.c_void_p)
    for name in ("render_frames_planes_halves_stats", "denoise_cross_planes", "plane_bufs"):
        assert callable(getattr(volpath, name)), name
    assert {m: len(volpath.PLANE_NAMES[m]) for m in MODES} == MODES
    assert volpath.PLANE_NAMES[3] == ("sun", "sky", "trans") and volpath.PLANE_NAMES[1] == ("fg", "trans") and volpath.PLANE_NAMES[2] == ("sun", "sky")
    assert volpath.PLANE_RESID_FLOOR["trans"] == 1e-2 and all(volpath.PLANE_RESID_FLOOR[n] == 1e-3 for n in ("fg", "sun", "sky"))
    b = volpath.plane_bufs([(0x10, 0x20), (C.c_void_p(0x30), 0x40)])
    assert [b.acc[0], b.acc[1], b.acc[2], b.rec[0], b.rec[1], b.rec[2]] == [0x10, 0x30, None, 0x20, 0x40, None]


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
def test_argument_refusals_come_before_the_device(mode):
    """every VP_E_ARG refusal of the header, with pointers that must never be followed; every call here is refused before the device"""
    import volpath
    L = volpath.lib()
    n = MODES[mode]
    P = volpath.make_param(16, 12)

    def call(h0=None, h1=None, m=mode, first=0, frames=4, p=C.byref(P), null0=False, null1=False):
        h0 = h0 if h0 is not None else _bufs(volpath, 0x10000, n)
        h1 = h1 if h1 is not None else _bufs(volpath, 0x20000, n)
        return L.vp_render_frames_planes_halves_stats(m, None if null0 else C.byref(h0), None if null1 else C.byref(h1), first, frames, p)

    assert call(null0=True) == E_ARG and call(null1=True) == E_ARG and call(p=None) == E_ARG
    assert SYM in L.vp_last_error().decode()
    assert call(frames=0) == E_ARG and call(frames=-3) == E_ARG and call(first=-1) == E_ARG
    assert SYM in L.vp_last_error().decode()
    for bad_mode in (0, 4, -1, 7):
        assert call(m=bad_mode) == E_ARG, bad_mode
    assert "mode" in L.vp_last_error().decode()
    for h in (0, 1):
        for k in range(n):
            for field in ("acc", "rec"):
                # a NULL used entry
                b = [_bufs(volpath, 0x10000, n), _bufs(volpath, 0x20000, n)]
                getattr(b[h], field)[k] = None
                assert call(b[0], b[1]) == E_ARG, (h, k, field)
                # the same buffer across the two halves
                b = [_bufs(volpath, 0x10000, n), _bufs(volpath, 0x20000, n)]
                getattr(b[h], field)[k] = getattr(b[1 - h], field)[(k + 1) % n]
                assert call(b[0], b[1]) == E_ARG, (h, k, field)
                # ... and within a half
                b = [_bufs(volpath, 0x10000, n), _bufs(volpath, 0x20000, n)]
                getattr(b[h], field)[k] = getattr(b[h], field)[(k + 1) % n]
                assert call(b[0], b[1]) == E_ARG, (h, k, field)
    assert "different buffers" in L.vp_last_error().decode()
    # entries beyond the mode's planes are ignored: garbage there -- the pointer of a used entry, which would be "one buffer given twice"
    # if it were looked at -- or NULL passes the buffer checks.  Shown without a device: the frame range is checked after the buffers,
    # so its message is the one that comes (a call that passed every check would go on to the device with these pointers)
    for k in range(n, 3):
        for fill in (0x10000, None):
            b = [_bufs(volpath, 0x10000, n), _bufs(volpath, 0x20000, n)]
            for h in (0, 1):
                b[h].acc[k] = fill
                b[h].rec[k] = fill + 0x80 if fill else None
            assert call(b[0], b[1], frames=0) == E_ARG
            assert "out of range" in L.vp_last_error().decode(), (k, fill, L.vp_last_error().decode())
    b = [_bufs(volpath, 0x10000, n), _bufs(volpath, 0x20000, n)]
    b[1].acc[n - 1] = b[0].acc[0]
    assert call(b[0], b[1], frames=0) == E_ARG and "different buffers" in L.vp_last_error().decode()      # (the order the lines above rest on)
    with pytest.raises(volpath.VolpathError, match=SYM):
        volpath.render_frames_planes_halves_stats(mode, [(0x1000, 0x2000)] * n, [(0x3000, 0x4000)] * n, 0, 4, P)      # (the same pair n times)


def test_the_flags_are_in_the_usage_text():
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in list(CROSS_FLAGS) + ["--plane-denoise-var", "--plane-resid-out"]:
        assert flag in r.stdout, flag
    assert SYM in r.stdout


@pytest.mark.parametrize("flag", sorted(CROSS_FLAGS))
def test_new_refusals_exit_with_2_and_name_both_flags(flag):
    base = [EXE, flag] + CROSS_FLAGS[flag]
    adaptive = ["--planes-noise", "0.1", "0.1", "0.1"] if flag == "--planes-denoise-cross" else ["--plane-noise", "0.1", "0.1"]
    for extra, named in ((["--gpus", "2"], "--gpus"), (["--noise", "0.1"], "--noise"), (adaptive, adaptive[0]), (["--denoise-cross"], "--denoise-cross"),
                         (["--denoise-var"], "--denoise-var"), (["--denoise-select"], "--denoise-select")):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        assert r.returncode == 2, (extra, r.stdout, r.stderr)
        assert flag in r.stderr and named in r.stderr, (extra, r.stderr)
    # the flag implies the mode's -denoise flag and needs what that flag needs
    r = subprocess.run([EXE, flag], capture_output=True, text=True)
    assert r.returncode == 2 and flag.replace("-cross", "") in r.stderr, r.stderr


def test_the_stage_flags_need_a_cross_flag():
    for extra, named in ((["--plane-denoise-var"], "--plane-denoise-var"), (["--plane-resid-out", "r"], "--plane-resid-out")):
        for base in ([], ["--planes-out", "p", "--planes-denoise"], ["--denoise-cross"]):
            r = subprocess.run([EXE] + base + extra, capture_output=True, text=True)
            assert r.returncode == 2, (base, extra, r.stderr)
            assert named in r.stderr and "--planes-denoise-cross" in r.stderr, r.stderr
    assert subprocess.run([EXE, "--planes-out", "p", "--planes-denoise-cross", "--plane-resid-out"], capture_output=True, text=True).returncode == 2


def test_the_beauty_cross_filter_still_refuses_plane_flags():
    for bad in (["--denoise-cross", "--layers-out", "l"], ["--denoise-cross", "--over", "0", "0", "0"], ["--denoise-cross", "--groups-out", "g"],
                ["--denoise-cross", "--sun-gain", "1", "1", "1"], ["--denoise-cross", "--planes-out", "p"],
                ["--denoise-cross", "--groups-out", "g", "--groups-denoise"], ["--denoise-cross", "--layers-out", "l", "--layers-denoise"],
                ["--denoise-cross", "--planes-out", "p", "--planes-denoise"]):
        r = subprocess.run([EXE] + bad, capture_output=True, text=True)
        assert r.returncode == 2 and "--denoise-cross with " in r.stderr and "not a plane's" in r.stderr, (bad, r.stderr)
