"""Sub-pixel sampling (include/volpath.h vp_set_subpixel / vp_subpixel_offset) without a GPU: the offset function against an
independent restatement, its stratification property, argument checks, the CLI flag, the constants."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cuda-volpath_amd", "volpath_render")
FACTORS = (1, 2, 4, 8)
# include/volpath.h: the sequence of S = 4 for k = (frame + h) mod 16 = 0 .. 15
S4_SEQUENCE = [(0, 0), (0, 2), (2, 0), (2, 2), (0, 1), (0, 3), (2, 1), (2, 3), (1, 0), (1, 2), (3, 0), (3, 2), (1, 1), (1, 3), (3, 1), (3, 3)]


def wang_hash(seed):
    """sampler.h:3-11 on numpy uint32 arrays"""
    seed = np.atleast_1d(np.asarray(seed, np.uint32))   # (arrays wrap silently; numpy warns about scalars)
    seed = (seed ^ np.uint32(61)) ^ (seed >> np.uint32(16))
    seed = seed * np.uint32(9)
    seed = seed ^ (seed >> np.uint32(4))
    seed = seed * np.uint32(0x27d4eb2d)
    seed = seed ^ (seed >> np.uint32(15))
    return seed


def offsets_of_k(k, s):
    """the definition's last three lines: reverse the 2m bits of k, de-interleave"""
    m = s.bit_length() - 1
    k = np.asarray(k, np.uint32)
    r = np.zeros_like(k)
    for b in range(2 * m):
        r |= ((k >> np.uint32(b)) & np.uint32(1)) << np.uint32(2 * m - 1 - b)
    i = np.zeros_like(k)
    j = np.zeros_like(k)
    for b in range(m):
        i |= ((r >> np.uint32(2 * b)) & np.uint32(1)) << np.uint32(b)
        j |= ((r >> np.uint32(2 * b + 1)) & np.uint32(1)) << np.uint32(b)
    return i.astype(np.int64), j.astype(np.int64)


def reference_offsets(x, y, f, s):
    """the five lines of the definition in numpy (uint32 wrap-around arithmetic)"""
    x = np.asarray(x, np.uint32); y = np.asarray(y, np.uint32); f = np.asarray(f, np.int64).astype(np.uint32)
    with np.errstate(over="ignore"):
        h = wang_hash(((x << np.uint32(16)) | y) ^ np.uint32(0x9E3779B9))
        k = (f + h) % np.uint32(s * s)
    return offsets_of_k(k, s)


def library_offsets(volpath, x, y, f, s):
    out = [volpath.subpixel_offset(int(a), int(b), int(c), s) for a, b, c in zip(x, y, f)]
    return np.array([o[0] for o in out], np.int64), np.array([o[1] for o in out], np.int64)


@pytest.mark.parametrize("s", FACTORS)
def test_offset_equals_the_definition(s):
    import volpath
    rng = np.random.default_rng(1234 + s)
    n = 4000
    x = rng.integers(0, 65536, n); y = rng.integers(0, 65536, n)
    f = rng.integers(0, 2 ** 31, n)
    f[:64] = 2 ** 31 - 1 - np.arange(64)      # frames near the top of the int range
    f[64:96] = np.arange(32)
    x[96:104] = [0, 65535, 0, 65535, 1, 2, 799, 599]; y[96:104] = [0, 0, 65535, 65535, 2, 1, 599, 799]
    gi, gj = library_offsets(volpath, x, y, f, s)
    ri, rj = reference_offsets(x, y, f, s)
    assert np.array_equal(gi, ri) and np.array_equal(gj, rj)
    assert gi.min() >= 0 and gi.max() < s and gj.min() >= 0 and gj.max() < s
    if s == 1:
        assert not gi.any() and not gj.any()


def test_s4_sequence_literal():
    import volpath
    ki, kj = offsets_of_k(np.arange(16), 4)
    assert list(zip(ki.tolist(), kj.tolist())) == S4_SEQUENCE
    # the library walks the same sequence, started at the pixel's hash
    for (x, y) in [(0, 0), (17, 3), (799, 599), (65535, 65535)]:
        h = int(wang_hash(((x << 16) | y) ^ 0x9E3779B9)[0])
        for f in list(range(40)) + [2 ** 31 - 1, 2 ** 31 - 17]:
            assert volpath.subpixel_offset(x, y, f, 4) == S4_SEQUENCE[(f + h) % 16]


@pytest.mark.parametrize("s", (2, 4, 8))
def test_stratification_of_consecutive_frames(s):
    """every window of 4^t consecutive frames, t <= m, hits each of the 2^t x 2^t sub-squares of the pixel exactly once"""
    import volpath
    m = s.bit_length() - 1
    rng = np.random.default_rng(99 + s)
    npix = 300
    xs = rng.integers(0, 4096, npix); ys = rng.integers(0, 4096, npix)
    starts = rng.integers(0, 2 ** 31 - 4 * s * s, npix)
    starts[:4] = [0, 1, 2 ** 31 - 1 - 2 * s * s, 5]
    for x, y, f0 in zip(xs, ys, starts):
        nf = 2 * s * s   # every start phase of every window size
        seq = [volpath.subpixel_offset(int(x), int(y), int(f0) + f, s) for f in range(nf)]
        for t in range(m + 1):
            win, cell = 4 ** t, s >> t
            for a in range(nf - win + 1):
                squares = {(i // cell, j // cell) for i, j in seq[a:a + win]}
                assert len(squares) == win, (s, t, x, y, f0, a)


def test_identity_and_refusals_before_the_device():
    import volpath
    L = volpath.lib()
    assert volpath.subpixel_offset(123, 45, 6789, 1) == (0, 0)
    for bad in (0, 3, 16, -1):
        assert L.vp_set_subpixel(bad) == -3   # VP_E_ARG
        assert "sub-pixel" in L.vp_last_error().decode()
        with pytest.raises(volpath.VolpathError, match="sub-pixel"):
            volpath.set_subpixel(bad)
        assert L.vp_subpixel_offset(1, 2, 3, bad, None, None) == -3
        with pytest.raises(volpath.VolpathError, match="sub-pixel"):
            volpath.subpixel_offset(1, 2, 3, bad)
    # coordinates that do not fit x << 16 | y, a negative frame
    assert L.vp_subpixel_offset(65536, 0, 0, 2, None, None) == -3
    assert L.vp_subpixel_offset(0, 65536, 0, 2, None, None) == -3
    assert L.vp_subpixel_offset(0, 0, -1, 2, None, None) == -3
    assert L.vp_subpixel_offset(5, 6, 7, 4, None, None) == 0   # null outputs are allowed
    # the setter itself needs no device either; the default is 1 (VP_SUBPIXEL unset in the test environment)
    if "VP_SUBPIXEL" not in os.environ:
        assert volpath.get_subpixel() == 1
    before = volpath.get_subpixel()
    try:
        for s in FACTORS:
            volpath.set_subpixel(s)
            assert volpath.get_subpixel() == s
    finally:
        volpath.set_subpixel(before)


def test_environment_default_of_new_contexts():
    """VP_SUBPIXEL=<s> sets the factor a context starts with; a malformed value is ignored"""
    code = "import sys; sys.path.insert(0, %r); import volpath; print(volpath.get_subpixel())" % os.path.join(ROOT, "cuda-volpath_amd")
    for val, want in (("4", "4"), ("8", "8"), ("1", "1"), ("3", "1"), ("bogus", "1")):
        env = dict(os.environ, VP_SUBPIXEL=val)
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stderr
        assert r.stdout.strip() == want, (val, r.stdout, r.stderr)


def test_cli_aa_flag():
    r = subprocess.run([EXE, "--aa", "3"], capture_output=True, text=True)
    assert r.returncode == 2
    assert "--aa" in r.stdout and "--aa" in r.stderr
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--aa 1|2|4|8" in r.stdout
    r = subprocess.run([EXE, "--aa"], capture_output=True, text=True)   # the value is missing
    assert r.returncode == 2


def test_constants_and_symbols_match_header():
    import volpath
    text = open(os.path.join(ROOT, "include", "volpath.h")).read()
    m = re.search(r"#define\s+VP_SUBPIXEL_MAX\s+(\d+)", text)
    assert m and int(m.group(1)) == volpath.SUBPIXEL_MAX == 8
    names = {"vp_set_subpixel", "vp_get_subpixel", "vp_subpixel_offset"}
    assert names <= set(volpath.PART2_SYMBOLS)
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, text), n
        assert hasattr(volpath.lib(), n)
