"""binary16 volumes (include/volpath.h vp_init_volume), the parts that need no GPU: the header's constants and
struct, the refusals that come before the device, float_to_half_rne against numpy's float32 -> float16 conversion (equality on the
16-bit patterns), the loader with a format, and the command line's --volume-format."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cuda-volpath_amd", "volpath_render")
E_STATE, E_ARG = -2, -3


@pytest.fixture(scope="module")
def host():
    from volpath import host as h
    h.lib()
    return h


def _half_bits(host, values):
    return host.float_to_half(np.asarray(values, np.float32)).view(np.uint16)


def _numpy_bits(values):
    with np.errstate(over="ignore"):
        return np.asarray(values, np.float32).astype(np.float16).view(np.uint16)


def test_header_constants_and_struct_layout():
    import volpath
    text = open(os.path.join(ROOT, "include", "volpath.h")).read()
    assert re.search(r"enum\s*\{\s*VP_VOL_U8\s*=\s*0\s*,\s*VP_VOL_F32\s*=\s*1\s*,\s*VP_VOL_F16\s*=\s*2\s*\}", text)
    assert (volpath.VOL_U8, volpath.VOL_F32, volpath.VOL_F16) == (0, 1, 2)
    assert re.search(r"typedef struct \{ int format; int nx, ny, nz; int cell_bytes; uint64_t cells_bytes; \} vp_volume_info;", text)
    for n in ("vp_init_volume", "vp_get_volume_info"):
        assert n in volpath.PART2_SYMBOLS and re.search(r"\bint\s+%s\s*\(" % n, text) and hasattr(volpath.lib(), n)
    V = volpath.VolumeInfo
    assert [(f, getattr(V, f).offset) for f, _ in V._fields_] == [("format", 0), ("nx", 4), ("ny", 8), ("nz", 12), ("cell_bytes", 16),
                                                                  ("cells_bytes", 24)]
    assert C.sizeof(V) == 32
    from volpath import host
    assert (host.VOL_U8, host.VOL_F32, host.VOL_F16) == (0, 1, 2)
    # init_cuda keeps its signature
    assert re.search(r"void init_cuda\(void\* h_volume, vp_extent volumeSize, bool quantized, const vp_float3\* boxmin,\s*const vp_float3\* boxmax\);", text)


def test_refusals_come_before_the_device():
    """NULL volume, unknown format, empty extent: VP_E_ARG; vp_get_volume_info without a volume: VP_E_STATE.  No device is asked for
    (this passes on a machine without one) and the volume pointer is never followed."""
    import volpath
    L = volpath.lib()
    vol = C.c_void_p(0x1000)   # never dereferenced
    ext = volpath.Extent(4, 4, 4)
    assert L.vp_init_volume(None, ext, volpath.VOL_F16, None, None) == E_ARG
    assert "null volume" in L.vp_last_error().decode()
    for fmt in (3, -1, 255):
        assert L.vp_init_volume(vol, ext, fmt, None, None) == E_ARG, fmt
    assert "format" in L.vp_last_error().decode()
    for e in ((0, 4, 4), (4, 0, 4), (4, 4, 0)):
        for fmt in (volpath.VOL_U8, volpath.VOL_F32, volpath.VOL_F16):
            assert L.vp_init_volume(vol, volpath.Extent(*e), fmt, None, None) == E_ARG, (e, fmt)
    assert "extent" in L.vp_last_error().decode()
    info = volpath.VolumeInfo()
    assert L.vp_get_volume_info(C.byref(info)) == E_STATE
    assert L.vp_get_volume_info(None) == E_ARG
    with pytest.raises(volpath.VolpathError):
        volpath.volume_info()


def test_float_to_half_every_half_pattern_round_trips(host):
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    wide = bits.view(np.float16).astype(np.float32)          # exact, subnormals and infinities included
    got = _half_bits(host, wide)
    nan = np.isnan(wide)
    assert np.array_equal(got[~nan], bits[~nan])
    assert np.all(np.isnan(got[nan].view(np.float16)))       # NaN stays NaN (which one is not part of the contract)


def test_float_to_half_rounding_ties_and_their_neighbours(host):
    """between every pair of adjacent halves (the step from 65504 to 2^16, where the overflow begins, included): the tie itself --
    which goes to the even pattern -- and the float on either side of it"""
    bits = np.arange(0x7c00, dtype=np.uint32).astype(np.uint16)              # +0 ... 65504
    lo = bits.view(np.float16).astype(np.float64)
    hi = np.append(lo[1:], 65536.0)
    tie = ((lo + hi) / 2).astype(np.float32)                                 # exact: 12 significant bits
    assert np.array_equal(tie.astype(np.float64), (lo + hi) / 2)
    below, above = np.nextafter(tie, np.float32(-np.inf)), np.nextafter(tie, np.float32(np.inf))
    for sign in (1.0, -1.0):
        for v in (tie, below, above):
            v = (v * np.float32(sign)).astype(np.float32)
            assert np.array_equal(_half_bits(host, v), _numpy_bits(v))
    # the ties themselves go to the even neighbour
    t = _half_bits(host, tie)
    assert np.all((t & 1) == 0) and t[-1] == 0x7c00


def test_float_to_half_subnormals_zeros_and_overflow(host):
    # the subnormal range of binary16 and below it, densely: 2^-24 is the smallest subnormal, 2^-25 (a tie) and less go to zero
    sub = np.linspace(0.0, 6.2e-5, 20001).astype(np.float32)
    tiny = (np.float32(2.0) ** np.arange(-40, -13, dtype=np.float32)).astype(np.float32)
    rnd = np.random.default_rng(5).uniform(0.0, 6.2e-5, 20000).astype(np.float32)
    for v in (sub, -sub, tiny, -tiny, np.nextafter(tiny, np.float32(1)), np.nextafter(tiny, np.float32(0)), rnd):
        assert np.array_equal(_half_bits(host, v), _numpy_bits(v))
    assert _half_bits(host, [2.0 ** -24])[0] == 0x0001 and _half_bits(host, [2.0 ** -25])[0] == 0x0000
    assert _half_bits(host, [np.nextafter(np.float32(2.0 ** -25), np.float32(1))])[0] == 0x0001      # produced, not flushed
    assert _half_bits(host, [3e-5])[0] == _numpy_bits([3e-5])[0] != 0
    assert list(_half_bits(host, [0.0, -0.0])) == [0x0000, 0x8000]
    assert list(_half_bits(host, [65504.0, -65504.0])) == [0x7bff, 0xfbff]
    assert list(_half_bits(host, [65520.0, -65520.0])) == [0x7c00, 0xfc00]                            # the first value that overflows
    assert _half_bits(host, [np.nextafter(np.float32(65520.0), np.float32(0))])[0] == 0x7bff
    assert list(_half_bits(host, [1e30, -1e30, np.inf, -np.inf])) == [0x7c00, 0xfc00, 0x7c00, 0xfc00]
    # and two million random bit patterns
    r = np.random.default_rng(6).integers(0, 2 ** 32, 2_000_000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    r = r[~np.isnan(r)]
    assert np.array_equal(_half_bits(host, r), _numpy_bits(r))


def test_loader_with_a_format(host, tmp_path):
    rng = np.random.default_rng(2)
    vol = (rng.random((3, 4, 5), dtype=np.float32) * 1.4 - 0.2).astype(np.float32)
    vol[0, 0, :4] = (0.0, 3e-5, 65504.0, 1e-8)
    p = str(tmp_path / "v.bin")
    assert host.dump_dense(p, vol)
    h = host.load_binary_as(p, host.VOL_F16)
    assert h.dtype == np.float16 and h.shape == (3, 4, 5)
    assert np.array_equal(h.view(np.uint16), vol.astype(np.float16).view(np.uint16))
    # the two forms the loader had: the same arrays as loadBinaryFile's
    assert np.array_equal(host.load_binary_as(p, host.VOL_F32), host.load_binary(p, quantized=False))
    assert np.array_equal(host.load_binary_as(p, host.VOL_U8), host.load_binary(p, quantized=True))
    assert host.lib().vph_load_binary_as(p.encode(), *(C.byref(C.c_int()) for _ in range(3)), 7) is None      # unknown format
    assert host.load_binary_as(str(tmp_path / "missing.bin"), host.VOL_F16) is None
    open(str(tmp_path / "cut.bin"), "wb").write(open(p, "rb").read()[:-6])
    assert host.load_binary_as(str(tmp_path / "cut.bin"), host.VOL_F16) is None
    assert host.load_vdb_as(str(tmp_path / "missing.vdb"), host.VOL_F16) is None
    assert struct.unpack("<iii", open(p, "rb").read()[:12]) == (5, 4, 3)


def test_cli_volume_format_flag(tmp_path):
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--volume-format u8|f32|f16" in r.stdout
    # an unknown value and a missing one: usage, exit code 2
    for bad in (["--volume-format", "f64"], ["--volume-format", "F16"], ["--volume-format"]):
        r = subprocess.run([EXE, "--bin", "x.bin"] + bad, capture_output=True, text=True)
        assert r.returncode == 2, (bad, r.stdout, r.stderr)
    # --julia voxelises to bytes: any other format is refused with a message, before anything is loaded or rendered
    for fmt in ("f16", "f32"):
        for args in (["--volume-format", fmt], ["--julia", "16", "--volume-format", fmt], ["--volume-format", fmt, "--julia", "16"]):
            r = subprocess.run([EXE] + args, capture_output=True, text=True)
            assert r.returncode == 2 and "--volume-format" in r.stderr and "--julia" in r.stderr, (args, r.stderr)
    # accepted with --bin: parsing goes through, the run ends where the file (or, without a GPU, the device) is missing -- not in usage
    for fmt in ("u8", "f32", "f16"):
        r = subprocess.run([EXE, "--bin", str(tmp_path / "missing.bin"), "--volume-format", fmt, "--size", "8", "8", "--spp", "1"],
                           capture_output=True, text=True)
        assert r.returncode == 1 and "volpath_render [" not in r.stdout, (fmt, r.returncode, r.stderr)
