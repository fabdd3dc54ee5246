"""The host's predicate for the folded fetch scale (csrc/vp_device.h fetch_scale_folds through vp_test_fetch_fold_axis), no GPU, and
the identity the fold rests on, in numpy: for a power-of-two box scale fl(fl(s * linv) * n - 0.5) = fl(s * (linv * n) - 0.5)."""
import numpy as np
import pytest

import fetch_fold_cases as FC

f32, u32 = np.float32, np.uint32


def _f(bits):
    return float(np.array([bits], u32).view(f32)[0])


CASES = [
    ("half", 0.5, 16, True),
    ("quarter", 0.25, 16, True),
    ("one", 1.0, 4096, True),
    ("two_thirds", float(f32(2.0) / f32(3.0)), 16, False),
    ("half_plus_ulp", _f(0x3F000001), 16, False),
    ("half_minus_ulp", _f(0x3EFFFFFF), 16, False),
    ("smallest_normal", _f(0x00800000), 16, True),
    ("subnormal_power_of_two", _f(0x00400000), 16, False),
    ("smallest_subnormal", _f(0x00000001), 16, False),
    ("zero", 0.0, 16, False),
    ("minus_half", -0.5, 16, False),
    ("inf", float("inf"), 16, False),
    ("nan", float("nan"), 16, False),
    ("largest_power", _f(0x7F000000), 1, True),
    ("product_overflows", _f(0x7F000000), 4, False),
    ("no_texels", 0.5, 0, False),
    ("too_many_texels", 0.5, 4097, False),
]


@pytest.mark.parametrize("name,linv,n,want", CASES, ids=[c[0] for c in CASES])
def test_host_predicate(name, linv, n, want):
    import volpath
    assert volpath.fetch_fold_axis(linv, n) is want
    with np.errstate(over="ignore"):
        in_range = bool(np.isfinite(linv) and 1 <= n <= 4096 and np.isfinite(f32(linv) * f32(n)))
    if in_range:
        assert FC.is_pow2(linv) is want


def _fma(a, b, c):
    """fl(a * b + c) for binary32 operands: the product of two 24-bit significands and the sum are exact in float64 wherever the
    exponents lie within its 53 bits of each other, which the operands below keep; one rounding to binary32"""
    return (a.astype(np.float64) * np.float64(b) + np.float64(c)).astype(f32)


@pytest.mark.parametrize("n", [4, 16, 256, 4096])
def test_one_rounding_equals_two_for_a_power_of_two(n):
    for k in range(-3, 4):
        linv = f32(2.0) ** k
        s = FC.grid_patterns(n, linv).view(f32)
        two = _fma((s * linv).astype(f32), f32(n), -0.5)
        one = _fma(s, linv * f32(n), -0.5)
        assert two.tobytes() == one.tobytes(), (n, k)
    linv = f32(2.0) / f32(3.0)
    s = FC.grid_patterns(n, linv).view(f32)
    assert _fma((s * linv).astype(f32), f32(n), -0.5).tobytes() != _fma(s, linv * f32(n), -0.5).tobytes(), "the control: 2/3 rounds twice"


def test_scene_table_matches_the_precondition():
    """the forms the GPU test expects of each scene follow from linv's bits alone"""
    class _O:   # grids of the right shapes without the oracle: the table's builders only slice and cast
        @staticmethod
        def julia(n): return np.zeros((n, n, n), np.uint8)
        @staticmethod
        def cloud(n): return np.zeros((n, n, n), f32)
    for name, (build, box, linear, fold, axes) in FC.SCENES.items():
        linv, n = FC.linv_of(build(_O), box)
        assert tuple(int(linear and FC.is_pow2(v)) for v in linv) == axes, (name, linv.tolist())
        assert fold == int(all(axes))
