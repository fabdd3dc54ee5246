"""The launch census (include/volpath.h vp_test_launch_census) and the probe agree on which kernels exist.

tests/golden/render_variants.txt tabulates, through the launcher of csrc/vp_dispatch.h and host stand-ins, which render_k instance and
which approach kernel every admitted request SELECTS.  The census reports, from the shipped library, which table entries hold a
kernel: render_built(), planes_built() and approach_built() evaluated at run time in each translation unit.  The two sets must be
the same set of names: a kernel compiled but never selectable fails here, and so does one selectable but not compiled.  No GPU:
the `built` half of the census is host arithmetic."""
import numpy as np
import pytest

from test_render_variants_cpu import GOLDEN, _selected


def _names(rows, kinds):
    return _selected(rows[:-1], kinds)


def _digits(name):
    """render_k's template arguments from a fixture name EST RNG . QUANT COUNT LDSB ACH MIS . TRK LIGHT CANCEL HALF"""
    a, b, c = name.split(".")
    keys = ("est", "rng", "quant", "count", "ldsb", "ach", "mis", "trk", "light", "cancel", "half")
    return dict(zip(keys, (int(ch) for ch in a + b + c)))


def test_table_lengths_and_argument_checks():
    import volpath as vp
    L = vp.lib()
    for unit in (vp.CENSUS_EXACT, vp.CENSUS_FAST):
        assert L.vp_test_launch_census(unit, vp.CENSUS_RENDER, None, None, 0, 0) == 10368
        assert L.vp_test_launch_census(unit, vp.CENSUS_LAYERS, None, None, 0, 0) == 10368
        assert L.vp_test_launch_census(unit, vp.CENSUS_APPROACH, None, None, 0, 0) == 18
    a, b = np.zeros(18, np.uint32), np.zeros(18, np.uint8)
    p = lambda x: x.ctypes.data
    assert L.vp_test_launch_census(2, 0, None, None, 0, 0) == -3          # VP_E_ARG
    assert L.vp_test_launch_census(0, 3, None, None, 0, 0) == -3
    assert L.vp_test_launch_census(0, 2, p(a), p(b), 17, 0) == -3
    assert b"vp_test_launch_census" in L.vp_last_error()
    assert L.vp_test_launch_census(0, 2, p(a), None, 18, 0) == 0 and L.vp_test_launch_census(0, 2, None, p(b), 18, 0) == 0
    with pytest.raises(vp.VolpathError):
        vp.launch_census(0, 5)


def test_names_follow_render_index():
    """census_name inverts the mixed radix of render_index() / approach_index() that include/volpath.h documents"""
    import volpath as vp
    radix = dict(est=3, rng=3, quant=2, count=2, ldsb=3, ach=2, mis=2, trk=3, light=2, cancel=2, half=2)
    seen = set()
    for i in (0, 1, 2, 7, 95, 4321, 10367):
        name = vp.census_name(vp.CENSUS_RENDER, i)
        d, j = _digits(name), 0
        for k, r in radix.items():
            assert 0 <= d[k] < r
            j = j * r + d[k]
        assert j == i
        seen.add(name)
    assert len(seen) == 7
    assert [vp.census_name(vp.CENSUS_APPROACH, i) for i in range(18)] == [
        "g0", "g0", "g1", "g1", "g2", "g2", "l00", "l01", "l10", "l11", "l20", "l21", "t0", "t0", "t1", "t1", "t2", "t2"]


def test_built_sets_equal_what_the_fixture_selects():
    import volpath as vp
    exact = vp.launch_census(vp.CENSUS_EXACT, vp.CENSUS_RENDER)
    fast = vp.launch_census(vp.CENSUS_FAST, vp.CENSUS_RENDER)
    assert set(exact) == _names(GOLDEN["exact full"], {"render", "light"}) and len(exact) == 322
    assert {n for n in exact if _digits(n)["light"]} == _names(GOLDEN["exact full"], {"light"}) and sum(_digits(n)["light"] for n in exact) == 30
    assert set(fast) == _names(GOLDEN["fast full"], {"render"}) and len(fast) == 60
    ea = vp.launch_census(vp.CENSUS_EXACT, vp.CENSUS_APPROACH)
    fa = vp.launch_census(vp.CENSUS_FAST, vp.CENSUS_APPROACH)
    assert set(ea) == _names(GOLDEN["exact full"], {"approach"}) and len(ea) == 12
    assert set(fa) == _names(GOLDEN["fast full"], {"approach"}) and len(fa) == 8


def test_layers_set_is_the_exact_set_without_trk_mis_count_cancel():
    import volpath as vp
    exact = vp.launch_census(vp.CENSUS_EXACT, vp.CENSUS_RENDER)
    layers = vp.launch_census(vp.CENSUS_EXACT, vp.CENSUS_LAYERS)
    want = {n for n in exact if not any(_digits(n)[k] for k in ("trk", "mis", "count", "cancel"))}
    assert set(layers) == want and len(layers) == 79
    assert vp.launch_census(vp.CENSUS_FAST, vp.CENSUS_LAYERS) == {}         # the layers kernels are the exact unit's
