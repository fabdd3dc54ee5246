"""Extreme media (tests/extreme_media.py) on the CPU: the oracle against the reference's own kernel code, byte for byte, on every case
and all three estimators, accumulators after every frame; the reference-made fixture tests/golden/ref_media.npz
(tests/golden/make_golden.py: ref_media) where oracle/_ref is absent; a census that shows every case reaches the edge it is named
for; and the guard that lets a case into the table only if its work per sample stays within 100 times julia_default's.

The pattern (`_need`, `_same`, the live-comparison count) is that of tests/test_reference_kernel_cpu.py.
"""
import os

import numpy as np
import pytest

import extreme_media as EM
import ref_cases as RC
import ref_lib

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_media.npz")
COMPARISONS = []        # one entry per byte comparison of an oracle result with a reference result
VARIANT_TAGS = ("g_pm1", "dead", "amplifying")
VARIANT_CASES = [c["name"] for c in EM.CASES if set(c["tags"]) & set(VARIANT_TAGS)]
WORK_FACTOR = 100       # a case may do this many times julia_default's density lookups + draws per sample


def _need(variant=""):
    st = ref_lib.status(variant)
    if st == "absent":
        pytest.skip("neither oracle/_ref/libkernel_ref*.so nor the reference tree is here")
    assert st == "ok", f"the reference tree is here but {ref_lib.path(variant)} is not: `make -C oracle ref` failed or did not run"


def _same(what, got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    COMPARISONS.append(what)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        raise AssertionError(f"{what}: oracle differs from the reference in {len(bad)} of {got.size} elements, first at "
                             f"{tuple(bad[0])}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}")


def rc_case(c, variant="", kw=None):
    """the case in the form tests/ref_cases.py renders"""
    return RC._case(c["name"], grid=c["grid"], kw=c["kw"] if kw is None else kw, frames=c["frames"], size=c["size"], variant=variant)


JULIA_DEFAULT = dict(name="julia_default", kw={}, base={}, grid=EM.GRID, size=(EM.W, EM.H), frames=EM.FRAMES, tags=())


# ---------------------------------------------------------------------------------------------------------------- the oracle
_RUNS = {}


def _subnormal(oracle):
    return oracle.lib().vpo_debug_subnormal_throughput()


def _run(oracle, c, est, which="kw"):
    """the oracle on a case (`which`: its medium, or "base": its neighbour): the accumulator after every frame, the image of every
    frame on its own, the counters summed and the subnormal hook's count.  Computed once, shared, never written to."""
    k = (c["name"], est, which)
    if k not in _RUNS:
        sc = RC.oracle_scene(oracle, rc_case(c), est)
        if RC.needs_opacity(c, est):
            sc.precompute_opacity()
        P = oracle.default_param(c["size"][0], c["size"][1], **c[which])
        before = _subnormal(oracle)
        acc, each, single, cnt = None, [], [], None
        for f in c["frames"]:
            acc, n = sc.render_frame(P, f, acc)
            each.append(acc.copy())
            d = n.as_dict()
            cnt = d if cnt is None else {q: cnt[q] + d[q] for q in d}
        subnormal = _subnormal(oracle) - before
        for f in c["frames"]:
            single.append(sc.render_frame(P, f, None)[0])
        for a in each + single:
            a.setflags(write=False)
        assert oracle.lib().vpo_debug_shadow_overflow() == 0, c["name"]
        _RUNS[k] = dict(each=each, single=single, counters=cnt, subnormal=subnormal)
    return _RUNS[k]


def _work(r):
    return (r["counters"]["density_lookups"] + r["counters"]["rng_draws"]) / r["counters"]["samples"]


# ------------------------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("est", RC.ALL_EST, ids=[RC.EST_NAMES[e] for e in RC.ALL_EST])
@pytest.mark.parametrize("name", EM.NAMES)
def test_extreme_medium_equals_the_references_kernel(oracle, name, est):
    c = EM.BY_NAME[name]
    _need()
    want = RC.ReferenceBackend(ref_lib, oracle).render(rc_case(c), est, c["frames"], each=True)
    got = _run(oracle, c, est)["each"]
    for f, g, w in zip(c["frames"], got, want):
        _same(f"{name}/{RC.EST_NAMES[est]} after frame {f}", g, w)


@pytest.mark.parametrize("est", RC.ALL_EST, ids=[RC.EST_NAMES[e] for e in RC.ALL_EST])
@pytest.mark.parametrize("variant", ("_mis", "_scalar", "_multichannel"))
@pytest.mark.parametrize("name", VARIANT_CASES)
def test_extreme_medium_equals_the_references_other_builds(oracle, name, variant, est):
    """PASSIVE_ENVMAP 0, SPECTRAL_TRACKING 0 and MULTI_CHANNEL 1 on g = +-1, the dead channel and the amplifying medium"""
    _need(variant)
    c = rc_case(EM.BY_NAME[name], variant)
    want = RC.ReferenceBackend(ref_lib, oracle).render(c, est, c["frames"], each=True)
    got = RC.OracleBackend(oracle).render(c, est, c["frames"], each=True)
    for f, g, w in zip(c["frames"], got, want):
        _same(f"{name}{variant}/{RC.EST_NAMES[est]} after frame {f}", g, w)


@pytest.mark.parametrize("name", [c["name"] for c in EM.tagged("ach_compare")])
def test_nudged_medium_equals_the_references_kernel(oracle, name):
    """the chromatic neighbour of an equal-by-compare medium, one ulp away in one channel (the GPU tests run both instances)"""
    _need()
    c = rc_case(EM.nudged(EM.BY_NAME[name]))
    for est in RC.ALL_EST:
        _same(f"{c['name']}/{RC.EST_NAMES[est]}", RC.OracleBackend(oracle).render(c, est, c["frames"]),
              RC.ReferenceBackend(ref_lib, oracle).render(c, est, c["frames"]))


@pytest.mark.parametrize("name", EM.NAMES)
def test_the_edit_reaches_the_kernel(oracle, name):
    """the case's render differs from that of its neighbour -- the same scene in the case's ordinary base medium -- in some byte of some
    estimator: the Param edit is not lost on the way"""
    c = EM.BY_NAME[name]
    differs = [_run(oracle, c, est)["each"][-1].tobytes() != _run(oracle, c, est, "base")["each"][-1].tobytes() for est in RC.ALL_EST]
    assert any(differs), name
    if c["group"] != "g" or abs(c["kw"]["g"]) >= 1e-3:
        assert all(differs), (name, differs)


@pytest.mark.parametrize("frame", EM.NAN_CLAMP_FRAMES[0])
def test_nan_before_the_clamp_equals_the_references_kernel(oracle, frame):
    """g = 1 and a draw of exactly 0 for the scatter direction: cos(theta) is 0 / 0 before the reference's clamp (kernel.cu:590) makes
    it 1.  The frames were found by scanning with the oracle's counter; sampler.h stream, the only one the reference has."""
    _need()
    c = RC._case("nan_clamp", kw=dict(g=1.0), frames=(frame,), size=EM.NAN_CLAMP_SIZE)
    before = oracle.lib().vpo_debug_hg_nan_clamp()
    got = RC.OracleBackend(oracle).render(c, RC.EST_GLOBAL, c["frames"])
    assert oracle.lib().vpo_debug_hg_nan_clamp() > before, "this frame no longer clamps a NaN"
    _same(f"NaN before the clamp, frame {frame}", got, RC.ReferenceBackend(ref_lib, oracle).render(c, RC.EST_GLOBAL, c["frames"]))
    assert np.isfinite(got).all()


# ------------------------------------------------------------------------------------------------------------------- census
@pytest.mark.parametrize("est", RC.ALL_EST, ids=[RC.EST_NAMES[e] for e in RC.ALL_EST])
@pytest.mark.parametrize("name", [c["name"] for c in EM.CASES if c["group"] == "g"])
def test_g_cases_scatter(oracle, name, est):
    assert _run(oracle, EM.BY_NAME[name], est)["counters"]["scatters"] > 0


@pytest.mark.parametrize("est", RC.ALL_EST, ids=[RC.EST_NAMES[e] for e in RC.ALL_EST])
def test_dead_channel_is_what_the_unscattered_part_leaves(oracle, est):
    """albedo (1, 1, 0): a sample that scattered carries nothing in the third channel -- the sun's light at its first collision is
    already weighted with the zero albedo -- so a single-sample image is exactly 0 there wherever the heat channel says it scattered,
    and an accumulated pixel holds exactly the sum of its unscattered samples"""
    (c,) = EM.tagged("dead")
    r = _run(oracle, c, est)
    total = np.zeros(r["single"][0].shape[:2], np.float32)
    scattered = 0
    for one in r["single"]:
        if est == RC.EST_BOUNDED:       # its heat counts segments, not scatters: a sample that gathered sunlight and no blue
            hot = (one[..., 0] > 0) & (one[..., 2] == 0)
        else:
            hot = one[..., 3] > 0
            assert (one[..., 2][hot] == 0).all() and (one[..., :2][hot] > 0).any()
        scattered += int(hot.sum())
        total = total + np.where(hot, np.float32(0), one[..., 2])
    assert scattered > 20
    assert np.array_equal(r["each"][-1][..., 2], total)


def test_amplifying_medium_exceeds_1e3(oracle):
    (c,) = EM.tagged("amplifying")
    for est in RC.ALL_EST:
        acc = _run(oracle, c, est)["each"][-1]
        assert np.isfinite(acc).all() and acc[..., :3].max() > 1e3, (est, acc[..., :3].max())


def test_overflowing_medium_overflows(oracle):
    """albedo 6 without absorption: every sample sees the sky or gathers sunlight, so it is positive (the default medium has no black
    sample) unless its throughput overflowed -- then the collision weight is inf / inf and fmaxf(NaN, 0) writes 0.  Some samples
    end so, in every estimator, and others come within a factor 1e8 of the largest float"""
    (c,) = EM.tagged("overflow")
    black = lambda r: sum(int((one[..., :3] == 0).all(-1).sum()) for one in r["single"])
    for est in RC.ALL_EST:
        r = _run(oracle, c, est)
        print(f"\nalbedo_overflow/{RC.EST_NAMES[est]}: {black(r)} samples overflowed, largest value {r['each'][-1][..., :3].max():.3g}", end="")
        assert black(r) > 0 and black(_run(oracle, JULIA_DEFAULT, est)) == 0, est
        assert r["each"][-1][..., :3].max() > 1e30, est


def test_g_minus_one_reaches_the_scatter_cap(oracle):
    (c,) = EM.tagged("cap")
    r = _run(oracle, c, RC.EST_DECOMP)
    for one in r["single"]:         # heat = scatters: some sample of every frame ends at the cap (not the same pixel's in frames 10 and 11)
        assert one[..., 3].max() == 800.0
    assert r["each"][-1][..., 3].max() > 800.0


def test_subnormal_channel_is_subnormal_at_a_collision(oracle):
    (c,) = EM.tagged("subnormal")
    for est in RC.ALL_EST:
        r = _run(oracle, c, est)
        assert r["subnormal"] > 0, est
        assert np.isfinite(r["each"][-1]).all()
    assert _run(oracle, JULIA_DEFAULT, RC.EST_GLOBAL)["subnormal"] == 0


# -------------------------------------------------------------------------------------------------------- termination guard
@pytest.mark.parametrize("name", EM.NAMES)
def test_case_terminates_within_the_cap(oracle, name):
    """density lookups + draws per sample, per estimator, against julia_default in the same run: at most WORK_FACTOR times as many"""
    c = EM.BY_NAME[name]
    for est in RC.ALL_EST:
        work, cap = _work(_run(oracle, c, est)), WORK_FACTOR * _work(_run(oracle, JULIA_DEFAULT, est))
        print(f"\n{name}/{RC.EST_NAMES[est]}: {work:.4g} lookups + draws per sample (julia_default {cap / WORK_FACTOR:.4g})", end="")
        assert work <= cap, (name, est, work, cap)


# ------------------------------------------------------------------------------------------------------------------ fixture
def golden_estimators(i, c):
    """the estimators whose reference-made accumulators the fixture keeps: one per case in rotation, all three where the case is one
    of the named edges"""
    if set(c["tags"]) & {"g_pm1", "dead", "amplifying", "subnormal"}:
        return RC.ALL_EST
    return (RC.ALL_EST[i % 3],)


def entries(b):
    """(name, thunk) of every entry of tests/golden/ref_media.npz; a thunk computes its entry with backend `b` of tests/ref_cases.py"""
    out = []
    for i, c in enumerate(EM.CASES):
        for est in golden_estimators(i, c):
            out.append((f"render/{c['name']}/{RC.EST_NAMES[est]}", lambda c=c, est=est: b.render(rc_case(c), est, c["frames"])))
    return out


ENTRY_NAMES = [n for n, _ in entries(None)]
_ENTRIES = {}


def _entry(oracle, who, name):
    if (who, name) not in _ENTRIES:
        b = RC.OracleBackend(oracle) if who == "oracle" else RC.ReferenceBackend(ref_lib, oracle)
        a = np.ascontiguousarray(dict(entries(b))[name]())
        a.setflags(write=False)
        _ENTRIES[who, name] = a
    return _ENTRIES[who, name]


@pytest.fixture(scope="module")
def fixture():
    return dict(np.load(FIXTURE))


@pytest.mark.parametrize("name", ENTRY_NAMES)
def test_oracle_reproduces_the_reference_made_fixture(oracle, fixture, name):
    """tests/golden/ref_media.npz was computed BY THE REFERENCE LIBRARIES; this runs where oracle/_ref is absent, too."""
    assert RC.same(fixture, name, _entry(oracle, "oracle", name)), name


def test_fixture_has_exactly_the_named_entries(fixture):
    assert {k.split("#")[0] for k in fixture} == set(ENTRY_NAMES)
    assert os.path.getsize(FIXTURE) <= 200 * 1024


@pytest.mark.parametrize("name", ENTRY_NAMES)
def test_fixture_is_what_the_reference_makes(oracle, fixture, name):
    """the committed fixture is current: the libraries built from the reference tree reproduce it"""
    _need()
    COMPARISONS.append("fixture " + name)
    assert RC.same(fixture, name, _entry(oracle, "reference", name)), name


def test_zz_live_comparisons_report():
    """last in the file: how many byte comparisons with the reference's own code ran (shown with -s)"""
    for v in ref_lib.VARIANTS:
        _need(v)
    print(f"\nlive comparisons with the reference's own code on extreme media: {len(COMPARISONS)}")
