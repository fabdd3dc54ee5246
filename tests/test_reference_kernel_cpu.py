"""The oracle against the reference's OWN kernel code.

oracle/vp_oracle.c is a restatement of the reference integrator, and every GPU test ends in "bit-identical to the oracle".  Here
the restatement is held against what it restates: the reference's kernel file and bound builder, compiled for the CPU behind
oracle/refshim (oracle/Makefile, target `ref`; tests/ref_lib.py), on the sampler.h stream.  Everything is compared as bytes:
whole accumulators after every frame, whole tables.  What the comparison rests on beside the reference's text are the two
definitions of oracle/refshim: the texture fetch rule and the elementary functions.

Where the reference tree is present the libraries must be too (a missing one FAILS); where neither is, the live comparisons skip
and the reference-made fixture tests/golden/ref_kernel.npz (tests/golden/make_golden.py: ref_kernel) still holds the oracle.
"""
import os

import numpy as np
import pytest

import ref_cases as RC
import ref_lib
import scenes

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_kernel.npz")
COMPARISONS = []        # one entry per byte comparison of an oracle result with a reference result


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
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: oracle differs from the reference in {len(bad)} of {got.size} elements, first at "
                             f"{tuple(bad[0]) if len(bad) else '(bit pattern only)'}: "
                             f"{got[tuple(bad[0])] if len(bad) else ''} vs {want[tuple(bad[0])] if len(bad) else ''}")


@pytest.fixture(scope="module")
def fixture():
    return dict(np.load(FIXTURE))


_ENTRIES = {}


def _entry(oracle, who, name):
    """an entry of the fixture as the oracle or the reference computes it: computed once, shared, never written to"""
    if (who, name) not in _ENTRIES:
        b = RC.OracleBackend(oracle) if who == "oracle" else RC.ReferenceBackend(ref_lib, oracle)
        a = np.ascontiguousarray(dict(RC.entries(b))[name]())
        a.setflags(write=False)
        _ENTRIES[who, name] = a
    return _ENTRIES[who, name]


# ------------------------------------------------------------------------------------------------------------------ renders
@pytest.mark.parametrize("est", RC.ALL_EST, ids=[RC.EST_NAMES[e] for e in RC.ALL_EST])
@pytest.mark.parametrize("name", [c["name"] for c in RC.RENDERS + RC.VARIANT_RENDERS])
def test_render_equals_the_references_kernel(oracle, name, est):
    c = RC.BY_NAME[name]
    _need(c["variant"])
    want = RC.ReferenceBackend(ref_lib, oracle).render(c, est, c["frames"], each=True)
    got = RC.OracleBackend(oracle).render(c, est, c["frames"], each=True)
    for f, g, w in zip(c["frames"], got, want):
        _same(f"{name}/{RC.EST_NAMES[est]} after frame {f}", g, w)
    if name == "caps":      # the case is what its name says: max_depth = 800 segments (heat 0.8) or scatters (heat 800)
        assert want[-1][..., 3].max() == (800.0 if est == RC.EST_DECOMP else np.float32(0.8))
    if name == "multichannel":
        assert ((want[-1][..., :3] > 0).sum(-1) <= len(c["frames"])).all() and (want[-1][..., 1:3] > 0).any()


@pytest.mark.parametrize("seed", range(16))
def test_random_scene_equals_the_references_kernel(oracle, seed):
    """scenes.random_case -- random volume, box, camera, medium, estimator, filter, image size, first frame, build -- forced to the
    sampler.h stream and the dense bound table, which are all the reference has."""
    from volpath import host
    c = scenes.random_case(seed, host)
    variant = "_mis" if c["env_mis"] else {0: "", 1: "_scalar", 2: "_multichannel"}[c["track"]]
    _need(variant)
    osc = oracle.OracleScene(c["grid"], c["env"], c["sun_dir"], c["sun_power"], box=c["box"], brick=1, linear=c["linear"],
                             estimator=c["est"], rng_mode=oracle.RNG_SAMPLERH, inv_view=c["cam"], env_mis=c["env_mis"],
                             track_mode=c["track"])
    rsc = ref_lib.RefScene(c["grid"], c["env"], c["sun_dir"], c["sun_power"], box=c["box"], linear=c["linear"], inv_view=c["cam"],
                           variant=variant)
    if c["late"]:
        osc.precompute_opacity()
        _same(f"random {seed}: opacity", osc.opacity, rsc.precompute_opacity())
    _same(f"random {seed}: bounds", osc.bounds, rsc.bounds())
    P = oracle.default_param(c["W"], c["H"], **c["kw"])
    got = want = None
    for f in range(c["first"], c["first"] + c["nframes"]):
        got, _ = osc.render_frame(P, f, got)
        want = rsc.render_frame(c["est"], P, f, want)
    _same(f"random {seed}: est {c['est']} {variant or 'shipped'} frames {c['first']}+{c['nframes']}", got, want)


@pytest.mark.parametrize("est,frame", RC.MIS_ZERO_PDF)
def test_mis_zero_pdf_continue_equals_the_references_kernel(oracle, est, frame):
    """kernel.cu:1540 / :1900 / :2266: an environment sample of zero pdf `continue`s the path loop from the OLD origin in the OLD
    direction.  It takes a draw of exactly 0 on a black first column; the frames were found by scanning with the oracle's counter."""
    _need("_mis")
    c = dict(RC.BY_NAME["mis_black_column"], size=(64, 48))
    before = oracle.lib().vpo_debug_mis_zero_pdf()
    got = RC.OracleBackend(oracle).render(c, est, (frame,))
    assert oracle.lib().vpo_debug_mis_zero_pdf() > before, "this frame no longer takes the zero-pdf branch"
    _same(f"zero-pdf continue, est {est} frame {frame}", got, RC.ReferenceBackend(ref_lib, oracle).render(c, est, (frame,)))


# ------------------------------------------------------------------------------------------------------------------- tables
@pytest.mark.parametrize("name", [n for n in RC.ENTRY_NAMES if not n.startswith("render/")])
def test_table_equals_the_references(oracle, name):
    _need("_mis" if name.startswith("env/") else "")
    want, got = _entry(oracle, "reference", name), _entry(oracle, "oracle", name)
    _same(name, got, want)
    if name.startswith("opacity/"):
        assert want.max() > 0
    if name.startswith("bounds/"):
        assert (want[..., 0] >= want[..., 1]).all() and (want[..., 0] > want[..., 1]).any()


def test_light_directions_leave_through_all_six_faces():
    """the three directions of the optical-depth tables, from the centres of the voxels of either grid"""
    for shape in ((32, 32, 32), (9, 14, 120)):
        nz, ny, nx = shape
        half = np.array([1.0, ny / nx, nz / nx])
        k, j, i = np.mgrid[0:nz, 0:ny, 0:nx]
        p = (np.stack([(i + 0.5) / nx, (j + 0.5) / ny, (k + 0.5) / nz], -1) * 2 - 1) * half
        faces = set()
        for d in RC.LIGHTS.values():
            d = np.array(d, np.float64)
            with np.errstate(divide="ignore"):
                t = np.where(d > 0, (half - p) / d, np.where(d < 0, (-half - p) / d, np.inf))
            axis = t.argmin(-1)
            faces |= {(int(a), int(np.sign(d[a]))) for a in np.unique(axis)}
        assert len(faces) == 6, (shape, faces)


# -------------------------------------------------------------------------------------------------------------- sensitivity
def test_reference_tells_the_restatement_from_its_misreadings(oracle):
    """The comparison can fail: on the soft chromatic volume the reference equals the oracle as restated, and differs from it under
    each of the oracle's what-if switches -- quirk Q1 (cos theta clamped to [-1, 1]), Q4, Q7 and Q8 read differently."""
    _need()
    c = RC.BY_NAME["soft_u8_chromatic"]
    frames = (0, 1, 2, 3)
    want = RC.ReferenceBackend(ref_lib, oracle).render(c, RC.EST_DECOMP, frames)

    def render(what_if):
        oracle.lib().vpo_debug_set_what_if(what_if)
        try:
            return RC.OracleBackend(oracle).render(c, RC.EST_DECOMP, frames)
        finally:
            oracle.lib().vpo_debug_set_what_if(0)

    _same("soft chromatic volume as restated", render(0), want)
    for bit in (2, 4, 8, 16):
        assert render(bit).tobytes() != want.tobytes(), f"what-if {bit} is invisible to the reference's own code"


# ------------------------------------------------------------------------------------------------------------------ fixture
@pytest.mark.parametrize("name", RC.ENTRY_NAMES)
def test_oracle_reproduces_the_reference_made_fixture(oracle, fixture, name):
    """tests/golden/ref_kernel.npz was computed BY THE REFERENCE LIBRARIES; this runs where oracle/_ref is absent, too."""
    assert RC.same(fixture, name, _entry(oracle, "oracle", name)), name


def test_fixture_has_exactly_the_named_entries(fixture):
    assert {k.split("#")[0] for k in fixture} == set(RC.ENTRY_NAMES)
    assert os.path.getsize(FIXTURE) <= 200 * 1024


@pytest.mark.parametrize("name", RC.ENTRY_NAMES)
def test_fixture_is_what_the_reference_makes(oracle, fixture, name):
    """the committed fixture is current: the libraries built from the reference tree reproduce it"""
    _need("_mis" if name.startswith("env/") else RC.BY_NAME[name.split("/")[1]]["variant"] if name.startswith("render/") else "")
    COMPARISONS.append("fixture " + name)
    assert RC.same(fixture, name, _entry(oracle, "reference", name)), name


def test_zz_live_comparisons_report():
    """last in the file: how many byte comparisons with the reference's own code ran (shown with -s)"""
    for v in ref_lib.VARIANTS:
        _need(v)
    print(f"\nlive comparisons with the reference's own code: {len(COMPARISONS)}")
