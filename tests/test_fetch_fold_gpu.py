"""The density fetch with the box scale folded into the texel scale (csrc/vp_device.h fetch_scales, sample_density01).

1. Hook level (vp_test_fetch_split): the two-step and the folded split of one axis agree in every word -- cell index and weight of
   the uchar split; index, weight and `low` of the float split -- on the bit patterns of tests/fetch_fold_cases.py, for power-of-two
   box scales 2^-3 .. 2^3 and n = 4, 16, 256, 4096.  A scale of 2/3 is the control: there the forms do differ, so the hook sees it.
2. The scales the host chose for each scene (vp_test_fetch_form), against the precondition restated on linv's bits.  They are the
   launch arguments' values; the kernels that read them are the global-majorant integrator on uchar volumes and
   vp_test_sample_density -- for float and binary16 volumes and the decomposition estimator the image tests below pin unchanged
   bits of kernels that scale in two steps.
3. Image level: 32 x 24, 8 frames, Philox2x32-7, global majorant and decomposition: the accumulator equals the CPU oracle's
   (tolerance 0) for every scene of fetch_fold_cases.SCENES, and equals the render of a fresh process under VP_NO_FETCH_FOLD=1, which
   reports the two-step form for all of them.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import fetch_fold_cases as FC
import scenes

pytestmark = pytest.mark.gpu

f32, u32 = np.float32, np.uint32
VP_E_ARG = -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# -------------------------------------------------------------------------------------------------------------- hook level
@pytest.mark.parametrize("n", [4, 16, 256, 4096])
def test_folded_split_equals_the_two_step_split(vp, n):
    fixed = FC.fixed_patterns()
    for k in range(-3, 4):
        linv = f32(2.0) ** k
        assert vp.fetch_fold_axis(linv, n)
        s = np.concatenate([fixed, FC.grid_patterns(n, linv)])
        two, fold = vp.test_fetch_split(linv, n, s)
        bad = np.argwhere((two != fold).any(axis=1)).ravel()
        assert bad.size == 0, (n, k, len(bad), hex(int(s[bad[0]])), two[bad[0]].tolist(), fold[bad[0]].tolist())
        # what the patterns are there for: every cell, every weight, both sides of `low`, and the clamps
        assert set(np.unique(two[:, 0]).tolist()) == set(range(n)) and set(np.unique(two[:, 2]).tolist()) == set(range(n))
        w = np.unique(two[:, 1].view(f32))
        w = w[np.isfinite(w)]
        assert len(w) == 257 and w[0] == 0.0 and w[-1] == 1.0, (n, k, len(w))
        assert set(np.unique(two[:, 4]).tolist()) == {0, 1}


def test_the_hook_sees_a_scale_that_does_not_fold(vp):
    linv = f32(2.0) / f32(3.0)
    assert not vp.fetch_fold_axis(linv, 16)
    two, fold = vp.test_fetch_split(linv, 16, FC.grid_patterns(16, linv))
    assert (two != fold).any(), "two roundings and one agree everywhere on 2/3: the hook compares nothing"


def test_hook_refuses_bad_arguments(vp):
    import ctypes as C
    L = vp.lib()
    s, a, b = np.zeros(1, u32), np.zeros(5, u32), np.zeros(5, u32)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    assert L.vp_test_fetch_split(0.5, 16, -1, p(s), p(a), p(b)) == VP_E_ARG
    assert L.vp_test_fetch_split(0.5, 0, 1, p(s), p(a), p(b)) == VP_E_ARG
    assert L.vp_test_fetch_split(0.5, 4097, 1, p(s), p(a), p(b)) == VP_E_ARG
    assert L.vp_test_fetch_split(0.5, 16, 1, None, p(a), p(b)) == VP_E_ARG
    assert L.vp_test_fetch_split(0.5, 16, 1, p(s), None, p(b)) == VP_E_ARG
    assert L.vp_test_fetch_split(0.5, 16, 1, p(s), p(a), None) == VP_E_ARG
    assert L.vp_test_fetch_split(0.5, 16, 0, p(s), p(a), p(b)) == 0
    assert L.vp_test_fetch_form(None, p(a), p(b)) == VP_E_ARG


# ------------------------------------------------------------------------------------------------------------- image level
def _setup(vp, grid, box, linear, est):
    vp.set_subpixel(1)
    vp.init_volume(grid, box=box, brick=1, linear=linear)
    vp.init_envmap(scenes.synthetic_env())
    vp.set_sun(scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER)
    vp.set_camera()
    vp.set_estimator(est)
    vp.set_rng(vp.RNG_PHILOX7, FC.KEY)
    vp.set_tracking(0)
    vp.set_envmap_sampling(vp.ENV_PASSIVE)
    vp.set_shard(0, 1)
    vp.enable_counters(False)
    if est == vp.EST_DECOMP:
        vp.precompute_opacity(scenes.DEFAULT_SUN_DIR)
    return vp.make_param(FC.W, FC.H)


def _render(vp, grid, box, linear, est):
    P = _setup(vp, grid, box, linear, est)
    buf = vp.DeviceBuffer(FC.W, FC.H)
    try:
        vp.render_frames(buf.ptr, FC.FIRST, FC.NFRAMES, P)
        return buf.download()
    finally:
        buf.free()


_GRIDS, _ORACLE = {}, {}


def _grid(oracle, name):
    if name not in _GRIDS:
        g = FC.SCENES[name][0](oracle)
        g.setflags(write=False)
        _GRIDS[name] = g
    return _GRIDS[name]


def _oracle(oracle, name, est):
    """the oracle's accumulator: computed once per case, shared, never written to"""
    if (name, est) not in _ORACLE:
        _, box, linear, _, _ = FC.SCENES[name]
        osc = oracle.OracleScene(_grid(oracle, name), scenes.synthetic_env(), scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER, box=box, linear=linear,
                                 estimator=est, rng_mode=oracle.RNG_PHILOX7, seed=FC.KEY)
        if est == oracle.EST_DECOMP:
            osc.precompute_opacity()
        oP = oracle.default_param(FC.W, FC.H)
        acc, fetches = None, 0
        for f in range(FC.FIRST, FC.FIRST + FC.NFRAMES):
            acc, c = osc.render_frame(oP, f, acc)
            fetches += c.as_dict()["density_lookups"]
        assert fetches > 1000, ("the scene fetches too little to test the fetch", name, est, fetches)
        acc.setflags(write=False)
        _ORACLE[(name, est)] = acc
    return _ORACLE[(name, est)]


@pytest.mark.parametrize("name", list(FC.SCENES))
def test_the_form_the_context_chose(vp, oracle, name):
    _, box, linear, want_fold, want_axes = FC.SCENES[name]
    grid = _grid(oracle, name)
    _setup(vp, grid, box, linear, vp.EST_GLOBAL)
    fold, fscale, fmul = vp.fetch_form()
    linv, n = FC.linv_of(grid, box)
    # the table's expectation is the precondition on the bits of linv
    assert tuple(int(linear and FC.is_pow2(linv[a])) for a in range(3)) == want_axes, (name, linv.tolist())
    assert fold == want_fold == int(all(want_axes)), (name, fold)
    for a in range(3):
        if want_axes[a]:
            assert fmul[a] == 1.0 and fscale[a] == linv[a] * f32(n[a]), (name, a, fmul.tolist(), fscale.tolist())
        else:
            assert fmul[a].tobytes() == linv[a].tobytes() and fscale[a] == f32(n[a]), (name, a, fmul.tolist(), fscale.tolist())
    if name == "slab16x8x4":
        assert linv.tolist() == [0.5, 1.0, 2.0] and fscale.tolist() == [8.0, 8.0, 8.0]
    # the filter mode moves the form with it: point sampling of the same volume folds nothing, and back
    vp.lib().set_texture_filter_mode(not linear)
    other = vp.fetch_form()[0]
    vp.lib().set_texture_filter_mode(bool(linear))
    assert vp.fetch_form()[0] == want_fold
    assert other == (0 if linear else int(all(FC.is_pow2(v) for v in linv)))


@pytest.mark.parametrize("est", list(FC.ESTIMATORS))
@pytest.mark.parametrize("name", list(FC.SCENES))
def test_images_equal_the_oracle(vp, oracle, name, est):
    _, box, linear, _, _ = FC.SCENES[name]
    e = FC.ESTIMATORS[est]
    ref = _oracle(oracle, name, e)
    got = _render(vp, _grid(oracle, name), box, linear, e)
    assert got.tobytes() == ref.tobytes(), (name, est, int((got != ref).any(-1).sum()), float(np.abs(got - ref).max()))


CHILD = """import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import volpath as vp, oracle_lib as oracle, fetch_fold_cases as FC, test_fetch_fold_gpu as T
vp.set_device(0)
out = {}
for name, (build, box, linear, _, _) in FC.SCENES.items():
    grid = build(oracle)
    for est, e in FC.ESTIMATORS.items():
        out[name + "/" + est] = T._render(vp, grid, box, linear, e)
        out[name + "/" + est + "/fold"] = np.array(vp.fetch_form()[0])
np.savez(%r, **out)
"""


def test_images_equal_the_two_step_form_of_a_fresh_process(vp, oracle, tmp_path):
    out_file = str(tmp_path / "nofold.npz")
    code = CHILD % (os.path.join(ROOT, "cuda-volpath_amd"), os.path.join(ROOT, "tests"), out_file)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, VP_NO_FETCH_FOLD="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with np.load(out_file) as z:
        for name, (_, box, linear, _, _) in FC.SCENES.items():
            for est, e in FC.ESTIMATORS.items():
                assert int(z[name + "/" + est + "/fold"]) == 0, (name, est, "the knob left the folded form on")
                mine = _render(vp, _grid(oracle, name), box, linear, e)
                theirs = z[name + "/" + est]
                assert mine.tobytes() == theirs.tobytes(), (name, est, int((mine != theirs).any(-1).sum()))
