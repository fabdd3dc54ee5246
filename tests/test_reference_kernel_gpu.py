"""The HIP library against results made by the reference's OWN kernel code.

tests/golden/ref_kernel.npz holds accumulators and tables computed by the reference's kernel file and bound builder, compiled for
the CPU behind oracle/refshim (tests/golden/make_golden.py: ref_kernel).  The HIP library must reproduce
every entry as bytes: exact arithmetic, sampler.h stream, dense bound table (brick = 1) -- the reference has no other.  The other
GPU tests compare with the oracle; this one does not go through it.

Reads tests/golden/ only: neither the reference tree nor oracle/_ref.  The oracle module supplies inputs (the Julia voxels).
"""
import os

import numpy as np
import pytest

import ref_cases as RC
import scenes

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_kernel.npz")
# what the product has no read-back for: the pdf tables (read under MULT_PDF only, never uploaded) and the directional sun power
NO_READBACK = ("/pdf_y", "/pdf_x", "sun_power")
NAMES = [n for n in RC.ENTRY_NAMES if not n.endswith(NO_READBACK)]


@pytest.fixture(scope="module")
def fixture():
    return dict(np.load(FIXTURE))


class GpuBackend:
    """the entries of the fixture, computed by the HIP library through its C ABI"""

    def __init__(self, vp, oracle, per_frame):
        self.vp, self.O, self.per_frame = vp, oracle, per_frame

    def _scene(self, g, e="sky", box=None, linear=True, cam=None, sun=scenes.DEFAULT_SUN_DIR):
        vp = self.vp
        vp.set_arithmetic(vp.ARITH_EXACT)
        vp.set_subpixel(1)
        vp.init_volume(RC.grid(g, self.O), box=box, brick=1, linear=linear)
        vp.init_envmap(RC.env(e))
        vp.set_sun(sun, scenes.DEFAULT_SUN_POWER)
        vp.set_camera() if cam is None else vp.set_camera(cam)
        vp.set_rng(vp.RNG_SAMPLERH, (0, 0))
        vp.set_shard(0, 1)

    def render(self, c, est, frames):
        vp = self.vp
        buf = vp.DeviceBuffer(*c["size"])
        try:
            vp.set_tracking(RC.TRACK_OF_VARIANT[c["variant"]])
            vp.set_envmap_sampling(vp.ENV_MIS if c["variant"] == "_mis" else vp.ENV_PASSIVE)
            self._scene(c["grid"], c["env"], c["box"], c["linear"], c["cam"], c["sun"])
            vp.set_estimator(est)
            if RC.needs_opacity(c, est, frames):
                vp.precompute_opacity(c["sun"])
            P = RC.param(vp.make_param, vp.mat, c)
            if self.per_frame:          # the reference's call pattern (the Part-1 ABI), look-ahead on
                vp.set_lookahead(vp.LOOKAHEAD_DEFAULT)
                for f in frames:
                    vp.render_kernel(buf.ptr, f, P)
            else:
                for first, n in RC.runs(frames):
                    vp.render_frames(buf.ptr, first, n, P)
            assert vp.last_arithmetic() == vp.ARITH_EXACT
            return buf.download()
        finally:
            vp.set_tracking(vp.TRACK_SPECTRAL)
            vp.set_envmap_sampling(vp.ENV_PASSIVE)
            vp.set_camera()
            buf.free()

    def bounds(self, g):
        self._scene(g)
        tab, brick, radius = self.vp.bound_table(RC.grid(g, self.O).dtype == np.uint8)
        assert brick == 1
        return tab

    def opacity(self, g, light):
        self._scene(g)
        self.vp.precompute_opacity(RC.LIGHTS[light])
        return self.vp.opacity_table(RC.grid(g, self.O).shape)

    def env_tables(self, e):
        vp = self.vp
        try:
            vp.set_envmap_sampling(vp.ENV_MIS)
            self._scene("tiny", e)
            h, w = RC.env(e).shape[:2]
            cdf_y, cdf_x, norm = vp.env_tables(w, h)
            return dict(cdf_y=cdf_y, cdf_x=cdf_x, pdfnorm_alt=np.float32(norm))
        finally:
            vp.set_envmap_sampling(vp.ENV_PASSIVE)

    def _post(self, call):
        a = RC.post_inputs()
        src, dst = self.vp.DeviceBuffer(len(a), 1), self.vp.DeviceBuffer(len(a), 1)
        try:
            src.upload(a)
            call(dst.ptr, src.ptr, len(a))
            return dst.download().reshape(a.shape)
        finally:
            src.free()
            dst.free()

    def scale(self, a, s):
        return self._post(lambda d, p, n: self.vp.scale(d, p, n, s))

    def gamma_correct(self, a, s, gamma):
        return self._post(lambda d, p, n: self.vp.gamma_correct(d, p, n, s, gamma))


def _check(fixture, name, got):
    if not RC.same(fixture, name, got):
        detail = ""
        if name in fixture and fixture[name].shape == np.shape(got):
            bad = np.argwhere(np.asarray(got) != fixture[name])
            detail = f": {len(bad)} of {fixture[name].size} elements differ" + (f", first at {tuple(bad[0])}" if len(bad) else "")
        raise AssertionError(f"{name}: the HIP library does not reproduce the reference-made entry{detail}")


@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith("render/")])
def test_render_frames_reproduces_the_references_accumulator(vp, oracle, fixture, name):
    _check(fixture, name, dict(RC.entries(GpuBackend(vp, oracle, per_frame=False)))[name]())


@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith("render/")])
def test_render_kernel_reproduces_the_references_accumulator(vp, oracle, fixture, name):
    """one render_kernel call per frame, as the reference's host loop makes them, with the frame look-ahead on"""
    _check(fixture, name, dict(RC.entries(GpuBackend(vp, oracle, per_frame=True)))[name]())


@pytest.mark.parametrize("name", [n for n in NAMES if not n.startswith("render/")])
def test_table_reproduces_the_references(vp, oracle, fixture, name):
    """vp_get_bound_table, vp_get_opacity, vp_get_env_tables, scale, gamma_correct"""
    _check(fixture, name, dict(RC.entries(GpuBackend(vp, oracle, per_frame=False)))[name]())
