"""GPU suite: consecutive vp_render_frames calls on two alternating render targets (the pipeline, vp_render.cpp pipe_target).

The pipeline moves a call's integrator launches onto an internal stream so that they start in the tail of the call before; the
write into the caller's buffer stays on the caller's stream.  Bar: every sequence -- with camera, sun, estimator, counter and
render_kernel calls between the calls -- gives the same accumulator bit for bit with the pipeline on and off (tolerance 0), a call
that does not fit the second target takes the single-target path with the same bits, and the reported kernel time of overlapping
launches does not exceed the wall time they span."""
import hashlib
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import scenes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 160, 120
CAM2 = (0.96, 0.0, 0.28, 0.3, 0.0, 1.0, 0.0, 0.05, -0.28, 0.0, 0.96, -3.9)


def _scene(vp, est):
    vp.set_lookahead(0)
    vp.init_volume(vp.julia_volume(64), brick=4 if est == vp.EST_DECOMP else 1, linear=True)
    vp.init_envmap(scenes.synthetic_env())
    vp.set_sun(scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER)
    vp.set_camera()
    vp.set_estimator(est)
    vp.set_tracking(0)
    vp.set_shard(0, 1)
    vp.set_rng(vp.RNG_PHILOX7, (5, 9))
    if est == vp.EST_DECOMP:
        vp.precompute_opacity(scenes.DEFAULT_SUN_DIR)


def _run(vp, pipeline, calls, between=None):
    """calls: [(first, n)] into one accumulator; between(i) runs before call i > 0.  Returns the image and the pipelined flags."""
    vp.set_pipeline(pipeline)
    P = vp.make_param(W, H)
    buf = vp.DeviceBuffer(W, H)
    flags = []
    try:
        for i, (first, n) in enumerate(calls):
            if i and between:
                between(i)
            vp.render_frames(buf.ptr, first, n, P)
            flags.append(vp.last_pipelined())
        return buf.download(), flags
    finally:
        buf.free()
        vp.set_pipeline(True)


@pytest.mark.parametrize("est", ["global", "decomposition"])
def test_pipelined_calls_match_the_single_target(vp, est):
    e = vp.EST_GLOBAL if est == "global" else vp.EST_DECOMP
    _scene(vp, e)
    calls = [(0, 64), (64, 64), (128, 16), (144, 64), (208, 2)]
    on, f_on = _run(vp, True, calls)
    off, f_off = _run(vp, False, calls)
    assert f_on == [1] * len(calls) and f_off == [0] * len(calls)
    assert on.tobytes() == off.tobytes()
    assert np.isfinite(on).all() and on[..., :3].mean() > 0


def test_state_changes_between_pipelined_calls(vp):
    """A camera move, a new sun, an estimator switch, counters on and off and a render_kernel call between pipelined calls: each
    waits for the launches in flight, and the next call renders with what it was given."""
    _scene(vp, vp.EST_GLOBAL)
    vp.precompute_opacity(scenes.DEFAULT_SUN_DIR)
    P = vp.make_param(W, H)

    def between(i):
        if i == 1:
            vp.set_camera(CAM2)
        elif i == 2:
            vp.set_sun((0.3, 0.8, -0.52), (2.0, 1.8, 1.5))
        elif i == 3:
            vp.set_estimator(vp.EST_DECOMP)
        elif i == 4:
            vp.enable_counters(True)
        elif i == 5:
            vp.read_counters(reset=True)
            vp.enable_counters(False)
        elif i == 6:
            side = vp.DeviceBuffer(W, H)
            vp.set_lookahead(vp.LOOKAHEAD_DEFAULT)
            for f in range(3):
                vp.render_kernel(side.ptr, f, P)
            vp.synchronize()
            side.free()
            vp.set_lookahead(0)
            vp.set_estimator(vp.EST_GLOBAL)

    calls = [(0, 48), (48, 48), (96, 48), (144, 64), (208, 8), (216, 48), (264, 48), (312, 48)]
    results = []
    for pipeline in (True, False):
        _scene(vp, vp.EST_GLOBAL)
        vp.precompute_opacity(scenes.DEFAULT_SUN_DIR)
        results.append(_run(vp, pipeline, calls, between))
    (on, f_on), (off, f_off) = results
    assert f_on == [1, 1, 1, 1, 0, 1, 1, 1] and not any(f_off)   # (the counting call stays on the caller's stream)
    assert on.tobytes() == off.tobytes()


def test_host_read_right_after_a_pipelined_call(vp):
    """The caller's buffer is written on the caller's stream: a synchronisation of that stream after the call is enough to read it."""
    _scene(vp, vp.EST_GLOBAL)
    P = vp.make_param(W, H)
    got = []
    for pipeline in (True, False):
        vp.set_pipeline(pipeline)
        buf = vp.DeviceBuffer(W, H)
        vp.render_frames(buf.ptr, 0, 32, P)
        vp.render_frames(buf.ptr, 32, 32, P)
        assert vp.last_pipelined() == int(pipeline)
        vp.synchronize()
        out = np.empty((H, W, 4), np.float32)
        assert vp.lib().vp_download(out.ctypes.data, buf.ptr, out.nbytes) == 0
        got.append(out)
        buf.free()
    vp.set_pipeline(True)
    assert got[0].tobytes() == got[1].tobytes()


def test_memory_capped_call_falls_back_with_the_same_bits():
    """A call the second target cannot hold in one launch (VP_STAGE_MB: a cap below one call's staging) renders on the caller's
    stream in several launches, as before the pipeline: same bits, no error."""
    code = (
        "import sys, hashlib; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import volpath as vp, scenes\n"
        "vp.set_device(0); W, H = %d, %d\n"
        "vp.init_volume(vp.julia_volume(64), brick=1); vp.init_envmap(scenes.synthetic_env())\n"
        "vp.set_sun(scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER); vp.set_camera(); vp.set_estimator(vp.EST_GLOBAL)\n"
        "vp.set_rng(vp.RNG_PHILOX7, (5, 9)); P = vp.make_param(W, H); b = vp.DeviceBuffer(W, H); flags = []\n"
        "for first in (0, 128, 256):\n"
        "    vp.render_frames(b.ptr, first, 128, P); flags.append(vp.last_pipelined())\n"
        "print('HASH', hashlib.sha1(b.download().tobytes()).hexdigest(), *flags)\n"
    ) % (os.path.join(ROOT, "cuda-volpath_amd"), os.path.join(ROOT, "tests"), W, H)
    res = {}
    # (128 frames of 160x120 pixels stage 39 MB: a 16 MB cap splits every call into three launches)
    for name, env in (("default", {}), ("capped", {"VP_STAGE_MB": "16"}), ("off", {"VP_NO_PIPELINE": "1"})):
        e = dict(os.environ)
        e.update(env)
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=e, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        res[name] = [l for l in r.stdout.splitlines() if l.startswith("HASH")][0].split()[1:]
    assert res["default"][1:] == ["1", "1", "1"]
    assert res["capped"][1:] == ["0", "0", "0"] and res["off"][1:] == ["0", "0", "0"]
    assert res["default"][0] == res["capped"][0] == res["off"][0]


def test_reported_kernel_time_fits_the_wall_time(vp):
    """Overlapping launches are reported from where their predecessor ended: the sum of the launch times and each class's sum stay
    within the wall time of the region that ran them."""
    _scene(vp, vp.EST_GLOBAL)
    P = vp.make_param(W, H)
    buf = vp.DeviceBuffer(W, H)
    vp.reserve_frames(P, 128)
    vp.synchronize()
    vp.render_time_ms(reset=True)
    vp.render_class_time_ms(reset=True)
    t0 = time.perf_counter()
    for i in range(8):
        vp.render_frames(buf.ptr, 128 * i, 128, P)
        assert vp.last_pipelined() == 1
    vp.synchronize()
    wall_ms = (time.perf_counter() - t0) * 1e3
    total, launches = vp.render_time_ms(reset=True)
    cls, _ = vp.render_class_time_ms(reset=True)
    buf.free()
    assert launches == 8 and 0 < total <= wall_ms
    assert 0 < cls["general"] <= wall_ms and cls["misses_box"] <= wall_ms
