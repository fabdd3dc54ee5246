"""Compositing layers, light groups and their statistics on the GPU, randomised (include/volpath.h vp_render_frames_layers,
vp_render_frames_groups and their _stats forms; DESIGN.md sections 2.6 to 2.8): the seeded random scenes of tests/scenes.py --
ragged uchar, float and binary16 grids, user boxes, cameras outside, inside and looking away, both filters, bricks 1 to 8, the three
estimators and streams, late first frames, the frame-11 switch, shards, the exit-flight modes -- as tests/planes_fuzz_lib.py turns them
into cases, rendered by the plane calls and held against that helper's expectation, which comes from the CPU oracle alone.

Bar: tolerance 0.  Accumulators against the expectation with np.array_equal, records by their bits, and the library's several ways to
the same result by their bytes.  Per case and kind: one call; the _stats call; the job split into two calls; the shards of
`world` ranks; a vp_render_frames call and a second plane call afterwards; and, for the long cases rendered in a context that takes
no volume for dense, the approach walk and tables that the plain call reports for the same launch.  A case that the helper does not
admit is skipped with its reason (of the default lists: short seeds 7 and 25, a path each that ends with a NaN throughput).

VP_FUZZ_PLANES_SEEDS and VP_FUZZ_PLANES_LONG set the number of short and long seeds (defaults 32 and 8)."""
import os

import numpy as np
import pytest

import adaptive_lib as AL
import plane_stats_lib as PS
import planes_fuzz_lib as PF

pytestmark = pytest.mark.gpu

KINDS = ("layers", "groups")


class Planes:
    """the two accumulators and the two record buffers of a plane call of `kind`"""

    def __init__(self, vp, kind, w, h):
        self.acc = (vp.DeviceBuffer(w, h), vp.DeviceBuffer(w, h))
        self.rec = (vp.StatsBuffer(w, h), vp.StatsBuffer(w, h))
        self._stats = {"groups": vp.render_frames_groups_stats, "layers": vp.render_frames_layers_stats}[kind]
        self._plain = {"groups": vp.render_frames_groups, "layers": vp.render_frames_layers}[kind]

    def plain(self, first, n, P):
        self._plain(self.acc[0].ptr, self.acc[1].ptr, first, n, P)
        return self.acc[0].download(), self.acc[1].download()

    def stats(self, first, n, P):
        self._stats(self.acc[0].ptr, self.acc[1].ptr, self.rec[0].ptr, self.rec[1].ptr, first, n, P)
        return self.acc[0].download(), self.acc[1].download(), self.rec[0].download(), self.rec[1].download()

    def reset(self):
        for b in self.acc + self.rec:
            b.reset()

    def free(self):
        for b in self.acc + self.rec:
            b.free()


def _set_scene(vp, c):
    """as tests/test_fuzz_gpu.py sets it"""
    vp.init_volume(c["grid"], box=c["box"], brick=c["brick"], linear=c["linear"])
    assert vp.volume_info()["format"] == {"u8": vp.VOL_U8, "f32": vp.VOL_F32, "f16": vp.VOL_F16}[PF.volume_format(c)]
    vp.init_envmap(c["env"])
    vp.set_sun(c["sun_dir"], c["sun_power"])
    vp.set_camera(c["cam"])
    vp.set_estimator(c["est"])
    vp.set_rng(c["rng_mode"], c["key"])
    vp.set_tracking(vp.TRACK_SPECTRAL)
    vp.set_envmap_sampling(vp.ENV_PASSIVE)
    vp.set_shard(0, 1)
    vp.set_exit_flights(c["seed"] % 3)            # exit flights: off / global-majorant estimator (default) / local majorants too
    if c["late"]:
        vp.precompute_opacity(c["sun_dir"])


def split_frame(c):
    """how many frames the first of the two calls renders, from the seed.  A long case splits so that one call is a launch of fewer
    than 64 frames and the other one of at least 64 (which part comes first is drawn too); a case of exactly 64 frames has no such
    split and is cut where the draw says"""
    rng = np.random.default_rng(31000 + 2 * c["seed"] + c["long"])
    n = c["nframes"]
    if c["long"] and n > 64:
        k = int(rng.integers(1, n - 64 + 1))
        return k if rng.random() < 0.5 else n - k
    return int(rng.integers(1, n))


def _same_acc(got, want, what, step):
    for j in (0, 1):
        assert np.array_equal(got[j], want[j], equal_nan=True), (what, step, PF.PLANES[what["kind"]][j], "%d pixels" % int((got[j] != want[j]).any(-1).sum()),
                                                                 float(np.nanmax(np.abs(got[j] - want[j]))))


def _same_rec(got, want, what, step, flags=None):
    for j in (0, 1):
        bad = PS.same_records(want[j], got[j], flags)
        diff = max(float(np.nanmax(np.abs(got[j][k] - getattr(want[j], k)))) for k in ("sum_y", "sum_y2"))
        assert bad is None, (what, step, PF.PLANES[what["kind"]][j], bad, diff)


def _modes(vp):
    return dict(approach_mode=vp.last_approach_mode(), approach_table=vp.last_approach_table(), ray_table=vp.last_ray_table())


def _run(vp, oracle, monkeypatch, long, seed, kind):
    c, E = PF.expectation(oracle, long, seed)
    why = PF.admissible(E)
    if why is not None:
        pytest.skip("seed %d: the header's equivalent forms do not define this case: %s" % (seed, why))
    W, H, first, n, world = c["W"], c["H"], c["first"], c["nframes"], c["world"]
    what = dict(PF.what(c), kind=kind)
    want = tuple(E.acc(k) for k in PF.PLANES[kind])
    records = E.stats(kind)
    assert all(records[j].acc.tobytes() == want[j].tobytes() for j in (0, 1))
    never_dense = bool(long and seed & 1)         # small random grids mostly count as dense, and a dense volume gets no approach walk
    if never_dense:
        monkeypatch.setenv("VP_DENSE_PERCENT", "101")
    ctx = vp.Context(0)
    if never_dense:
        monkeypatch.delenv("VP_DENSE_PERCENT")
    ctx.__enter__()
    p, b = Planes(vp, kind, W, H), vp.DeviceBuffer(W, H)
    try:
        _set_scene(vp, c)
        P = vp.make_param(W, H, **c["kw"])
        err = vp.lib().vp_last_error()

        # 1. one call, from zero
        one = p.plain(first, n, P)
        plane_modes = _modes(vp)
        _same_acc(one, want, what, "one call")
        assert vp.lib().vp_last_error() == err, (what, vp.lib().vp_last_error())
        assert not p.rec[0].download()["n"].any() and not p.rec[1].download()["n"].any(), (what, "the plain call wrote records")

        # 2. the _stats call; flags hold a pattern and keep it
        board = np.zeros((H, W), vp.PIXEL_STATS_DTYPE)
        yy, xx = np.mgrid[0:H, 0:W]
        board["flags"] = (((xx + yy) % 2) * AL.FROZEN + (xx % 3 == 0) * 0x5a000000 + (seed << 8)).astype(np.uint32)
        p.reset()
        for r in p.rec:
            r.upload(board)
        got = p.stats(first, n, P)
        assert got[0].tobytes() == one[0].tobytes() and got[1].tobytes() == one[1].tobytes(), (what, "_stats: the accumulators of the plain call")
        _same_rec(got[2:], records, what, "_stats", flags=board["flags"])
        assert vp.lib().vp_last_error() == err, (what, vp.lib().vp_last_error())
        p.reset()
        whole = p.stats(first, n, P)              # ... and from zeroed records, for the bytes of steps 3 and 4

        # 3. the job in two calls: accumulators and records carry over
        if n > 1:
            k = split_frame(c)
            assert 0 < k < n and (not long or n == 64 or min(k, n - k) < 64 <= max(k, n - k))
            p.reset()
            part = p.stats(first, k, P)
            _same_acc(part, tuple(E.acc(q, 0, k) for q in PF.PLANES[kind]), what, "the first %d frames" % k)
            _same_rec(part[2:], E.stats(kind, 0, k), what, "the first %d frames" % k)
            got = p.stats(first + k, n - k, P)
            assert [a.tobytes() for a in got] == [a.tobytes() for a in whole], (what, "%d + %d frames" % (k, n - k))

        # 4. shards: `world` ranks into the same accumulators, each into records of its own
        if world > 1:
            p.reset()
            seen = np.zeros((H, W), int)
            sum_rec = [np.zeros((H, W), vp.PIXEL_STATS_DTYPE) for _ in (0, 1)]
            for r in range(world):
                vp.set_shard(r, world)
                owned = AL.owned_pixels(vp, W, H, r, world)
                for s in p.rec:
                    s.reset()
                got = p.stats(first, n, P)
                for j in (0, 1):
                    assert not np.frombuffer(got[2 + j][~owned].tobytes(), np.uint8).any(), (what, "rank %d of %d wrote records outside its tiles" % (r, world))
                    sum_rec[j][owned] = got[2 + j][owned]
                seen += owned
            vp.set_shard(0, 1)
            assert (seen == 1).all()
            assert got[0].tobytes() == one[0].tobytes() and got[1].tobytes() == one[1].tobytes(), (what, "the sum of %d shards" % world)
            assert [a.tobytes() for a in sum_rec] == [a.tobytes() for a in whole[2:]], (what, "the records of %d shards" % world)

        # 5. nothing left behind: the plain render is the oracle's, a second plane call is the first
        vp.render_frames(b.ptr, first, n, P)
        plain_modes = _modes(vp)
        beauty = E.acc("beauty")
        got = b.download()
        assert np.array_equal(got, beauty, equal_nan=True), (what, "vp_render_frames afterwards", float(np.nanmax(np.abs(got - beauty))))
        p.reset()
        again = p.plain(first, n, P)
        assert again[0].tobytes() == one[0].tobytes() and again[1].tobytes() == one[1].tobytes(), (what, "a second call")
        assert vp.lib().vp_last_error() == err, (what, vp.lib().vp_last_error())

        # 6. the same launch plan as the plain call: the walk and the tables it reads
        if never_dense:
            assert plane_modes == plain_modes == _modes(vp), (what, plane_modes, plain_modes, _modes(vp))
        if os.environ.get("VP_FUZZ_VERBOSE"):
            print("seed %d%s %s: est %d %s %s light const %d" % (seed, " long" if long else "", kind, c["est"], c["grid"].dtype, plane_modes, vp.last_light_const()))
    finally:
        vp.set_shard(0, 1)
        vp.set_exit_flights(1)
        vp.set_tracking(vp.TRACK_SPECTRAL)
        vp.set_envmap_sampling(vp.ENV_PASSIVE)
        vp.set_camera()
        p.free()
        b.free()
        ctx.__exit__(None, None, None)
        ctx.destroy()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("seed", range(int(os.environ.get("VP_FUZZ_PLANES_SEEDS", str(PF.SHORT_SEEDS)))))
def test_random_scene_planes_bit_exact(vp, oracle, monkeypatch, seed, kind):
    _run(vp, oracle, monkeypatch, False, seed, kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("seed", range(int(os.environ.get("VP_FUZZ_PLANES_LONG", str(PF.LONG_SEEDS)))))
def test_random_scene_long_launch_planes_bit_exact(vp, oracle, monkeypatch, seed, kind):
    """Launches of 64 frames and more: the approach walks hand their samples over, the decomposition estimator's walk reads the
    per-view segment table and the constants of the launch are staged once.  Odd seeds render in a context made under
    VP_DENSE_PERCENT=101, so that the walk runs in most of them; there the plane call must report the approach mode, the segment
    table and the ray table that vp_render_frames reports for the same scene and frame count."""
    _run(vp, oracle, monkeypatch, True, seed, kind)
