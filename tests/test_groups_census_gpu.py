"""Every compiled light-groups instance of render_k runs once and is held to the groups expectation.

csrc/vp_dispatch.h compiles a groups twin (render_k's GRP argument) of the 79 instances that have a layers twin and launches them
through a table of its own, counted by vp_test_groups_census.  The pattern is that of tests/test_instance_census_gpu.py's layers
test, whose volumes, media, contexts and plan rows are used as they are: per (estimator, stream) the rows `timed`, `segment table`
and `pairs, timed` -- a 24 x 16 image with 3 frames, and per decomposition group one launch of 64 frames on 6 x 4 pixels -- each
request held to the expectation of tests/groups_lib.py (the oracle's zero-environment and zero-sun twins) at tolerance 0; then the
census must show that every built instance of the group has run."""
import numpy as np
import pytest

import groups_lib as GL
import scenes
import test_instance_census_gpu as IC

pytestmark = pytest.mark.gpu

GROUPS_ROWS = IC.LAYERS_ROWS


class GroupsCensus:
    """the launches of the groups table, request by request (IC.Census for vp_test_groups_census)"""

    def __init__(self, vp):
        self.vp, self.total = vp, {}
        vp.groups_census(reset=True)

    def take(self, what, est, rng, vol):
        delta = {k: v for k, v in self.vp.groups_census(reset=True).items() if v}
        for k, v in delta.items():
            self.total[k] = self.total.get(k, 0) + v
        dt = IC.VOLUMES[vol].dtype
        want = dict(est=est, rng=rng, quant=int(dt == np.uint8), half=int(dt == np.float16), count=0, mis=0, trk=0)
        general = [k for k in delta if not IC._digits(k)["light"]]
        assert general, (what, "no general-class kernel ran", delta)
        for k in general:
            d = IC._digits(k)
            assert all(d[f] == v for f, v in want.items()), (what, "ran", k, "asked for", want)
        return delta

    def assert_all_ran(self, est, rng):
        built = self.vp.groups_census()
        must = {k for k in built if IC._digits(k)["est"] == est and IC._digits(k)["rng"] == rng}
        assert must, "the group has no kernel"
        missing = sorted(k for k in must if not self.total.get(k))
        assert not missing, (len(missing), "of", len(must), "built instances never ran:", missing)
        assert set(self.total) <= must, sorted(set(self.total) - must)


@pytest.mark.parametrize("est,rng", IC.EXACT_GROUPS, ids=IC._ids(IC.EXACT_GROUPS))
def test_every_groups_render_k_instance_runs_and_equals_the_expectation(vp, oracle, monkeypatch, est, rng):
    census = None
    layers_before = sum(vp.launch_census(vp.CENSUS_EXACT, vp.CENSUS_LAYERS).values())
    for cname, rows in IC._by_context(IC._rows(est, rng, GROUPS_ROWS)).items():
        c = IC._context(vp, monkeypatch, cname)
        try:
            with c:
                if census is None:
                    census = GroupsCensus(vp)
                for name, _, vols, media, _, _, _, call, _ in rows:
                    for vol in vols:
                        for med in media:
                            what = (name, cname, vol, med)
                            long = call == "long"
                            size, frames = (IC.LONG_SIZE, IC.LONG_FRAMES) if long else ((IC.W, IC.H), IC.FRAMES)

                            def make():
                                trio = GL.scenes_for(oracle, IC._wide(vol), IC.ENV, scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER, brick=IC._brick(est),
                                                     estimator=est, rng_mode=rng, seed=IC.KEY)
                                if long:
                                    for s in trio:
                                        s.precompute_opacity()
                                return trio + (oracle.default_param(size[0], size[1], **IC.MEDIA[med]), range(frames))
                            E = GL.expectation(oracle, ("census", vol, med, est, rng, long), make)
                            P = IC._scene(vp, vol, med, est, rng, opacity=long, size=size)
                            sun, sky = vp.DeviceBuffer(*size), vp.DeviceBuffer(*size)
                            try:
                                vp.render_frames_groups(sun.ptr, sky.ptr, 0, frames, P)
                                got = sun.download(), sky.download()
                            finally:
                                sun.free()
                                sky.free()
                            ran = census.take(what, est, rng, vol)
                            assert np.array_equal(got[0], E.sun, equal_nan=True), (what, sorted(ran), "sun", int((got[0] != E.sun).any(-1).sum()))
                            assert np.array_equal(got[1], E.sky, equal_nan=True), (what, sorted(ran), "sky", int((got[1] != E.sky).any(-1).sum()))
                            if not long:
                                assert E.scattered.any() and not E.scattered.all() and E.miss.any() and E.lit_sun.any() and E.lit_sky.any(), what
        finally:
            c.destroy()
    census.assert_all_ran(est, rng)
    # a groups launch goes through its own table only
    assert sum(vp.launch_census(vp.CENSUS_EXACT, vp.CENSUS_LAYERS).values()) == layers_before
