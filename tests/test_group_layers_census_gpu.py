"""Every compiled group-layers instance of render_k runs once and is held to the group-layers expectation.

csrc/vp_dispatch.h compiles a twin with both LYR and GRP of the 79 instances that have a layers twin and launches them through a third
table, counted by vp_test_group_layers_census.  The pattern is tests/test_groups_census_gpu.py's, with the volumes, media, contexts and
plan rows of tests/test_instance_census_gpu.py as they are; each request is held to the expectation of tests/group_layers_lib.py at
tolerance 0, then the census must show that every built instance of the group has run -- and that neither the layers table nor the
groups table counted a launch."""
import numpy as np
import pytest

import group_layers_lib as GLL
import scenes
import test_instance_census_gpu as IC

pytestmark = pytest.mark.gpu

ROWS = IC.LAYERS_ROWS


class Census:
    """the launches of the group-layers table, request by request (IC.Census for vp_test_group_layers_census)"""

    def __init__(self, vp):
        self.vp, self.total = vp, {}
        vp.group_layers_census(reset=True)

    def take(self, what, est, rng, vol):
        delta = {k: v for k, v in self.vp.group_layers_census(reset=True).items() if v}
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
        built = self.vp.group_layers_census()
        must = {k for k in built if IC._digits(k)["est"] == est and IC._digits(k)["rng"] == rng}
        assert must, "the group has no kernel"
        missing = sorted(k for k in must if not self.total.get(k))
        assert not missing, (len(missing), "of", len(must), "built instances never ran:", missing)
        assert set(self.total) <= must, sorted(set(self.total) - must)


@pytest.mark.parametrize("est,rng", IC.EXACT_GROUPS, ids=IC._ids(IC.EXACT_GROUPS))
def test_every_group_layers_render_k_instance_runs_and_equals_the_expectation(vp, oracle, monkeypatch, est, rng):
    census = None
    others = lambda: (sum(vp.launch_census(vp.CENSUS_EXACT, vp.CENSUS_LAYERS).values()), sum(vp.groups_census().values()))
    before = others()
    for cname, rows in IC._by_context(IC._rows(est, rng, ROWS)).items():
        c = IC._context(vp, monkeypatch, cname)
        try:
            with c:
                if census is None:
                    census = Census(vp)
                for name, _, vols, media, _, _, _, call, _ in rows:
                    for vol in vols:
                        for med in media:
                            what = (name, cname, vol, med)
                            long = call == "long"
                            size, frames = (IC.LONG_SIZE, IC.LONG_FRAMES) if long else ((IC.W, IC.H), IC.FRAMES)

                            def make():
                                four = GLL.scenes_for(oracle, IC._wide(vol), IC.ENV, scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER, opacity=long,
                                                      brick=IC._brick(est), estimator=est, rng_mode=rng, seed=IC.KEY)
                                return four + (oracle.default_param(size[0], size[1], **IC.MEDIA[med]), range(frames))
                            E = GLL.expectation(oracle, ("census", vol, med, est, rng, long), make)
                            want = E.accs()
                            P = IC._scene(vp, vol, med, est, rng, opacity=long, size=size)
                            bufs = [vp.DeviceBuffer(*size) for _ in GLL.PLANES]
                            try:
                                vp.render_frames_group_layers(*[b.ptr for b in bufs], 0, frames, P)
                                got = [b.download() for b in bufs]
                            finally:
                                for b in bufs:
                                    b.free()
                            ran = census.take(what, est, rng, vol)
                            for k, plane in enumerate(GLL.PLANES):
                                assert np.array_equal(got[k], want[k], equal_nan=True), (what, sorted(ran), plane, int((got[k] != want[k]).any(-1).sum()))
                            if not long:
                                assert E.unscattered.any() and not E.unscattered.all() and E.miss.any() and all(a[..., :3].max() > 0 for a in want), what
        finally:
            c.destroy()
    census.assert_all_ran(est, rng)
    # a group-layers launch goes through its own table only
    assert others() == before
