"""Every compiled render_k and approach kernel runs once and is held to its reference.

csrc/vp_dispatch.h compiles 322 render_k kernels into the exact translation unit, a layers twin of 79 of them, 60 into the fast
arithmetic's unit, and 12 + 8 approach kernels.  The launch census (include/volpath.h vp_test_launch_census) counts, per table entry,
how often each has been launched.  A group here is one (unit, kind, estimator, stream): it resets the census, runs the requests of
PLAN -- each held to its reference --, and then asserts FROM THE CENSUS that every built instance of the group has run.  The plan
is data; which instances it must reach is not derived from it.

Shapes: the smallest at which each mechanism exists.  A 16^3 blob with empty margins as uchar, float and binary16, and its binary
(0 / 255) version, whose brick table has three distinct pairs and so goes through LDS as 2-bit codes; bricks of 4 for the
local-majorant estimators; a 24 x 16 image from the default camera, which has general, light and box-missing pixels (asserted);
frames 0..2 in one staged launch, before the decomposition estimator's frame-11 switch; and per decomposition group one launch of
64 frames on 6 x 4 pixels, where the approach walk reads the per-view segment table.  An achromatic and a chromatic medium.

Contexts (the knobs are read when a context is made).  All of them: VP_DENSE_PERCENT=101 (the walks run whatever the grid's fill),
VP_NO_LIGHT_CONST=1 (the light class runs its kernel instead of being written as constants), VP_LDS_COMPACT_CHROMATIC=1.  `pairs`
adds VP_LDS_PAIRS=1 (timed launches read the 16-bit brick table through LDS: LDSB 1 without COUNT or CANCEL), `nolds` adds
VP_NO_LDS_BOUNDS=1 (counting and look-ahead launches of the decomposition estimator on a uchar volume read it from global memory:
LDSB 0 with COUNT or CANCEL -- vp_render.cpp brick_table_form).

Bars.  Exact unit: np.array_equal with the oracle's render of the same request (a binary16 volume: of the widened floats), and equal
work counters for counting launches.  Layers: the expectation of tests/layers_lib.py, bit for bit.  Fast unit: no tolerance of its
own -- one-frame launches (the base instance of each format and medium) against the exact mode by check 2 and check 3 of
tests/test_fuzz_fast_gpu.py, and every other way to the same samples (staged with the walk, look-ahead, the other LDS forms) against
the sum of those one-frame launches at tolerance 0.  After every request the census delta must name general-class instances whose
EST, RNG, QUANT, HALF, COUNT, MIS and TRK are the request's.

Measured on an MI355X: the slowest case takes 1.40 s (the fast unit's decomposition groups: 6 scenes x 64 paired one-frame renders
in both modes), the exact groups at most 0.36 s, the layers groups at most 0.29 s; all 22 cases 10.8 s.  Before this test the rest
of the GPU suite had launched 249 of the 322 exact render_k kernels, 17 of the 79 layers kernels, 42 of the 60 fast ones and 7 of
the 8 fast approach kernels (one run of it with the census read at its end)."""
import numpy as np
import pytest

import layers_lib as LL
import scenes
from test_fuzz_fast_gpu import PAIRED_FRAMES, assert_paired_agreement

pytestmark = pytest.mark.gpu

W, H, FRAMES = 24, 16, 3
LONG_SIZE, LONG_FRAMES = (6, 4), 64
N = 16
KEY = (11, 22)
ENV = scenes.synthetic_env()
COUNTERS = ("samples", "density_lookups", "bound_lookups", "opacity_lookups", "env_lookups", "scatters")

_BLOB = scenes.blob_volume_f32(N)
VOLUMES = {
    "u8": np.ascontiguousarray((_BLOB * 255.0).astype(np.uint8)),
    "f32": np.ascontiguousarray(_BLOB),
    "f16": np.ascontiguousarray(_BLOB.astype(np.float16)),
    "bin": np.ascontiguousarray((_BLOB > 0).astype(np.uint8) * np.uint8(255)),
}
MEDIA = {
    "ach": dict(density=300.0, g=0.877),
    "chr": dict(density=300.0, g=0.877, sigma_t=(1.0, 0.8, 0.55), albedo=(0.9, 0.8, 0.95)),     # ACH = 0
}
BASE = {"VP_DENSE_PERCENT": "101", "VP_NO_LIGHT_CONST": "1", "VP_LDS_COMPACT_CHROMATIC": "1"}
CONTEXTS = {"base": BASE, "pairs": dict(BASE, VP_LDS_PAIRS="1"), "nolds": dict(BASE, VP_NO_LDS_BOUNDS="1")}

ALL, DENSITY = ("u8", "f32", "f16", "bin"), ("u8", "f32", "f16")
BOTH = ("ach", "chr")
# (row, context, volumes, media, count, mis, trk, call, estimators)
#   call: frames = one staged launch of FRAMES frames; kernel = frame-by-frame render_kernel calls with the look-ahead on (the
#   batches are the CANCEL instances); long = one launch of LONG_FRAMES frames on LONG_SIZE with the optical-depth table
PLAN = [
    ("timed",                 "base",  ALL,     BOTH,     0, 0, 0, "frames", (0, 1, 2)),
    ("counting",              "base",  ALL,     BOTH,     1, 0, 0, "frames", (0, 1, 2)),
    ("look-ahead",            "base",  ALL,     BOTH,     0, 0, 0, "kernel", (0, 1, 2)),
    ("MIS",                   "base",  DENSITY, BOTH,     0, 1, 0, "frames", (0, 1, 2)),
    ("MIS, counting",         "base",  DENSITY, BOTH,     1, 1, 0, "frames", (0, 1, 2)),
    ("scalar tracking",       "base",  DENSITY, ("chr",), 0, 0, 1, "frames", (0, 1, 2)),
    ("multi-channel",         "base",  DENSITY, ("chr",), 0, 0, 2, "frames", (0, 1, 2)),
    ("segment table",         "base",  ("u8",), ("ach",), 0, 0, 0, "long",   (1,)),
    ("pairs, timed",          "pairs", ("u8",), BOTH,     0, 0, 0, "frames", (1,)),
    ("global memory, counting",    "nolds", ("u8",), BOTH,     1, 0, 0, "frames", (1,)),
    ("global memory, look-ahead",  "nolds", ("u8", "bin"), BOTH, 0, 0, 0, "kernel", (1,)),
]
# what a layers call and the fast arithmetic admit of it (vp_render.cpp): no counters, no MIS, spectral tracking; layers: no look-ahead
LAYERS_ROWS = ("timed", "segment table", "pairs, timed")
FAST_ROWS = ("timed", "look-ahead", "segment table", "pairs, timed", "global memory, look-ahead")

# Built instances that no state of the library can launch: each with the proof, from vp_render.cpp, beside it.  Empty: none known.
UNREACHED = set()

EXACT_GROUPS = [(e, r) for e in (0, 1, 2) for r in (0, 1, 2)]
FAST_GROUPS = [(e, r) for e in (0, 1) for r in (1, 2)]
_ids = lambda gs: ["est%d-rng%d" % g for g in gs]


def _digits(name):
    a, b, c = name.split(".")
    keys = ("est", "rng", "quant", "count", "ldsb", "ach", "mis", "trk", "light", "cancel", "half")
    return dict(zip(keys, (int(ch) for ch in a + b + c)))


def _rows(est, rng, names=None):
    for row in PLAN:
        name, _, _, _, _, mis, trk, _, ests = row
        if est not in ests or (names is not None and name not in names):
            continue
        if rng == 2 and (mis or trk):          # VP_RNG_PHILOX7 is built for spectral tracking with the passive environment
            continue
        yield row


class Census:
    """the launches of one unit and kind, request by request"""

    def __init__(self, vp, unit, kind):
        self.vp, self.unit, self.kind, self.total = vp, unit, kind, {}
        vp.launch_census(unit, kind, reset=True)
        vp.launch_census(unit, vp.CENSUS_APPROACH, reset=True)

    def take(self, what, est, rng, vol, count=0, mis=0, trk=0):
        """what ran since the last call; it must be the request's instances"""
        delta = {k: v for k, v in self.vp.launch_census(self.unit, self.kind, reset=True).items() if v}
        for k, v in delta.items():
            self.total[k] = self.total.get(k, 0) + v
        dt = VOLUMES[vol].dtype
        want = dict(est=est, rng=rng, quant=int(dt == np.uint8), half=int(dt == np.float16), count=count, mis=mis, trk=trk)
        general = [k for k in delta if not _digits(k)["light"]]
        assert general, (what, "no general-class kernel ran", delta)
        for k in general:
            d = _digits(k)
            assert all(d[f] == v for f, v in want.items()), (what, "ran", k, "asked for", want)
        return delta

    def assert_all_ran(self, est, rng, walks):
        built = self.vp.launch_census(self.unit, self.kind)
        must = {k for k in built if _digits(k)["est"] == est and _digits(k)["rng"] == rng} - UNREACHED
        assert must, "the group has no kernel"
        missing = sorted(k for k in must if not self.total.get(k))
        assert not missing, (len(missing), "of", len(must), "built instances never ran:", missing)
        assert set(self.total) <= must | UNREACHED, sorted(set(self.total) - must)
        ran = self.vp.launch_census(self.unit, self.vp.CENSUS_APPROACH)
        assert set(walks) <= set(ran), (walks, sorted(ran))
        idle = sorted(k for k in walks if not ran[k])
        assert not idle, ("approach kernels that never ran:", idle, ran)
        return len(must)


def _context(vp, monkeypatch, name):
    for k, v in CONTEXTS[name].items():
        monkeypatch.setenv(k, v)
    c = vp.Context(0)
    for k in CONTEXTS[name]:
        monkeypatch.delenv(k)
    return c


def _brick(est):
    return 1 if est == 0 else 4


def _scene(vp, vol, med, est, rng, mis=0, trk=0, opacity=False, size=(W, H)):
    g = VOLUMES[vol]
    vp.init_volume(g, brick=_brick(est), linear=True)
    assert vp.volume_info()["format"] == {np.dtype(np.uint8): vp.VOL_U8, np.dtype(np.float32): vp.VOL_F32, np.dtype(np.float16): vp.VOL_F16}[g.dtype]
    vp.init_envmap(ENV)
    vp.set_sun(scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER)
    vp.set_camera()
    vp.set_estimator(est)
    vp.set_rng(rng, KEY)
    vp.set_tracking(trk)
    vp.set_envmap_sampling(vp.ENV_MIS if mis else vp.ENV_PASSIVE)
    vp.set_shard(0, 1)
    if opacity:
        vp.precompute_opacity(scenes.DEFAULT_SUN_DIR)
    P = vp.make_param(size[0], size[1], **MEDIA[med])
    if size == (W, H) and not trk:          # (scalar and multi-channel tracking have no pixel classes: every pixel runs the integrator)
        general, light, miss = vp.pixel_lists(P)
        assert len(general) and len(light) and len(miss), (vol, len(general), len(light), len(miss))   # else the light kernels are skipped silently
    return P


def _reset_modes(vp):
    vp.enable_counters(False)
    vp.set_lookahead(vp.LOOKAHEAD_DEFAULT)
    vp.set_tracking(vp.TRACK_SPECTRAL)
    vp.set_envmap_sampling(vp.ENV_PASSIVE)
    vp.set_arithmetic(vp.ARITH_EXACT)


def _wide(vol):
    g = VOLUMES[vol]
    return np.ascontiguousarray(g.astype(np.float32)) if g.dtype == np.float16 else g      # a binary16 volume renders as the widened floats


_ORACLE = {}


def _oracle_render(oracle, vol, med, est, rng, mis, trk, long):
    """(image, counters) of the oracle for one request's samples: once per session, read-only"""
    k = (vol, med, est, rng, mis, trk, long)
    if k not in _ORACLE:
        osc = oracle.OracleScene(_wide(vol), ENV, scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER, brick=_brick(est), estimator=est, rng_mode=rng,
                                 seed=KEY, env_mis=bool(mis), track_mode=trk)
        size, frames = (LONG_SIZE, LONG_FRAMES) if long else ((W, H), FRAMES)
        if long:
            osc.precompute_opacity()
        oP = oracle.default_param(size[0], size[1], **MEDIA[med])
        ref, cnt = None, None
        for f in range(frames):
            ref, c = osc.render_frame(oP, f, ref)
            d = c.as_dict()
            cnt = d if cnt is None else {q: cnt[q] + d[q] for q in d}
        ref.setflags(write=False)
        _ORACLE[k] = (ref, cnt)
    return _ORACLE[k]


def _by_context(rows):
    out = {}
    for row in rows:
        out.setdefault(row[1], []).append(row)
    return out


def _look_ahead(vp, buf, P, frames):
    vp.set_lookahead(64)
    for f in range(frames):
        vp.render_kernel(buf.ptr, f, P)
    vp.synchronize()
    vp.set_lookahead(vp.LOOKAHEAD_DEFAULT)


# ------------------------------------------------------------------------------------------------- the exact unit against the oracle
@pytest.mark.parametrize("est,rng", EXACT_GROUPS, ids=_ids(EXACT_GROUPS))
def test_every_exact_render_k_instance_runs_and_equals_the_oracle(vp, oracle, monkeypatch, est, rng):
    census = None
    for cname, rows in _by_context(_rows(est, rng)).items():
        c = _context(vp, monkeypatch, cname)
        try:
            with c:
                if census is None:
                    census = Census(vp, vp.CENSUS_EXACT, vp.CENSUS_RENDER)
                for name, _, vols, media, count, mis, trk, call, _ in rows:
                    for vol in vols:
                        for med in media:
                            what = (name, cname, vol, med)
                            long = call == "long"
                            ref, cnt = _oracle_render(oracle, vol, med, est, rng, mis, trk, long)
                            size, frames = (LONG_SIZE, LONG_FRAMES) if long else ((W, H), FRAMES)
                            P = _scene(vp, vol, med, est, rng, mis, trk, opacity=long, size=size)
                            buf = vp.DeviceBuffer(*size)
                            try:
                                vp.enable_counters(bool(count))
                                vp.read_counters(reset=True)
                                if call == "kernel":
                                    _look_ahead(vp, buf, P, frames)
                                else:
                                    vp.render_frames(buf.ptr, 0, frames, P)
                                got = buf.download()
                                k = vp.read_counters() if count else None
                            finally:
                                _reset_modes(vp)
                                buf.free()
                            ran = census.take(what, est, rng, vol, count, mis, trk)
                            assert np.array_equal(got, ref, equal_nan=True), (what, sorted(ran), int((got != ref).any(-1).sum()), "pixels differ")
                            if count:
                                for q in COUNTERS:
                                    assert k[q] == cnt[q], (what, sorted(ran), q, k[q], cnt[q])
                            if call == "kernel":
                                assert any(_digits(n)["cancel"] for n in ran), (what, "no look-ahead batch ran", sorted(ran))
        finally:
            c.destroy()
    walks = ["g%d" % rng] if est == 0 else ["l%d0" % rng, "l%d1" % rng, "t%d" % rng] if est == 1 else []
    census.assert_all_ran(est, rng, walks)


# ------------------------------------------------------------------------------------------- the layers twin against its expectation
@pytest.mark.parametrize("est,rng", EXACT_GROUPS, ids=_ids(EXACT_GROUPS))
def test_every_layers_render_k_instance_runs_and_equals_the_expectation(vp, oracle, monkeypatch, est, rng):
    census = None
    for cname, rows in _by_context(_rows(est, rng, LAYERS_ROWS)).items():
        c = _context(vp, monkeypatch, cname)
        try:
            with c:
                if census is None:
                    census = Census(vp, vp.CENSUS_EXACT, vp.CENSUS_LAYERS)
                for name, _, vols, media, _, _, _, call, _ in rows:
                    for vol in vols:
                        for med in media:
                            what = (name, cname, vol, med)
                            long = call == "long"
                            size, frames = (LONG_SIZE, LONG_FRAMES) if long else ((W, H), FRAMES)

                            def make():
                                real, twin = LL.scenes_for(oracle, _wide(vol), ENV, scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER, brick=_brick(est),
                                                           estimator=est, rng_mode=rng, seed=KEY)
                                if long:
                                    real.precompute_opacity()
                                    twin.precompute_opacity()
                                return real, twin, oracle.default_param(size[0], size[1], **MEDIA[med]), range(frames)
                            E = LL.expectation(oracle, ("census", vol, med, est, rng, long), make)
                            P = _scene(vp, vol, med, est, rng, opacity=long, size=size)
                            fg, tr = vp.DeviceBuffer(*size), vp.DeviceBuffer(*size)
                            try:
                                vp.render_frames_layers(fg.ptr, tr.ptr, 0, frames, P)
                                got = fg.download(), tr.download()
                            finally:
                                fg.free()
                                tr.free()
                            ran = census.take(what, est, rng, vol)
                            assert np.array_equal(got[0], E.fg, equal_nan=True), (what, sorted(ran), "fg", int((got[0] != E.fg).any(-1).sum()))
                            assert np.array_equal(got[1], E.trans, equal_nan=True), (what, sorted(ran), "trans", int((got[1] != E.trans).any(-1).sum()))
                            if not long:
                                assert E.unscattered.any() and not E.unscattered.all() and E.miss.any(), what
        finally:
            c.destroy()
    census.assert_all_ran(est, rng, [])


# -------------------------------------------------------------------------------------------------------------------- the fast unit
def _frames_one_by_one(vp, buf, P, frames):
    buf.reset()
    for f in range(frames):
        vp.render_frames(buf.ptr, f, 1, P)          # one-frame launches: no walk, no staging, the base instance
    return buf.download()


@pytest.mark.parametrize("est,rng", FAST_GROUPS, ids=_ids(FAST_GROUPS))
def test_every_fast_render_k_instance_runs_and_agrees(vp, monkeypatch, est, rng):
    census, base = None, {}
    for cname, rows in _by_context(_rows(est, rng, FAST_ROWS)).items():
        c = _context(vp, monkeypatch, cname)
        try:
            with c:
                if census is None:
                    census = Census(vp, vp.CENSUS_FAST, vp.CENSUS_RENDER)
                for name, _, vols, media, _, _, _, call, _ in rows:
                    for vol in vols:
                        for med in media:
                            what = (name, cname, vol, med)
                            long = call == "long"
                            size, frames = (LONG_SIZE, LONG_FRAMES) if long else ((W, H), FRAMES)
                            P = _scene(vp, vol, med, est, rng, opacity=long or est == 1, size=size)
                            buf = vp.DeviceBuffer(*size)
                            try:
                                if (vol, med, long) not in base:
                                    assert cname == "base"
                                    if not long and vol != "bin":
                                        _base_instance_against_the_exact_mode(vp, buf, P, what)
                                    vp.set_arithmetic(vp.ARITH_FAST)
                                    one = _frames_one_by_one(vp, buf, P, frames)
                                    assert np.isfinite(one).all() and (one >= 0).all() and one[..., :3].max() > 0, what
                                    one.setflags(write=False)
                                    base[(vol, med, long)] = one
                                    census.take(what + ("one frame at a time",), est, rng, vol)
                                vp.set_arithmetic(vp.ARITH_FAST)
                                buf.reset()
                                if call == "kernel":
                                    _look_ahead(vp, buf, P, frames)
                                else:
                                    vp.render_frames(buf.ptr, 0, frames, P)
                                got = buf.download()
                                assert vp.last_arithmetic() == vp.ARITH_FAST
                            finally:
                                _reset_modes(vp)
                                buf.free()
                            ran = census.take(what, est, rng, vol)
                            assert np.array_equal(got, base[(vol, med, long)]), (what, sorted(ran), int((got != base[(vol, med, long)]).any(-1).sum()), "pixels differ")
                            if call == "kernel":
                                assert any(_digits(n)["cancel"] for n in ran), (what, "no look-ahead batch ran", sorted(ran))
        finally:
            c.destroy()
    walks = ["g%d" % rng] if est == 0 else ["l%d0" % rng, "l%d1" % rng, "t%d" % rng]
    census.assert_all_ran(est, rng, walks)


def _base_instance_against_the_exact_mode(vp, buf, P, what):
    """checks 2 and 3 of tests/test_fuzz_fast_gpu.py on PAIRED_FRAMES one-frame renders in both arithmetic modes"""
    cls = vp.pixel_table(P)[..., 5].astype(int)
    d = np.empty((PAIRED_FRAMES, P.height, P.width, 3), np.float64)
    e = np.empty_like(d)
    for i in range(PAIRED_FRAMES):
        for m, out in ((vp.ARITH_EXACT, e), (vp.ARITH_FAST, d)):
            vp.set_arithmetic(m)
            buf.reset()
            vp.render_frames(buf.ptr, i, 1, P)
            out[i] = buf.download()[..., :3]
        assert np.array_equal(d[i][cls != 0], e[i][cls != 0]), (what, i, "box-missing / light pixels")
    assert_paired_agreement(d, e, what)
