"""The random cases of tests/planes_fuzz_lib.py on the CPU: that their expectation is the header's (include/volpath.h, compositing
layers, light groups, statistics on planes), that few are left out, and that the lists reach what they are there for.  No GPU: this is
what tests/test_fuzz_planes_gpu.py holds the library against, checked on its own.  The lists are the defaults (32 short seeds, 8 long
ones), whatever the environment says."""
import numpy as np
import pytest

import adaptive_lib as AL
import layers_lib as LL
import planes_fuzz_lib as PF

F32 = np.float32
LISTS = {"short": (False, PF.SHORT_SEEDS), "long": (True, PF.LONG_SEEDS)}


def _pairs(oracle, which):
    """the (case, Frames) of a list; building them runs the helper's per-sample assertions: every twin stays on the path"""
    long, n = LISTS[which]
    return [PF.expectation(oracle, long, s) for s in range(n)]


def _admitted(oracle, which):
    return [(c, E) for c, E in _pairs(oracle, which) if PF.admissible(E) is None]


@pytest.mark.parametrize("which", LISTS)
def test_twins_stay_on_the_path_and_few_cases_are_left_out(oracle, which):
    pairs = _pairs(oracle, which)
    assert len(pairs) == LISTS[which][1]
    out = [(c["seed"], PF.admissible(E)) for c, E in pairs if PF.admissible(E) is not None]
    assert 16 * len(out) <= len(pairs), out                         # at most 1 case in 16
    for c, E in pairs:
        assert E.n == c["nframes"] and E.fg.shape == (c["nframes"], c["H"], c["W"], 4)
        if c["long"]:
            assert c["nframes"] >= 64 and c["W"] <= PF.MAX_W and c["H"] <= PF.MAX_H and max(c["grid"].shape) <= 20
        assert not c["env_mis"] and c["track"] == 0


def test_the_lists_are_not_vacuous(oracle):
    pairs = _admitted(oracle, "short") + _admitted(oracle, "long")
    n = PF.coverage(pairs)
    for k in ("est0", "est1", "est2", "u8", "f32", "f16", "user_box", "point_filter", "brick_gt1", "first_ge_977", "across_switch", "world_gt1",
              "rng0", "rng1", "rng2"):
        assert n[k] > 0, (k, n)
    assert n["cases"] == len(pairs)
    # a binary16 case is a float32 case rounded: its widened grid is not the float32 grid it came from, or the format would test nothing
    from volpath import host
    import scenes
    for c, _ in pairs:
        if c["grid"].dtype == np.float16:
            src = scenes.random_case((PF.LONG_BASE if c["long"] else PF.SHORT_BASE) + c["seed"], host)["grid"]
            assert src.dtype == np.float32 and not np.array_equal(c["grid"].astype(F32), src[:20, :20, :20] if c["long"] else src)


@pytest.mark.parametrize("which", LISTS)
def test_each_pixel_group_occurs_in_a_quarter_of_the_cases(oracle, which):
    pairs = _admitted(oracle, which)
    n = PF.coverage(pairs)
    for k in ("miss", "unscattered", "scattered", "mixed"):
        assert 4 * n[k] >= len(pairs), (k, n)
    assert n["no_miss"] > 0, n                                       # a camera inside the box, or a volume that fills the frame


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _in_disc(E):
    """(H, W) bool: the camera ray of the pixel lies inside the sun's disc (the rule of layers_lib.background)"""
    cos_sun = F32(94.0) / np.sqrt(F32(94.0) * F32(94.0) + F32(0.45) * F32(0.45), dtype=F32)
    out = np.zeros((E.H, E.W), bool)
    for y in range(E.H):
        for x in range(E.W):
            d = LL.camera_dir(E.inv_view, E.W, E.H, x, y)
            out[y, x] = d[0] * E.sun_dir[0] + d[1] * E.sun_dir[1] + d[2] * E.sun_dir[2] > cos_sun
    return out


@pytest.mark.parametrize("which", LISTS)
def test_per_sample_the_definitions_agree_with_each_other(oracle, which):
    seen_disc = 0
    for c, E in _admitted(oracle, which):
        w = _bits(E.beauty[..., 3])
        for k in ("fg", "sun", "sky"):
            assert np.array_equal(_bits(getattr(E, k)[..., 3]), w), (c["seed"], k, "w")
        u = E.unscattered
        assert np.array_equal(_bits(E.trans[..., 3]), np.where(u, _bits(F32(1.0)), np.uint32(0))), (c["seed"], "trans.w")
        assert not _bits(E.fg[u][:, :3]).any(), (c["seed"], "fg of an unscattered sample is +0")
        assert not _bits(E.trans[~u]).any(), (c["seed"], "trans of a scattered sample is +0")
        assert np.array_equal(_bits(E.fg[~u]), _bits(E.beauty[~u])), (c["seed"], "fg of a scattered sample is the beauty sample")
        # the disc rule (include/volpath.h, light groups): an unscattered path has R = 0 and ends along its camera ray
        disc = np.broadcast_to(_in_disc(E), u.shape)
        seen_disc += int((u & disc).sum())
        for m, lit, dark in ((u & disc, E.sun, E.sky), (u & ~disc, E.sky, E.sun)):
            assert np.array_equal(_bits(lit[m][:, :3]), _bits(E.beauty[m][:, :3])), (c["seed"], "the lit group is the beauty sample")
            assert not dark[m][:, :3].any(), (c["seed"], "the other group is 0")
        assert E.miss.shape == (c["H"], c["W"]) and u[:, E.miss].all()
    print(which, "unscattered samples inside the sun's disc:", seen_disc)


PINNED = ((False, 16), (False, 3), (True, 6))     # est 1 across the switch; binary16, sampler.h stream; a long case (the smallest)


@pytest.mark.parametrize("long,seed", PINNED)
def test_the_c_loop_is_the_python_loop_byte_for_byte(oracle, long, seed):
    """vpo_render_samples against the per-sample loop over layers_lib.sample and groups_lib.sample, each twin with an optical-depth
    table of its own"""
    c, E = PF.expectation(oracle, long, seed)
    P = PF.Frames(oracle, c, loop="python", share_opacity=False)
    for k in PF.VALUES + PF.FLAGS + ("miss",):
        assert getattr(E, k).tobytes() == getattr(P, k).tobytes(), (seed, k)
    assert E.unscattered.any() and not E.unscattered.all()
    assert c["late"] == ((long, seed) != PINNED[1])                 # two of the three read the optical-depth table


def test_accumulators_and_records_derive_from_the_samples(oracle):
    """Frames.acc and Frames.stats: float32 sums in frame order, the fold of plane_stats_lib, and a job in two parts is the job"""
    c, E = PF.expectation(oracle, False, 16)
    for kind, planes in PF.PLANES.items():
        whole = E.stats(kind)
        part = E.stats(kind, 2, None, into=E.stats(kind, 0, 2))
        for j, name in enumerate(planes):
            a = np.zeros((E.H, E.W, 4), F32)
            for i in range(E.n):
                a += getattr(E, name)[i]
            assert E.acc(name).tobytes() == a.tobytes() == whole[j].acc.tobytes() == part[j].acc.tobytes()
            assert AL.same_state(whole[j], part[j].acc, part[j].records()) is None
            assert (whole[j].n == E.n).all() and (whole[j].sum_y > 0).any()
