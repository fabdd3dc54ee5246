"""What vp_render_adaptive_group_layers must leave behind (include/volpath.h): the definition restated on three
adaptive_lib.Stats, one per plane (sun, sky, trans).  A helper, not a test.

frame_triple(f) -> the three (H, W, 4) float32 one-frame images of the planes: group_layers_lib.Samples on the CPU oracle (of_samples),
or one-frame vp_render_frames_group_layers calls of the library (plane_stats_lib.library_frames).  A pixel is active while FROZEN is
clear in all three records; an active pixel receives every frame of the round in all three planes (Stats.add_frame); after the round it
is frozen, in all three records, iff each record has min_frames and meets adaptive_lib.criterion with its own n, tolerance and floor."""
import numpy as np

import adaptive_lib as AL
import adaptive_planes_lib as AP

FROZEN = AL.FROZEN
PLANES = ("sun", "sky", "trans")


def active_mask(st3, owned):
    m = owned.copy()
    for st in st3:
        m &= (st.flags & FROZEN) == 0
    return m


def render_adaptive_group_layers(st3, frame_triple, first, max_frames, rel_tol, floor_y, min_frames, round_frames, owned=None, tally=None):
    """the call on the state st3 (continued from whatever it holds); returns the result fields as a dict.  tally (a dict, optional)
    gains the pixel-rounds in which plane k ALONE held a pixel back -- the other two planes' halves of the decision held and plane k's
    did not: "held0", "held1", "held2"."""
    W, H = st3[0].W, st3[0].H
    owned = AL.all_pixels(W, H) if owned is None else owned
    done = rounds = samples = 0
    while done < max_frames:
        active = active_mask(st3, owned)
        if not active.any():
            break
        f = min(round_frames, max_frames - done)
        for k in range(f):
            for st, img in zip(st3, frame_triple(first + done + k)):
                st.add_frame(img, active)
        samples += int(active.sum()) * f          # one per pixel and frame, not per plane
        done += f
        rounds += 1
        ok = [AP.plane_ok(st3[k], k, rel_tol, floor_y, min_frames) for k in (0, 1, 2)]
        freeze = active & ok[0] & ok[1] & ok[2]
        for st in st3:
            st.flags[freeze] |= FROZEN
        if tally is not None:
            for k in (0, 1, 2):
                a, b = [j for j in (0, 1, 2) if j != k]
                tally["held%d" % k] = tally.get("held%d" % k, 0) + int((active & ok[a] & ok[b] & ~ok[k]).sum())
    return {"samples": samples, "rounds": rounds, "active_left": int(active_mask(st3, owned).sum()), "frames_used": done}


def new_triple(W, H):
    return tuple(AL.Stats(W, H) for _ in PLANES)


def copy_triple(st3):
    return tuple(s.copy() for s in st3)


def census(st3, min_frames, max_frames):
    """how a call from zeroed records went, by pixel: frozen at exactly min_frames, frozen strictly between, still active"""
    n = st3[0].n.astype(np.int64)
    for st in st3[1:]:
        assert np.array_equal(st3[0].n, st.n) and np.array_equal(st3[0].flags & FROZEN, st.flags & FROZEN)
    frozen = (st3[0].flags & FROZEN) != 0
    return {"at_min": int((frozen & (n == min_frames)).sum()), "between": int((frozen & (n > min_frames) & (n < max_frames)).sum()),
            "active": int((~frozen).sum())}


def same_triple(want, got):
    """None if (acc0, acc1, acc2, rec0, rec1, rec2) downloaded equal the three Stats bit for bit, flags included, else what differs"""
    for k in (0, 1, 2):
        bad = AL.same_state(want[k], got[k], got[3 + k])
        if bad is not None:
            return "plane %s: %s" % (PLANES[k], bad)
    return None


def of_samples(E):
    """frame_triple(f) of a group_layers_lib.Samples"""
    return lambda f: tuple(getattr(E, p)[f - E.first] for p in PLANES)


# ---- the anchors of the issue: layers_lib's scenes at 16 x 12 under key (11, 22)
ANCHOR_ARGS = dict(floor_y=(1e-3, 1e-3, 1e-2), min_frames=8, round_frames=4)
ANCHOR_FRAMES = 48
# (scene, estimator, stream, first frame) -> rel_tol (sun, sky, trans): the global majorant on Philox from frame 0; the decomposition
# estimator on Philox-7 from frame 4, which crosses its switch to the optical-depth table at frame 11
ANCHOR_TOL = {("soft", 0, 1, 0): (0.3, 0.1, 0.5), ("soft", 1, 2, 4): (0.3, 0.1, 0.5), ("julia", 0, 1, 0): (0.3, 0.1, 0.5), ("julia", 1, 2, 4): (0.5, 0.1, 0.3)}
ANCHORS = list(ANCHOR_TOL)
# the census of the four anchors on the CPU oracle: (frozen at min_frames, frozen later but before the last round, still active), and the
# pixel-rounds held back alone by (sun, sky, trans).  (The table these anchors were chosen from lists 171 for the last anchor's first
# count; this restatement gives 176 -- 176 + 11 + 5 is all 192 pixels, none is frozen by the last round -- and every other count as listed.)
ANCHOR_CENSUS = {("soft", 0, 1, 0): ((159, 10, 21), (13, 83, 8)), ("soft", 1, 2, 4): ((159, 7, 24), (21, 79, 6)),
                 ("julia", 0, 1, 0): ((172, 5, 14), (134, 22, 14)), ("julia", 1, 2, 4): ((176, 11, 5), (28, 21, 11))}
# a large floor takes a plane out of the decision; tolerances at which each plane alone freezes some pixels of the first anchor and not all
# (162, 182 and 172 of 192 on the oracle)
BIG_FLOOR, FLOOR_TOL = 1e30, (0.15, 0.15, 0.15)
_CACHE = {}


def anchor_samples(oracle, name, est, rng, first):
    """the group_layers_lib.Samples of an anchor's frames from the CPU oracle, once per session (group_layers_lib keeps them)"""
    import group_layers_lib as GLL
    return GLL.expected(oracle, name, est, rng, frames=range(first, first + ANCHOR_FRAMES))


def anchor_frames(oracle, name, est, rng, first):
    return of_samples(anchor_samples(oracle, name, est, rng, first))


def anchor_expected(oracle, name, est, rng, first):
    """(the three Stats, the result dict, the tally) of an anchor from zeroed records"""
    key = (name, est, rng, first)
    if key not in _CACHE:
        st, tally = new_triple(16, 12), {}
        res = render_adaptive_group_layers(st, anchor_frames(oracle, name, est, rng, first), first, ANCHOR_FRAMES, ANCHOR_TOL[key], tally=tally, **ANCHOR_ARGS)
        _CACHE[key] = (st, res, tally)
    st, res, tally = _CACHE[key]
    return copy_triple(st), dict(res), dict(tally)
