"""What vp_render_adaptive_groups and vp_render_adaptive_layers must leave behind (include/volpath.h): the
definition restated on two adaptive_lib.Stats, one per plane.  A helper, not a test.

frame_pair(f) -> the two (H, W, 4) float32 one-frame images of the planes: plane_stats_lib.oracle_group_frames / oracle_layer_frames
on the CPU oracle, plane_stats_lib.library_frames through the library's own plain plane calls, or planes_fuzz_lib.Frames.pair.  A pixel
is active while FROZEN is clear in both records; an active pixel receives every frame of the round in both planes (Stats.add_frame);
after the round it is frozen, in both records, iff each record has min_frames and meets adaptive_lib.criterion with its own n,
tolerance and floor."""
import numpy as np

import adaptive_lib as AL

FROZEN = AL.FROZEN


def active_mask(st_pair, owned):
    return owned & ((st_pair[0].flags & FROZEN) == 0) & ((st_pair[1].flags & FROZEN) == 0)


def plane_ok(st, k, rel_tol, floor_y, min_frames):
    """record by record: plane k's own half of the decision"""
    return (st.n >= min_frames) & AL.criterion(st.sum_y, st.sum_y2, st.n, rel_tol[k], floor_y[k])


def render_adaptive_planes(st_pair, frame_pair, first, max_frames, rel_tol, floor_y, min_frames, round_frames, owned=None, tally=None):
    """the call on the state st_pair (continued from whatever it holds); returns the result fields as a dict.  tally (a dict, optional)
    gains the pixel-rounds in which exactly one plane's half of the decision held: "only0", "only1"."""
    W, H = st_pair[0].W, st_pair[0].H
    owned = AL.all_pixels(W, H) if owned is None else owned
    done = rounds = samples = 0
    while done < max_frames:
        active = active_mask(st_pair, owned)
        if not active.any():
            break
        f = min(round_frames, max_frames - done)
        for k in range(f):
            for st, img in zip(st_pair, frame_pair(first + done + k)):
                st.add_frame(img, active)
        samples += int(active.sum()) * f          # one per pixel and frame, not per plane
        done += f
        rounds += 1
        ok = [plane_ok(st_pair[k], k, rel_tol, floor_y, min_frames) for k in (0, 1)]
        freeze = active & ok[0] & ok[1]
        for st in st_pair:
            st.flags[freeze] |= FROZEN
        if tally is not None:
            tally["only0"] = tally.get("only0", 0) + int((active & ok[0] & ~ok[1]).sum())
            tally["only1"] = tally.get("only1", 0) + int((active & ok[1] & ~ok[0]).sum())
    return {"samples": samples, "rounds": rounds, "active_left": int(active_mask(st_pair, owned).sum()), "frames_used": done}


def new_pair(W, H):
    return AL.Stats(W, H), AL.Stats(W, H)


def copy_pair(st_pair):
    return tuple(s.copy() for s in st_pair)


def census(st_pair, min_frames, max_frames):
    """how a call from zeroed records went, by pixel: frozen at exactly min_frames, frozen strictly between, still active"""
    n = st_pair[0].n.astype(np.int64)
    assert np.array_equal(st_pair[0].n, st_pair[1].n) and np.array_equal(st_pair[0].flags & FROZEN, st_pair[1].flags & FROZEN)
    frozen = (st_pair[0].flags & FROZEN) != 0
    return {"at_min": int((frozen & (n == min_frames)).sum()), "between": int((frozen & (n > min_frames) & (n < max_frames)).sum()),
            "active": int((~frozen).sum())}


def same_pair(want, got):
    """None if (acc0, acc1, rec0, rec1) downloaded equal the two Stats bit for bit, flags included, else what differs"""
    for k in (0, 1):
        bad = AL.same_state(want[k], got[k], got[2 + k])
        if bad is not None:
            return "plane %d: %s" % (k, bad)
    return None


# ---- the anchors of the issue: layers_lib's scenes at 16 x 12 under key (11, 22)
ANCHOR_ARGS = dict(floor_y=(1e-3, 1e-3), min_frames=8, round_frames=4)
ANCHOR_FRAMES = 48
ANCHOR_TOL = {"groups": (0.5, 0.05), "layers": (0.15, 0.5)}
# (estimator, stream, first frame): the global majorant on Philox from frame 0; the decomposition estimator on Philox-7 from frame 4,
# which crosses its switch to the optical-depth table at frame 11
ANCHOR_MODES = ((0, 1, 0), (1, 2, 4))
ANCHORS = [(kind, name, est, rng, first) for kind in ("groups", "layers") for name in ("soft", "julia") for est, rng, first in ANCHOR_MODES]
# the per-plane parameters: a large floor takes one plane out of the decision; tolerances at which either plane alone freezes some pixels
# of the scene and not all (178 and 172 of 192 on the oracle)
FLOOR_CASE, FLOOR_TOL, BIG_FLOOR = ("layers", "soft", 0, 1, 0), (0.15, 0.15), 1e30
_CACHE = {}


def anchor_frames(oracle, kind, name, est, rng, first):
    """frame_pair(f) of an anchor from the CPU oracle, with a memory that lasts the session"""
    import plane_stats_lib as PS
    key = (kind, name, est, rng)
    if key not in _CACHE:
        make = {"groups": PS.oracle_group_frames, "layers": PS.oracle_layer_frames}[kind]
        _CACHE[key] = make(oracle, name, est, rng, range(first, first + ANCHOR_FRAMES))
    return _CACHE[key]


def anchor_expected(oracle, kind, name, est, rng, first):
    """(the two Stats, the result dict, the tally) of an anchor from zeroed records"""
    key = ("run", kind, name, est, rng, first)
    if key not in _CACHE:
        st, tally = new_pair(16, 12), {}
        res = render_adaptive_planes(st, anchor_frames(oracle, kind, name, est, rng, first), first, ANCHOR_FRAMES, ANCHOR_TOL[kind], tally=tally, **ANCHOR_ARGS)
        _CACHE[key] = (st, res, tally)
    st, res, tally = _CACHE[key]
    return copy_pair(st), dict(res), dict(tally)
