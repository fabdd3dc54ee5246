"""What vp_render_adaptive_halves and vp_render_adaptive_planes_halves must leave behind (include/volpath.h): the
definition restated on 2 N adaptive_lib.Stats -- N planes (N = 1: the beauty image) in two halves.  A helper, not a test.

halves = (h0, h1), each a tuple of N Stats in the mode's plane order.  frame_planes(f) -> the N (H, W, 4) float32 one-frame images of
the planes: adaptive_lib.oracle_frames / library_frames wrapped by beauty(), the plane sample tables of layers_lib, groups_lib and
group_layers_lib on the CPU oracle (oracle_plane_frames), or one-frame plain plane calls of the library (plane_stats_lib.library_frames).
A pixel is active while FROZEN is clear in all 2 N records; an active pixel receives every frame of the round, frame f in the N planes
of half halves_lib.half_of_frame(f, S) alone (Stats.add_frame: float32 luminance, float64 sums in frame order); after the round it is
frozen, in all 2 N records, iff every plane's two records hold two samples each, min_frames together and meet adaptive_lib.criterion on
their sums -- each one float64 addition, half 0 + half 1."""
import numpy as np

import adaptive_lib as AL
import halves_lib as HL

FROZEN = AL.FROZEN
LAYERS, GROUPS, GROUP_LAYERS = 1, 2, 3
PLANES = {0: ("beauty",), LAYERS: ("fg", "trans"), GROUPS: ("sun", "sky"), GROUP_LAYERS: ("sun", "sky", "trans")}


def new_halves(W, H, N=1):
    return tuple(tuple(AL.Stats(W, H) for _ in range(N)) for _ in (0, 1))


def copy_halves(halves):
    return tuple(tuple(s.copy() for s in h) for h in halves)


def beauty(frame):
    """frame_planes(f) of a one-plane frame(f)"""
    return lambda f: (frame(f),)


def _seq(v, N):
    return tuple(v) if np.ndim(v) else (v,) * N


def active_mask(halves, owned):
    m = owned.copy()
    for h in halves:
        for st in h:
            m &= (st.flags & FROZEN) == 0
    return m


def pooled(r0, r1):
    """(sum_y, sum_y2, n) of a plane's two records together: one float64 addition each, half 0 + half 1"""
    sy, sy2 = r0.sum_y + r1.sum_y, r0.sum_y2 + r1.sum_y2
    assert sy.dtype == AL.F64 and sy2.dtype == AL.F64
    return sy, sy2, r0.n + r1.n


def plane_ok(r0, r1, rel_tol, floor_y, min_frames):
    """one plane's part of the decision: two samples in each half, min_frames in both, the criterion on the pooled sums"""
    sy, sy2, n = pooled(r0, r1)
    return (r0.n >= 2) & (r1.n >= 2) & (n >= min_frames) & AL.criterion(sy, sy2, n, rel_tol, floor_y)


def add_round(halves, frame_planes, first, n, active, S=1):
    """frames [first, first + n) to the pixels of `active`: frame f into the planes of its half alone"""
    for f in range(first, first + n):
        for st, img in zip(halves[HL.half_of_frame(f, S)], frame_planes(f)):
            st.add_frame(img, active)


def freeze_round(halves, active, rel_tol, floor_y, min_frames):
    N = len(halves[0])
    tol, fl = _seq(rel_tol, N), _seq(floor_y, N)
    freeze = active.copy()
    for k in range(N):
        freeze &= plane_ok(halves[0][k], halves[1][k], tol[k], fl[k], min_frames)
    for h in halves:
        for st in h:
            st.flags[freeze] |= FROZEN
    return freeze


def render_adaptive_halves(halves, frame_planes, first, max_frames, rel_tol, floor_y, min_frames, round_frames, S=1, owned=None):
    """the call on the state `halves` (continued from whatever it holds); returns the result fields as a dict"""
    W, H = halves[0][0].W, halves[0][0].H
    owned = AL.all_pixels(W, H) if owned is None else owned
    done = rounds = samples = 0
    while done < max_frames:
        active = active_mask(halves, owned)
        if not active.any():
            break
        f = min(round_frames, max_frames - done)
        add_round(halves, frame_planes, first + done, f, active, S)
        samples += int(active.sum()) * f          # one per pixel and frame, not per plane or half
        done += f
        rounds += 1
        freeze_round(halves, active, rel_tol, floor_y, min_frames)
    return {"samples": samples, "rounds": rounds, "active_left": int(active_mask(halves, owned).sum()), "frames_used": done}


def frozen_mask(halves):
    """the pixels frozen in every record (what a call from zeroed records leaves: all 2 N flags agree)"""
    m = (halves[0][0].flags & FROZEN) != 0
    for h in halves:
        for st in h:
            assert np.array_equal((st.flags & FROZEN) != 0, m)
    return m


def census(halves, min_frames, max_frames):
    """how a call from zeroed records went, by pixel, with n the frames of both halves together: frozen with exactly min_frames, frozen
    strictly between, with all max_frames frames, still active"""
    n = halves[0][0].n.astype(np.int64) + halves[1][0].n.astype(np.int64)
    frozen = frozen_mask(halves)
    return {"at_min": int((frozen & (n == min_frames)).sum()), "between": int((frozen & (n > min_frames) & (n < max_frames)).sum()),
            "all_frames": int((n == max_frames).sum()), "active": int((~frozen).sum())}


def same_halves(want, got):
    """got: (h0's accumulators, h1's accumulators, h0's records, h1's records), each in plane order, downloaded.  None if they equal the
    2 N Stats bit for bit, flags included, else what differs"""
    N = len(want[0])
    assert len(got) == 4 * N
    for h in (0, 1):
        for k in range(N):
            bad = AL.same_state(want[h][k], got[h * N + k], got[2 * N + h * N + k])
            if bad is not None:
                return "half %d plane %d: %s" % (h, k, bad)
    return None


def prefilled(W, H, N, seed):
    """halves that already hold something (halves_lib.prefill: -0.0f among the accumulators, non-zero sums and counts, flag bits 0..1)"""
    out = new_halves(W, H, N)
    i = 0
    for h in out:
        for st in h:
            acc, rec = HL.prefill(W, H, seed + i)
            st.acc[:], st.sum_y[:], st.sum_y2[:], st.n[:], st.flags[:] = acc, rec["sum_y"], rec["sum_y2"], rec["n"], rec["flags"]
            i += 1
    return out


# ---- frames
_CACHE = {}


def anchor_frames(oracle, scenes, anchor):
    """frame(f) of an adaptive_lib anchor by the CPU oracle, with a memory that lasts the session"""
    key = ("anchor", anchor["est"], anchor["rng"], anchor["key"])
    if key not in _CACHE:
        osc, oP = AL.anchor_oracle(oracle, scenes, anchor)
        _CACHE[key] = AL.oracle_frames(osc, oP)
    return _CACHE[key]


def oracle_plane_frames(oracle, mode, name, est, rng_mode, frames):
    """frame_planes(f) of a plane mode from the CPU oracle's plane sample tables (layers_lib / groups_lib / group_layers_lib scenes at
    their 16 x 12), with a memory that lasts the session"""
    import adaptive_group_layers_lib as AGL
    import group_layers_lib as GLL
    import plane_stats_lib as PS
    key = ("planes", mode, name, est, rng_mode, frames[0], len(frames))
    if key not in _CACHE:
        if mode == GROUP_LAYERS:
            _CACHE[key] = AGL.of_samples(GLL.expected(oracle, name, est, rng_mode, frames=frames))
        else:
            make = {GROUPS: PS.oracle_group_frames, LAYERS: PS.oracle_layer_frames}[mode]
            _CACHE[key] = make(oracle, name, est, rng_mode, frames)
    return _CACHE[key]
