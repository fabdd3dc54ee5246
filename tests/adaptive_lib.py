"""What the statistics / adaptive-sampling tests share: the numpy restatement of include/volpath.h's definition.

A sample is a pure function of (pixel, frame, keys, scene), so everything a stats-carrying render leaves behind is defined by the
frames themselves: `frame(f)` below is frame f rendered on its own into a zeroed buffer, (H, W, 4) float32 -- by the CPU oracle, or
by the library one frame at a time.  The restatement is float32 luminance, float64 sums in frame order, the criterion in float64
with the binary32 arguments widened, the round loop, and the output stage.  numpy rounds every operation to its dtype and contracts
nothing, so the bits are the definition's."""
import numpy as np

FROZEN = 1
F32 = np.float32
F64 = np.float64


def luminance(v):
    """y = (0.2126f * v.x + 0.7152f * v.y) + 0.0722f * v.z in binary32"""
    v = np.asarray(v, F32)
    y = (F32(0.2126) * v[..., 0] + F32(0.7152) * v[..., 1]) + F32(0.0722) * v[..., 2]
    assert y.dtype == F32
    return y


class Stats:
    """accumulator and records of a W x H image, zeroed"""

    def __init__(self, W, H):
        self.W, self.H = W, H
        self.acc = np.zeros((H, W, 4), F32)
        self.sum_y = np.zeros((H, W), F64)
        self.sum_y2 = np.zeros((H, W), F64)
        self.n = np.zeros((H, W), np.uint32)
        self.flags = np.zeros((H, W), np.uint32)

    def copy(self):
        c = Stats(self.W, self.H)
        for k in ("acc", "sum_y", "sum_y2", "n", "flags"):
            setattr(c, k, getattr(self, k).copy())
        return c

    def add_frame(self, img, mask):
        """one sample per pixel of `mask` from the one-frame image img"""
        img = np.asarray(img, F32)
        y = luminance(img).astype(F64)
        self.acc[mask] = self.acc[mask] + img[mask]
        self.sum_y[mask] = self.sum_y[mask] + y[mask]
        self.sum_y2[mask] = self.sum_y2[mask] + y[mask] * y[mask]
        self.n[mask] += 1

    def records(self):
        """the records as the library's structured array (volpath.PIXEL_STATS_DTYPE layout)"""
        out = np.zeros((self.H, self.W), np.dtype([("sum_y", F64), ("sum_y2", F64), ("n", np.uint32), ("flags", np.uint32)]))
        out["sum_y"], out["sum_y2"], out["n"], out["flags"] = self.sum_y, self.sum_y2, self.n, self.flags
        return out


def all_pixels(W, H):
    return np.ones((H, W), bool)


def owned_pixels(volpath, W, H, rank, world):
    """the pixels of the 8x8 tiles that vp_tile_owner deals to `rank`"""
    m = np.zeros((H, W), bool)
    for ty in range((H + 7) // 8):
        for tx in range((W + 7) // 8):
            if volpath.tile_owner(tx, ty, world) == rank:
                m[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8] = True
    return m


def render_uniform(st, frame, first, n, owned=None):
    """vp_render_frames_stats: every owned pixel receives every frame; flags are neither read nor written"""
    owned = all_pixels(st.W, st.H) if owned is None else owned
    for f in range(first, first + n):
        st.add_frame(frame(f), owned)
    return st


def criterion(sum_y, sum_y2, n, rel_tol, floor_y):
    """lhs <= rhs of the definition, binary64, the binary32 arguments widened; False where either side is NaN"""
    tol, fl = F64(F32(rel_tol)), F64(F32(floor_y))
    nd = n.astype(F64)
    with np.errstate(all="ignore"):
        lhs = nd * sum_y2 - sum_y * sum_y
        nf = nd * fl
        m = np.where(sum_y > nf, sum_y, nf)
        rhs = ((tol * tol) * (nd - 1.0)) * (m * m)
        return lhs <= rhs


def freeze_round(st, active, rel_tol, floor_y, min_frames):
    """after a round: each pixel that was active in it is frozen iff n >= min_frames and the criterion holds"""
    freeze = active & (st.n >= min_frames) & criterion(st.sum_y, st.sum_y2, st.n, rel_tol, floor_y)
    st.flags[freeze] |= FROZEN
    return freeze


def render_adaptive(st, frame, first, max_frames, rel_tol, floor_y, min_frames, round_frames, owned=None):
    """vp_render_adaptive on the state st (continued from whatever it holds); returns the result fields as a dict"""
    owned = all_pixels(st.W, st.H) if owned is None else owned
    done = rounds = samples = 0
    while done < max_frames:
        active = owned & ((st.flags & FROZEN) == 0)
        if not active.any():
            break
        f = min(round_frames, max_frames - done)
        for k in range(f):
            st.add_frame(frame(first + done + k), active)
        samples += int(active.sum()) * f
        done += f
        rounds += 1
        freeze_round(st, active, rel_tol, floor_y, min_frames)
    return {"samples": samples, "rounds": rounds, "active_left": int((owned & ((st.flags & FROZEN) == 0)).sum()), "frames_used": done}


def scale_by_count(src, n, scale):
    """vp_scale_by_count: each channel times (scale / (float)n), the divide in binary32; n == 0 gives 0"""
    src = np.asarray(src, F32)
    with np.errstate(all="ignore"):
        s = F32(scale) / n.astype(F32)
    out = src * s[..., None]
    out[n == 0] = 0
    assert out.dtype == F32
    return out


def rel_error(sum_y, sum_y2, n, floor_y):
    """vp_stats_rel_error in binary64 (the library rounds it once to binary32); n < 2 gives 0"""
    fl = F64(F32(floor_y))
    nd = n.astype(F64)
    with np.errstate(all="ignore"):
        lhs = nd * sum_y2 - sum_y * sum_y
        var = np.where(lhs > 0.0, lhs, 0.0) / (nd * nd * (nd - 1.0))
        mean = sum_y / nd
        out = np.sqrt(var) / np.where(mean > fl, mean, fl)
    out[n < 2] = 0.0
    return out


def cached(frame):
    """frame(f) with a memory: the same frames feed several restatements"""
    memo = {}

    def get(f):
        if f not in memo:
            memo[f] = frame(f)
        return memo[f]
    return get


def oracle_frames(osc, oP):
    """frame(f) by the CPU oracle"""
    return cached(lambda f: osc.render_frame(oP, f, None)[0])


def library_frames(vp, P):
    """(frame(f), buffer) through the library itself: one plain frame at a time into a zeroed buffer (current scene and modes)"""
    buf = vp.DeviceBuffer(P.width, P.height)

    def frame(f):
        buf.reset()
        vp.render_frames(buf.ptr, f, 1, P)
        return buf.download()
    return cached(frame), buf


def equal_bits(a, b):
    """float arrays of one dtype compared by their bit patterns; a NaN equals a NaN (its sign and payload are not defined)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.dtype in (F32, F64) and a.shape == b.shape
    u = np.uint32 if a.dtype == F32 else np.uint64
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(u)[~na], b.view(u)[~nb])


def same_state(st, acc, rec):
    """None if the accumulator and the downloaded records equal the restatement bit for bit, else what differs"""
    acc = np.ascontiguousarray(acc, F32)
    if not equal_bits(st.acc, acc):
        return "accumulator (%d pixels)" % int(((st.acc != acc) & ~(np.isnan(st.acc) & np.isnan(acc))).any(axis=-1).sum())
    if not np.array_equal(st.n, rec["n"]):
        return "n (%d pixels)" % int((st.n != rec["n"]).sum())
    if not np.array_equal(st.flags, rec["flags"]):
        return "flags (%d pixels)" % int((st.flags != rec["flags"]).sum())
    if not equal_bits(st.sum_y, rec["sum_y"]):
        return "sum_y"
    if not equal_bits(st.sum_y2, rec["sum_y2"]):
        return "sum_y2"
    return None


def estimate_ratio(records):
    """Does the estimate mean what it says?  records: K uniform renders of one scene under independent keys.  Over the pixels whose K
    means differ at all: root mean square of the estimated standard error of the mean (the noise map's numerator) over the root mean
    square spread of the K means (sample variance, K - 1).  1 for an honest estimate.  Returns (ratio, pixels)."""
    means, var = [], []
    for r in records:
        nd = r["n"].astype(F64)
        means.append(r["sum_y"] / nd)
        var.append(np.maximum(nd * r["sum_y2"] - r["sum_y"] * r["sum_y"], 0.0) / (nd * nd * (nd - 1.0)))
    means, var = np.array(means), np.array(var)
    spread = means.var(axis=0, ddof=1)
    m = spread > 0
    return float(np.sqrt(var[:, m].mean() / spread[m].mean())), int(m.sum())


def census(st, first_min, max_frames):
    """how an adaptive render went: pixels frozen with exactly first_min frames, frozen strictly between, with all max_frames frames, still
    active; and the per-boundary counts in between"""
    n, frozen = st.n.astype(np.int64), (st.flags & FROZEN) != 0
    between = frozen & (n > first_min) & (n < max_frames)
    per = {int(k): int((between & (n == k)).sum()) for k in np.unique(n[between])}
    return {"at_min": int((frozen & (n == first_min)).sum()), "between": int(between.sum()), "all_frames": int((n == max_frames).sum()),
            "active": int((~frozen).sum()), "per_boundary": per, "samples": int(n.sum())}


# ---- the two anchors of the issue: Julia-32, 64x48, default camera and sun, scenes.synthetic_env()
ANCHOR1 = dict(est="global", rng="philox", key=(1, 2), rel_tol=0.1, floor_y=1e-3, min_frames=16, round_frames=8, max_frames=96)
ANCHOR2 = dict(est="decomp", rng="philox7", key=(1, 2), rel_tol=0.2, floor_y=1e-3, min_frames=8, round_frames=4, max_frames=32)
ANCHOR_W, ANCHOR_H = 64, 48


def anchor_oracle(oracle, scenes, anchor):
    """(OracleScene, Param) of an anchor"""
    est = {"global": oracle.EST_GLOBAL, "decomp": oracle.EST_DECOMP}[anchor["est"]]
    rng = {"philox": oracle.RNG_PHILOX, "philox7": oracle.RNG_PHILOX7}[anchor["rng"]]
    osc = oracle.OracleScene(oracle.julia(32), scenes.synthetic_env(), scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER, estimator=est, rng_mode=rng,
                             seed=anchor["key"])
    if est == oracle.EST_DECOMP:
        osc.precompute_opacity()
    return osc, oracle.default_param(ANCHOR_W, ANCHOR_H)


def anchor_args(anchor):
    return {k: anchor[k] for k in ("rel_tol", "floor_y", "min_frames", "round_frames")}
