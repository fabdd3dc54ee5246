"""What vp_render_frames_groups_stats and vp_render_frames_layers_stats must leave in their record buffers (include/volpath.h,
DESIGN.md section 2.8).  A helper, not a test.

The expectation is the definition restated: the per-frame sample of each plane -- groups_lib.sample / layers_lib.sample on the CPU
oracle, or a one-frame library render of the plane call into zeroed buffers -- folded with adaptive_lib.Stats.add_frame, one Stats per
plane: float32 luminance of the plane's sample, float64 sums in frame order, n + 1 per frame.  Stats.acc is the plane's accumulator,
which must equal groups_lib's / layers_lib's own Expectation of the same frames."""
import numpy as np

import adaptive_lib as AL
import groups_lib as GL
import layers_lib as LL
import scenes

F32 = np.float32
W, H, FRAMES, LONG, KEY = LL.W, LL.H, LL.FRAMES, LL.LONG, LL.KEY


def fold(frame_pair, W, H, first, n, owned=None, into=None):
    """(Stats of plane 0, Stats of plane 1) after frames first .. first + n - 1, continued from `into` where given;
    frame_pair(f) -> the two (H, W, 4) float32 one-frame images of the planes"""
    st = into if into is not None else (AL.Stats(W, H), AL.Stats(W, H))
    owned = AL.all_pixels(W, H) if owned is None else owned
    for f in range(first, first + n):
        for s, img in zip(st, frame_pair(f)):
            s.add_frame(img, owned)
    return st


def _scene_args(oracle, name, est, rng_mode, frames, density):
    g = LL.grid_of(name, oracle)
    g = np.ascontiguousarray(g.astype(np.float32)) if g.dtype == np.float16 else g      # a binary16 volume renders as the widened floats
    kw = dict(estimator=est, rng_mode=rng_mode, seed=KEY)
    pk = dict(LL.param_kw(name), **({} if density is None else {"density": density}))
    return g, kw, oracle.default_param(W, H, **pk), est == 1 and max(frames) > 10


def oracle_group_frames(oracle, name, est, rng_mode, frames, density=None):
    """frame_pair(f) of a groups call from groups_lib.sample on the oracle's twins: (sun image, sky image)"""
    g, kw, P, opacity = _scene_args(oracle, name, est, rng_mode, frames, density)
    trio = GL.scenes_for(oracle, g, GL.ENV, scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER, **kw)
    if opacity:
        for s in trio:
            s.precompute_opacity()

    def frame(f):
        sun, sky = np.zeros((H, W, 4), F32), np.zeros((H, W, 4), F32)
        for y in range(H):
            for x in range(W):
                sun[y, x], sky[y, x] = GL.sample(*trio, P, x, y, f)[:2]
        return sun, sky
    return AL.cached(frame)


def oracle_layer_frames(oracle, name, est, rng_mode, frames, density=None):
    """frame_pair(f) of a layers call from layers_lib.sample on the oracle: (fg image, trans image)"""
    g, kw, P, opacity = _scene_args(oracle, name, est, rng_mode, frames, density)
    real, twin = LL.scenes_for(oracle, g, LL.ENV, scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER, **kw)
    if opacity:
        real.precompute_opacity()
        twin.precompute_opacity()
    Q = LL.twin_param(oracle, P)

    def frame(f):
        fg, tr = np.zeros((H, W, 4), F32), np.zeros((H, W, 4), F32)
        for y in range(H):
            for x in range(W):
                fg[y, x], tr[y, x] = LL.sample(oracle, real, twin, P, x, y, f, Q)[:2]
        return fg, tr
    return AL.cached(frame)


_CACHE = {}


def expected(oracle, kind, name, est, rng_mode, frames=FRAMES, density=None):
    """the two read-only Stats of `kind` ("groups": sun, sky; "layers": fg, trans) on layers_lib's scene `name` over `frames` (a run of
    consecutive frames), from the oracle: once per session"""
    key = (kind, name, est, rng_mode, tuple(frames), density)
    if key not in _CACHE:
        frames = tuple(frames)
        assert frames == tuple(range(frames[0], frames[0] + len(frames)))
        make = {"groups": oracle_group_frames, "layers": oracle_layer_frames}[kind]
        st = fold(make(oracle, name, est, rng_mode, frames, density), W, H, frames[0], len(frames))
        for s in st:
            for k in ("acc", "sum_y", "sum_y2", "n", "flags"):
                getattr(s, k).setflags(write=False)
        _CACHE[key] = st
    return _CACHE[key]


def library_frames(render_pair, bufs):
    """frame_pair(f) through the library itself: render_pair(f) renders frame f alone with a plain plane call into the two zeroed
    DeviceBuffers `bufs` (current scene and modes)"""
    def frame(f):
        for b in bufs:
            b.reset()
        render_pair(f)
        return tuple(b.download() for b in bufs)
    return AL.cached(frame)


def same_records(st, rec, flags=None):
    """None if the downloaded records equal the restatement's bit for bit (flags: what they must hold, default 0), else what differs"""
    want = st.records()
    if flags is not None:
        want["flags"] = flags
    for k in ("n", "flags"):
        if not np.array_equal(want[k], rec[k]):
            return "%s (%d pixels)" % (k, int((want[k] != rec[k]).sum()))
    for k in ("sum_y", "sum_y2"):
        if not AL.equal_bits(want[k], rec[k]):
            return "%s (%d pixels)" % (k, int((want[k] != rec[k]).sum()))
    return None
