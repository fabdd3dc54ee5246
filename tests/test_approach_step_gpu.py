"""GPU parity for the approach walks' trimmed free-flight step (approach_k, approach_local_k, approach_local_tab_k;
profiles/experiments/approach_step.txt):

  - logf_'s exponent bias folded into its first constant, and logf_pos_ (no answer for 0): vp_test_log_forms compares both with the
    chain as it stood, on every bit pattern of their domains;
  - one compare per step against the nearer limit, a zero draw tested by the loop, the stream's state formed behind the loop, two steps
    per iteration: vp_test_approach_walk runs the walks as built and the loops as they stood on scripted streams -- every field of
    the hand-over (distance, steps, the stream's state, through) equal, bit for bit, in every case;
  - end to end at the smallest shapes that take every path: a 32^3 volume with one blob in the corner far from the camera, 48 x 32
    pixels, 5 / 64 / 128 frames per launch (the untabulated walk; the tabulated one, one and two blocks of 64 frames), the three
    estimators on three streams, uchar and float cells, with the walk's step cap unset, 0, 1 and 7: image and work counters equal
    the CPU oracle's, tolerance 0.
No exclusions, no tolerance."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import scenes

pytestmark = pytest.mark.gpu

f32, u32 = np.float32, np.uint32
VP_E_ARG = -3


def _bits(x):
    return int(f32(x).view(u32))


@contextlib.contextmanager
def _arith(vp, mode):
    vp.set_arithmetic(mode)
    try:
        yield
    finally:
        vp.set_arithmetic(vp.ARITH_EXACT)


# ------------------------------------------------------------------------------------------ 1. the logarithm's forms, every pattern
@pytest.mark.parametrize("arith", [0, 1], ids=["exact", "fast"])
def test_logf_equals_the_unfolded_chain_on_every_non_negative_float(vp, arith):
    """+0, the subnormals (outside logf_'s domain, equal all the same), every normal float and +inf: 0x7f800001 patterns"""
    with _arith(vp, arith):
        bad, first = vp.test_log_forms(0, 0x00000000, 0x7F800000)
    print(f"logf_: {bad} mismatches, first {first}")
    assert (bad, first) == (0, None)


@pytest.mark.parametrize("arith", [0, 1], ids=["exact", "fast"])
def test_logf_pos_equals_the_unfolded_chain_on_its_domain(vp, arith):
    """[2^-126, +inf]: every pattern from 0x00800000 to 0x7f800000"""
    with _arith(vp, arith):
        bad, first = vp.test_log_forms(1, 0x00800000, 0x7F800000)
    print(f"logf_pos_: {bad} mismatches, first {first}")
    assert (bad, first) == (0, None)


def test_logf_pos_has_no_answer_for_zero(vp):
    """what the walks test for themselves: at 0 the chain without the select is not -inf (if it were, the select would be free)"""
    bad, first = vp.test_log_forms(1, 0, 0)
    assert (bad, first) == (1, 0)


def test_hooks_refuse_bad_arguments(vp):
    L = vp.lib()
    m, f = C.c_uint64(0), C.c_uint32(0)
    assert L.vp_test_log_forms(2, 0, 0, C.byref(m), C.byref(f)) == VP_E_ARG
    assert L.vp_test_log_forms(-1, 0, 0, C.byref(m), C.byref(f)) == VP_E_ARG
    assert L.vp_test_log_forms(0, 2, 1, C.byref(m), C.byref(f)) == VP_E_ARG
    assert L.vp_test_log_forms(0, 0, 0, None, C.byref(f)) == VP_E_ARG
    assert L.vp_test_log_forms(0, 0, 0, C.byref(m), None) == VP_E_ARG
    par, scr, words = np.zeros((1, 4), f32), np.array([[1, 0, 2, 0]], u32), np.zeros(2, u32)
    new, ref = np.zeros((1, 5), u32), np.zeros((1, 5), u32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.vp_test_approach_walk(2, 1, p(par), p(scr), p(words), 2, p(new), p(ref)) == VP_E_ARG
    assert L.vp_test_approach_walk(0, -1, p(par), p(scr), p(words), 2, p(new), p(ref)) == VP_E_ARG
    assert L.vp_test_approach_walk(0, 1, None, p(scr), p(words), 2, p(new), p(ref)) == VP_E_ARG
    assert L.vp_test_approach_walk(0, 1, p(par), p(scr), p(words), 2, None, p(ref)) == VP_E_ARG
    assert L.vp_test_approach_walk(0, 1, p(par), p(scr), None, 2, p(new), p(ref)) == VP_E_ARG
    assert L.vp_test_approach_walk(0, 1, p(par), p(scr), p(words), 1, p(new), p(ref)) == VP_E_ARG      # two words asked for, one given
    scr[0, 1] = 3
    assert L.vp_test_approach_walk(0, 1, p(par), p(scr), p(words), 2, p(new), p(ref)) == VP_E_ARG      # the script starts behind the words
    assert L.vp_test_approach_walk(0, 0, p(par), p(scr), p(words), 2, p(new), p(ref)) == 0             # no case: nothing to check


# ------------------------------------------------------------------------------------------ 2. scripted walks
N_CASES = 20000
BIG_CAPS = (250, 251, 1 << 20, (1 << 20) + 1)


def _cases(kind, seed):
    """(params [n, 4], script [n, 4], words): N_CASES seeded cases of walk `kind`.  A flight is -log(u) / majorant, about one
    reciprocal long: the limits are laid a random number of flights away, so walks end by a limit, by the cap (kind 0), by a zero
    draw and by the script's end (draws of 0 behind it) in comparable numbers."""
    rng = np.random.default_rng(seed)
    n = N_CASES
    count = rng.integers(0, 301, n).astype(u32)                      # words per case: 0..300
    first = np.concatenate([[0], np.cumsum(count)[:-1]]).astype(u32)
    words = rng.integers(512, 2 ** 32, int(count.sum()), dtype=np.uint64).astype(u32)   # no zero draw unless one is put there
    inv = (10.0 ** rng.uniform(-3.5, -0.5, n)).astype(f32)           # the majorant's reciprocal over three decades
    dist = np.where(rng.random(n) < 0.2, 0.0, rng.uniform(0.0, 2.0, n)).astype(f32)
    # the certified-empty distance a random number of flights ahead; the other limit on either side of it
    t_empty = (dist + inv * rng.uniform(0.0, 320.0, n)).astype(f32)
    t_box = (dist + inv * rng.uniform(0.0, 320.0, n)).astype(f32)
    far = rng.random(n) < 0.3
    t_box[far] = (t_empty[far] * f32(4.0) + f32(1.0))
    # caps of 0, 1, 2, 3 and large odd / even ones (two steps per iteration); a cap inside the script for every fourth case
    cap = rng.choice(np.array((0, 1, 2, 3) + BIG_CAPS, np.int64), n)
    inside = rng.random(n) < 0.25
    cap[inside] = rng.integers(0, 301, int(inside.sum()))
    # half of the cases draw exactly 0 somewhere: a word below 512 at a random place, at the first step, at the cap (the last step
    # the cap allows and the first it does not), and in the second step of an iteration
    zero = np.flatnonzero((rng.random(n) < 0.5) & (count > 0))
    how = rng.integers(0, 5, zero.size)
    for i, h in zip(zero, how):
        c = int(count[i])
        pos = (int(rng.integers(0, c)), 0, max(int(cap[i]) - 1, 0), int(cap[i]), 2 * int(rng.integers(0, c)) + 1)[h]
        if h in (2, 3) and cap[i] >= c:   # a large cap: put the cap at the zero instead
            pos = int(rng.integers(0, c))
            cap[i] = pos + (1 if h == 2 else 0)
        words[int(first[i]) + min(pos, c - 1)] = rng.integers(0, 512)
    # special certificates: 0, NaN, 1e30
    special = rng.permutation(n)[:600]
    t_empty[special[:200]] = 0.0
    t_empty[special[200:400]] = np.nan
    t_empty[special[400:]] = 1e30
    pair0 = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(u32)
    pair0[rng.random(n) < 0.2] = 0
    pair0[rng.random(n) < 0.05] = 0xFFFFFFF0                          # the pair index wraps inside the walk
    par = np.stack([dist, t_empty, t_box, inv], 1).astype(f32)
    scr = np.stack([cap.astype(u32), first, count, pair0], 1).astype(u32)
    return par, scr, words


def _exact_landings(vp, kind, par, scr, words):
    """cases whose flight lands exactly ON the limit, built by solving for t_empty from a recorded distance: walk with the limits
    out of the way and a cap of k steps (kind 0) / a far limit (kind 1), take the distance reached d_k, and lay t_empty at d_k, one
    ulp below and one ulp above it: the k-th flight must stop, stop and pass"""
    rng = np.random.default_rng(77 + kind)
    pick = np.flatnonzero(scr[:, 2] >= 8)[:2000]
    p, s = par[pick].copy(), scr[pick].copy()
    p[:, 1] = 1e30
    p[:, 2] = 1e30 if kind == 0 else p[:, 0] + p[:, 3] * f32(40.0)
    k = rng.integers(1, 8, pick.size).astype(u32)
    s[:, 0] = k
    _, ref = vp.test_approach_walk(kind, p, s, words)
    d_k = ref[:, 0].copy().view(f32)
    ok = np.isfinite(d_k) & (ref[:, 1] >= 1)
    out_p, out_s = [], []
    for shift in (0, -1, 1):
        q, t = p[ok].copy(), s[ok].copy()
        q[:, 1] = (d_k[ok].view(u32).astype(np.int64) + shift).astype(u32).view(f32)
        q[:, 2] = 1e30 if kind == 0 else q[:, 0] + q[:, 3] * f32(400.0)
        t[:, 0] = 1 << 20
        out_p.append(q)
        out_s.append(t)
    assert ok.sum() > 500
    return np.concatenate(out_p), np.concatenate(out_s)


@pytest.mark.parametrize("arith", [0, 1], ids=["exact", "fast"])
@pytest.mark.parametrize("kind", [0, 1], ids=["global", "local"])
def test_scripted_walks_hand_over_what_the_loops_they_replaced_did(vp, kind, arith):
    par, scr, words = _cases(kind, 1000 + kind)
    with _arith(vp, arith):
        new, ref = vp.test_approach_walk(kind, par, scr, words)
        lp, ls = _exact_landings(vp, kind, par, scr, words)
        lnew, lref = vp.test_approach_walk(kind, lp, ls, words)
    # the census: every way out of the loop is taken, in both of an iteration's steps
    steps, through = ref[:, 1].astype(np.int64), ref[:, 4]
    at_cap = (kind == 0) & (steps == scr[:, 0])
    ran_out = steps == scr[:, 2]
    stopping = np.minimum(scr[:, 1].astype(np.int64) + steps, len(words) - 1)     # the word of the flight that ended the walk
    zero_stop = (~at_cap) & (scr[:, 2] > steps) & (words[stopping] < 512)
    census = dict(cases=len(steps), no_step=int((steps == 0).sum()), odd=int((steps % 2 == 1).sum()), even=int(((steps % 2 == 0) & (steps > 0)).sum()),
                  at_cap=int(at_cap.sum()), script_end=int(ran_out.sum()), zero_draw=int(zero_stop.sum()), through=int(through.sum()),
                  nan_certificate=int(np.isnan(par[:, 1]).sum()), longest=int(steps.max()), landings=len(lref))
    print(f"kind {kind} arith {arith}: {census}")
    assert census["cases"] == N_CASES and census["odd"] > 2000 and census["even"] > 2000 and census["no_step"] > 500
    assert census["zero_draw"] > 1000 and census["script_end"] > 200 and census["longest"] >= 250
    assert (census["at_cap"] > 2000) if kind == 0 else (200 < census["through"] < N_CASES - 200)
    # the bar: every field of every hand-over
    for got, want, what in ((new, ref, "cases"), (lnew, lref, "landings")):
        differ = np.flatnonzero((got != want).any(1))
        assert differ.size == 0, (what, differ.size, differ[:5].tolist(), got[differ[:3]].tolist(), want[differ[:3]].tolist())
    # the landings do what they were built for: on the limit and below it the walk makes one step less than above it
    third = len(lref) // 3
    on, below, above = lref[:third, 1].astype(np.int64), lref[third:2 * third, 1].astype(np.int64), lref[2 * third:, 1].astype(np.int64)
    assert (below <= on).all() and (above >= on + 1).all()


@pytest.mark.parametrize("kind", [0, 1], ids=["global", "local"])
def test_a_majorant_with_a_minus_sign_keeps_its_bits(vp, kind):
    """flights that run backwards (a negative reciprocal, -0 included) mean nothing, and a zero draw does not stop them: the walks
    keep the loop with logf_ for them"""
    par, scr, words = _cases(kind, 5000 + kind)
    par, scr = par[:2000].copy(), scr[:2000].copy()
    par[:, 3] = -par[:, 3]
    par[::7, 3] = -0.0
    scr[:, 0] = np.minimum(scr[:, 0], 400)
    new, ref = vp.test_approach_walk(kind, par, scr, words)
    assert np.array_equal(new, ref)


# ------------------------------------------------------------------------------------------ 3. end to end
W, H = 48, 32
DENSITY = 100.0     # a hundred null collisions per unit length on the way to the blob: oracle frames stay cheap
KEY = (0xA9904C, 5)
FRAMES = (5, 64, 128)
COUNTERS = ("samples", "density_lookups", "bound_lookups", "opacity_lookups", "env_lookups", "scatters")
ESTS = {"global": 0, "decomp": 1, "bounded": 2}
RNGS = {"philox7": 2, "philox": 1, "samplerh": 0}


def _grid(cells):
    """32^3, empty but for a 6^3 blob in the corner far from the default camera (which looks down -x from x = +3.9, y = -0.8):
    low x, high y, low z -- a long certified-empty stretch, then a fetch"""
    g = np.zeros((32, 32, 32), np.uint8)
    g[0:6, 26:32, 0:6] = 255
    return g if cells == "u8" else g.astype(f32) * f32(1.0 / 255.0)


_ORACLE = {}


def _oracle(oracle, cells, est, rng_mode):
    """{frames: (accumulator, summed counters)} after 5, 64 and 128 frames from frame 0: one pass, shared, never written to"""
    k = (cells, est, rng_mode)
    if k not in _ORACLE:
        sc = oracle.OracleScene(_grid(cells), scenes.synthetic_env(), scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER, brick=1, estimator=est,
                                rng_mode=rng_mode, seed=KEY)
        if est == oracle.EST_DECOMP:
            sc.precompute_opacity()
        P = oracle.default_param(W, H, density=DENSITY)
        acc, cnt, out = None, None, {}
        for f in range(max(FRAMES)):
            acc, c = sc.render_frame(P, f, acc)
            d = c.as_dict()
            cnt = d if cnt is None else {q: cnt[q] + d[q] for q in d}
            if f + 1 in FRAMES:
                snap = acc.copy()
                snap.setflags(write=False)
                assert np.isfinite(snap).all()
                out[f + 1] = (snap, dict(cnt))
        _ORACLE[k] = out
    return _ORACLE[k]


@contextlib.contextmanager
def _context(vp, cap):
    """a context created with the walk's step cap `cap` (None: unset; knobs are read at creation, the mechanism of test_c4_gpu.py's knob
    test) that takes no volume for dense: the approach walks always run"""
    env = dict(VP_DENSE_PERCENT="101")
    if cap is not None:
        env["VP_APPROACH_STEPS"] = str(cap)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        c = vp.Context(0)
    finally:
        for k, v in old.items():
            os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)
    try:
        with c:
            yield c
    finally:
        c.destroy()


def _scene(vp, cells, est, rng_mode):
    vp.set_arithmetic(vp.ARITH_EXACT)
    vp.set_subpixel(1)
    vp.init_volume(_grid(cells), brick=1, linear=True)
    vp.init_envmap(scenes.synthetic_env())
    vp.set_sun(scenes.DEFAULT_SUN_DIR, scenes.DEFAULT_SUN_POWER)
    vp.set_camera()
    vp.set_estimator(est)
    vp.set_rng(rng_mode, KEY)
    vp.set_tracking(0)
    vp.set_envmap_sampling(vp.ENV_PASSIVE)
    vp.set_shard(0, 1)
    if est == vp.EST_DECOMP:
        vp.precompute_opacity(scenes.DEFAULT_SUN_DIR)


@pytest.mark.parametrize("cap", [None, 0, 1, 7], ids=["cap_unset", "cap0", "cap1", "cap7"])
@pytest.mark.parametrize("cells", ["u8", "f32"])
@pytest.mark.parametrize("est", list(ESTS))
def test_renders_and_work_counters_equal_the_oracle(vp, oracle, monkeypatch, est, cells, cap):
    e = ESTS[est]
    with _context(vp, cap):
        P = vp.make_param(W, H, density=DENSITY)
        buf = vp.DeviceBuffer(W, H)
        try:
            for rng_name, r in RNGS.items():
                ref = _oracle(oracle, cells, e, r)
                assert ref[max(FRAMES)][0][..., 3].max() > 0.0, "no path reaches the blob"
                _scene(vp, cells, e, r)
                for n in FRAMES:
                    what = (est, cells, cap, rng_name, n)
                    acc, cnt = ref[n]
                    buf.reset()
                    vp.render_frames(buf.ptr, 0, n, P)                       # the timed kernels
                    got = buf.download()
                    assert got.tobytes() == acc.tobytes(), (what, int((got != acc).any(-1).sum()))
                    mode, table = vp.last_approach_mode(), vp.last_approach_table()
                    if e != vp.EST_BOUNDED:
                        assert mode != 0, (what, "no approach walk in this launch")
                    if e == vp.EST_DECOMP and cells == "u8":
                        assert table == (1 if n >= 64 else 0), (what, table)      # approach_local_tab_k from 64 frames on
                    # a counting launch with the approach kernels tallying their own steps
                    monkeypatch.setenv("VP_COUNT_APPROACH", "1")
                    try:
                        vp.enable_counters(True)
                        vp.read_counters(reset=True)
                        buf.reset()
                        vp.render_frames(buf.ptr, 0, n, P)
                        k = vp.read_counters()
                        got = buf.download()
                    finally:
                        vp.enable_counters(False)
                        monkeypatch.delenv("VP_COUNT_APPROACH")
                    assert got.tobytes() == acc.tobytes(), (what, "counting launch")
                    for q in COUNTERS:
                        assert k[q] == cnt[q], (what, q, k[q], cnt[q])
        finally:
            buf.free()
