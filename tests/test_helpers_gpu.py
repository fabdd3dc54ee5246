"""The integrator's elementary helpers (vp_math.h through vp_test_math, include/volpath.h) against float64, in both arithmetic modes.

Every reference is float64 arithmetic on the float32 input (for the turns form: sin(2 pi t) of the float32 t).  Each bound has the
shape of the operation's error, not a flat ulp count, and the reason is written at the assert.  The exact bounds are at least as
tight as test_oracle_cpu.py::test_math_accuracy; the fast bounds were measured once on an MI355X and carry at most 4x margin
(the measured figure is written next to each).  The helpers the fast mode does not substitute are bit-identical between modes.
A fast case runs in a context of its own: the session's `vp` context keeps the exact default."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32 = np.float32
TINY = float(np.finfo(np.float32).tiny)      # 2^-126
EPS = 2.0 ** -24


@pytest.fixture(params=["exact", "fast"])
def mode(request, vp):
    c = vp.Context(0)
    try:
        with c:
            vp.set_arithmetic(vp.ARITH_FAST if request.param == "fast" else vp.ARITH_EXACT)
            yield request.param
    finally:
        c.destroy()


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _nb(x):
    """x and its float32 neighbours"""
    x = _f32(x)
    return np.concatenate([np.nextafter(x, F32(-np.inf)), x, np.nextafter(x, F32(np.inf))])


def _ulp(ref):
    """the spacing of float32 at the float64 reference (the ulp a correctly rounded result is judged in)"""
    return np.abs(np.spacing(np.abs(ref).astype(np.float32))).astype(np.float64)


def log_inputs():
    rng = np.random.default_rng(11)
    unit = _f32(rng.random(100000))
    unit = unit[unit > 0]
    edges = _f32([EPS, 1.0 - EPS, 1.0, TINY, 0.5, 2.0 ** -100])
    wide = _f32(2.0 ** rng.uniform(-126.0, 100.0, 100000))
    near1 = _f32(1.0 + rng.uniform(-1e-3, 1e-3, 20000))
    return np.concatenate([unit, edges, wide, near1, _f32([2.0 ** 100])])


def exp_inputs():
    rng = np.random.default_rng(12)
    x = _f32(rng.uniform(-87.0, 0.0, 100000))
    small = _f32(-(10.0 ** rng.uniform(-8, 0, 20000)))
    return np.concatenate([x, small, _f32([0.0, -0.0, -87.0, 88.0, -1.0, -50.0])])


def normal_inputs(lo=-126.0, hi=127.0, seed=13, n=100000):
    """log-spaced normals with random mantissas, both signs"""
    rng = np.random.default_rng(seed)
    return _f32(2.0 ** rng.uniform(lo, hi, n))


def turns_inputs():
    rng = np.random.default_rng(14)
    return np.concatenate([_f32(rng.random(100000)), _nb([0.25, 0.5, 0.75, 1.0]), _f32([0.0, 2.0 ** -30, 1e-6])])


# ---- logf_ ---------------------------------------------------------------------------------------------------------------------
def test_logf(vp, mode):
    x = log_inputs()
    got = vp.test_math(0, x).astype(np.float64)
    ref = np.log(x.astype(np.float64))
    assert vp.test_math(0, _f32([0.0, -0.0])).tolist() == [-np.inf, -np.inf]   # log(0) = -inf: -log of a zero draw is +inf
    err = np.abs(got - ref)
    if mode == "exact":
        # Cephes logf: under 1 ulp of the result everywhere on [2^-126, 2^100] (test_math_accuracy: < 1 ulp on (0,1))
        assert (err / _ulp(ref)).max() < 1.0, float((err / _ulp(ref)).max())
        return
    # fast: v_log_f32 (log2) times ln 2 rounded.  Relative to |log x| where that is not small, but v_log_f32 is accurate in absolute
    # terms near x = 1 (where log2 x -> 0 and a relative bound means nothing): an absolute term plus a relative one.
    # measured on the MI355X: absolute 1.13e-10 (|log x| < 1e-3), relative 1.61e-7 (|log x| >= 1e-3) -- each term 4x
    tol = 4.5e-10 + 6.4e-7 * np.abs(ref)
    assert (err <= tol).all(), float((err / tol).max())


# ---- expf_ ---------------------------------------------------------------------------------------------------------------------
def test_expf(vp, mode):
    x = exp_inputs()
    got = vp.test_math(1, x).astype(np.float64)
    ref = np.exp(x.astype(np.float64))
    rel = np.abs(got / ref - 1)
    # the guards, in both modes: below -87 the result is 0, above 88 +inf, and -87 / 88 themselves are computed
    g = vp.test_math(1, _f32([-87.0, np.nextafter(F32(-87.0), F32(-np.inf)), -100.0, -np.inf, 88.0, np.nextafter(F32(88.0), F32(np.inf)), np.inf]))
    assert g[0] > 0 and g[1] == 0 and g[2] == 0 and g[3] == 0, g
    assert np.isfinite(g[4]) and abs(g[4] / np.exp(88.0) - 1) < 1e-5 and g[5] == np.inf and g[6] == np.inf, g
    assert abs(g[0] / np.exp(-87.0) - 1) < 1e-5, g
    assert vp.test_math(1, _f32([0.0, -0.0])).tolist() == [1.0, 1.0]
    if mode == "exact":
        # Cephes expf: under 1.5 ulp (as test_math_accuracy, now over all of [-87, 0])
        assert (np.abs(got - ref) / _ulp(ref)).max() < 1.5
        return
    # fast: x * log2e is rounded first (relative 2^-24, an ABSOLUTE error of |x| log2e 2^-24 in the exponent), so the result's
    # relative error grows as ln2 * |x * log2e| * 2^-24 = |x| * 6e-8, on top of v_exp_f32's own ~1 ulp.
    # measured on the MI355X: max rel / (1 + |x|) = 7.1e-8 (7.3e-8 |x| for |x| > 10, 8.5e-8 for |x| < 1) -- bound 3.4x
    tol = 2.4e-7 * (1.0 + np.abs(x.astype(np.float64)))
    assert (rel <= tol).all(), float((rel / tol).max())


# ---- rcp_, sqrt_, rsqrt_ -------------------------------------------------------------------------------------------------------
def test_rcp_sqrt_rsqrt(vp, mode):
    xr = normal_inputs(-125.0, 125.0)            # 1/x normal as well
    xr[::2] = -xr[::2]
    xs = normal_inputs(-126.0, 127.0, seed=15)
    r = vp.test_math(7, xr).astype(np.float64)
    s = vp.test_math(8, xs).astype(np.float64)
    q = vp.test_math(9, xs).astype(np.float64)
    rr = 1.0 / xr.astype(np.float64)
    rs = np.sqrt(xs.astype(np.float64))
    rq = 1.0 / rs
    if mode == "exact":
        # IEEE: 1/x and sqrt correctly rounded (numpy's float32 operations are the same); 1/sqrt rounds twice -- half an ulp of the
        # root (relative 2^-24, half of it in the reciprocal) and half an ulp of the quotient: < 1.5 ulp (the oracle: 1.47)
        assert np.array_equal(r, (F32(1.0) / xr).astype(np.float64))
        assert np.array_equal(s, np.sqrt(xs).astype(np.float64))
        assert (np.abs(q - rq) / _ulp(rq)).max() < 1.5
    else:
        # v_rcp_f32 / v_sqrt_f32 / v_rsq_f32: one instruction each, about an ulp of the result.
        # measured on the MI355X: 0.87 (rcp), 0.90 (sqrt), 0.81 (rsqrt) ulp -- bound 3.2 ulp (3.6x to 3.95x)
        assert (np.abs(r - rr) / _ulp(rr)).max() <= 3.2, float((np.abs(r - rr) / _ulp(rr)).max())
        assert (np.abs(s - rs) / _ulp(rs)).max() <= 3.2, float((np.abs(s - rs) / _ulp(rs)).max())
        assert (np.abs(q - rq) / _ulp(rq)).max() <= 3.2, float((np.abs(q - rq) / _ulp(rq)).max())


def test_denormal_inputs(vp, mode):
    """the hardware instructions flush denormal inputs (read as +0).  The inputs lie above 1/FLT_MAX, where
    the IEEE reciprocal of a denormal is still finite."""
    d = _f32([3.0e-39, 5.0e-39, 1.0e-38, 1.1e-38])
    assert (np.abs(d) < TINY).all() and (d > 0).all()
    r, s, q = vp.test_math(7, d), vp.test_math(8, d), vp.test_math(9, d)
    if mode == "exact":
        assert np.isfinite(r).all() and np.array_equal(r, F32(1.0) / d)
        assert np.array_equal(s, np.sqrt(d)) and np.isfinite(q).all()
    else:
        assert (r == np.inf).all(), r          # the input is read as +0: 1/0
        assert (s == 0).all(), s
        assert (q == np.inf).all(), q


# ---- sincos_turns_ -------------------------------------------------------------------------------------------------------------
def test_sincos_turns(vp, mode):
    t = turns_inputs()
    sn, cs = vp.test_math(10, t).astype(np.float64), vp.test_math(11, t).astype(np.float64)
    a = 2.0 * np.pi * t.astype(np.float64)
    es, ec = np.abs(sn - np.sin(a)), np.abs(cs - np.cos(a))
    if mode == "exact":
        # sincosf_ of fl(fl(2 pi) * t): the argument carries an absolute error up to 2 pi * 2^-24 * t (the product's rounding and
        # that of fl(2 pi)), i.e. < 4.2e-7 at t = 1, plus the polynomial's 2e-7 (test_math_accuracy): absolute 2e-7 + 4.2e-7 t (the oracle, bit for bit this helper: 0.73 of it)
        tol = 2e-7 + 4.2e-7 * t.astype(np.float64)
        assert (es <= tol).all() and (ec <= tol).all(), (float((es / tol).max()), float((ec / tol).max()))
    else:
        # v_sin_f32 / v_cos_f32 take the turns themselves (no 2 pi product to round): an absolute error, flat over [0, 1].
        # measured on the MI355X: 1.23e-7 (sin), 1.22e-7 (cos) -- bound 4.8e-7 (3.9x)
        assert es.max() <= 4.8e-7 and ec.max() <= 4.8e-7, (es.max(), ec.max())
    # the quarter turns: within either mode's bound at t = 1 (exact: 6.2e-7), and the signs right
    q = vp.test_math(10, _f32([0.0, 0.25, 0.5, 0.75, 1.0])), vp.test_math(11, _f32([0.0, 0.25, 0.5, 0.75, 1.0]))
    assert np.allclose(q[0], [0, 1, 0, -1, 0], atol=6.2e-7) and np.allclose(q[1], [1, 0, -1, 0, 1], atol=6.2e-7), q
    assert q[0][1] > 0 and q[0][3] < 0 and q[1][0] > 0 and q[1][2] < 0


# ---- the helpers the fast mode does not substitute -----------------------------------------------------------------------------
def _exact_only_inputs():
    rng = np.random.default_rng(16)
    u = _f32(rng.random(100000))
    xa = _f32(u * F32(6.2831855))
    xa = np.concatenate([xa, _f32([0.0, np.pi / 2, np.pi, 3 * np.pi / 2, 2 * np.pi])])
    xc = np.concatenate([_f32(u * 2 - 1), _nb([-1.0, 1.0]), _f32([0.0, 0.5, -0.5])])
    big = _f32(10.0 ** rng.uniform(-3, 38, 20000)) * np.where(rng.random(20000) < 0.5, F32(-1), F32(1))
    xt = np.concatenate([_f32(np.tan((u - 0.5) * 3.1)), big, _f32([0.0, -0.0, 1e-30, -1e-30, 1.0, -1.0])])
    return xa, xc, xt


def test_sincos_acos_atan_exact_and_unchanged_by_the_mode(vp, mode):
    xa, xc, xt = _exact_only_inputs()
    outs = {w: vp.test_math(w, x) for w, x in ((2, xa), (3, xa), (4, xc), (5, xt))}
    if mode == "fast":
        # not substituted by the fast mode: the same bits as the exact helpers (the same context, switched to exact for the call)
        vp.set_arithmetic(vp.ARITH_EXACT)
        try:
            for w, x in ((2, xa), (3, xa), (4, xc), (5, xt)):
                assert np.array_equal(vp.test_math(w, x), outs[w], equal_nan=True), w
        finally:
            vp.set_arithmetic(vp.ARITH_FAST)
    a64 = xa.astype(np.float64)
    # sincosf_ on [0, 2 pi]: 2e-7 absolute (test_math_accuracy)
    assert np.abs(outs[2] - np.sin(a64)).max() < 2e-7 and np.abs(outs[3] - np.cos(a64)).max() < 2e-7
    # acosf_ on [-1, 1]: < 2 ulp; |x| > 1 is clamped to +-1 (acos(1 + e) = 0, acos(-1 - e) = pi in binary32)
    rc = np.arccos(np.clip(xc.astype(np.float64), -1, 1))
    inside = np.abs(xc) <= 1
    assert (np.abs(outs[4][inside] - rc[inside]) / _ulp(rc[inside])).max() < 2.0
    assert np.array_equal(vp.test_math(4, _f32([1.0, np.nextafter(F32(1), F32(2)), 2.0, -1.0, np.nextafter(F32(-1), F32(-2)), -2.0])),
                          _f32([0.0, 0.0, 0.0, np.pi, np.pi, np.pi]))
    # atanf_ over the whole line: < 4 ulp (test_math_accuracy); +-inf -> +-pi/2, NaN -> 0, denormals and tiny values: x itself
    rt = np.arctan(xt.astype(np.float64))
    assert (np.abs(outs[5] - rt) / _ulp(rt)).max() < 4.0
    special = vp.test_math(5, _f32([np.inf, -np.inf, np.nan, 1e-40, -1e-40, 1e-20]))
    assert special.tolist()[:3] == [F32(np.pi / 2), -F32(np.pi / 2), 0.0]
    assert np.array_equal(special[3:], _f32([1e-40, -1e-40, 1e-20]))
