"""Extreme media, inputs only (no oracle, no product): Param sets at the ends of what the integrators accept, each on an existing
small scene.  The CPU tests (tests/test_extreme_media_cpu.py) hold the oracle to the reference's own kernel code on every one
of them; the GPU tests (tests/test_extreme_media_gpu.py) hold the HIP path to the oracle.

Why these: beside the oracle's straight-line arithmetic the HIP path has forms that are decided by, or argued from, the values of
Param -- the collision-constant rows (div_(0.5, g) infinite for g = 0, rcp_(0) in the last row for g = 1), the in-range roots
behind a clamp that has to turn a NaN into 1, the achromatic instance chosen with == (0.0 == -0.0), the checks that a null
collision in empty space is the identity (sigma_t' = 0, subnormal, a zero channel), and the deferred light sum with throughputs
that die, underflow or grow.  The randomised scenes draw g from [-0.5, 0.95], albedo from [0.3, 1] and sigma_t from [0.2, 1].

The domain (asserted below for every case): every value finite, density >= 0, sigma_t >= 0 without a negative zero, |g| <= 1, and
max(sigma_t) * density * |box diagonal| <= 1e5 (a shadow ray stays inside the 2^20 pairs of its sub-stream).  Outside it the free
flight need not advance (a negative or non-finite majorant, g > 1): termination is not promised there, and nothing here goes there.

A case is its base medium (an ordinary one: the case's NEIGHBOUR, which every test that needs "something else" renders) and the edit
that makes it extreme.  Every number is an exact binary32 value where that matters (the neighbours of 1e-6f are np.nextafter's).
"""
import numpy as np

f32 = np.float32
W, H = 16, 12
FRAMES = (10, 11)               # 10 is the last frame that never reads the optical-depth table, 11 the first that may: one staged launch
GRID = "julia32"
BOX_DIAGONAL = float(np.sqrt(12.0))     # the default +-1 box of a cubic grid
MAJORANT_CAP = 1e5

SWITCH = f32(1e-6)              # hg_sample_local: fabsf(g) > 1e-6f samples Henyey-Greenstein, else the isotropic form
CHROMATIC = dict(albedo=(0.95, 0.8, 0.6), sigma_t=(1.0, 0.7, 0.45), density=120.0)
DENORM_MIN = float(np.nextafter(f32(0.0), f32(1.0)))        # 2^-149


def _c(name, group, edit, base=None, tags=()):
    base = dict(base or {})
    return dict(name=name, group=group, base=base, kw={**base, **edit}, grid=GRID, size=(W, H), frames=FRAMES, tags=tuple(tags))


def _g(name, g, **kw):
    return _c(name, "g", dict(g=float(g)), **kw)


# Measured on the CPU (tests/test_extreme_media_cpu.py::test_case_terminates_within_the_cap prints them with -s): density lookups +
# draws per sample over frames 10 and 11 at 16x12, sampler.h stream, decomposition / global majorant / bounded.  julia_default (the
# default medium on the same scene) 367 / 1599 / 384; a case may do 100 times as much per estimator, the largest ratio is 24:
#   g_one 289 / 1534 / 289           g_minus_one 598 / 2412 / 873       g_0.999 275 / 1536 / 275        g_minus_0.999 583 / 2310 / 709
#   g_switch, g_switch_below, g_minus_switch, g_minus_switch_below, g_1e-7, g_neg_zero (all isotropic) 505 / 2043 / 531
#   g_switch_above 494 / 1968 / 668  g_minus_switch_above 542 / 1902 / 712   g_one_chromatic 152 / 317 / 152
#   albedo_zero, albedo_signed_zero 300 / 1728 / 300    albedo_signed_zero_first 96 / 330 / 96
#   albedo_dead_channel, albedo_amplifying 168 / 633 / 171              albedo_subnormal 1031 / 4828 / 1221
#   sigma_t_zero_channel 734 / 1311 / 767    sigma_t_wide 997 / 2057 / 1021   sigma_t_zero, density_1e-6, density_1e-40 48 / 0.5 / 48
#   density_2e4 3191 / 38970 / 3371  brightness_zero 367 / 1599 / 384   albedo_overflow 361 / 1590 / 381
CASES = [
    # ---- g: both ends, just inside them, and both sides of the |g| > 1e-6f switch
    _g("g_one", 1.0, tags=("g_pm1", "long")),                   # 1 - g g = 0: hg_eval 0 / 0 for cos = 1; the last row's sigma_t' = 0
    _g("g_minus_one", -1.0, tags=("g_pm1", "long", "cap")),     # every scatter turns the path round: the 800-scatter cap
    _g("g_0.999", 0.999),
    _g("g_minus_0.999", -0.999),
    _g("g_switch", SWITCH, tags=("long",)),                                                     # not above: isotropic
    _g("g_switch_below", np.nextafter(SWITCH, f32(0)), tags=("long",)),
    _g("g_switch_above", np.nextafter(SWITCH, f32(1)), tags=("long",)),                       # the first Henyey-Greenstein g
    _g("g_minus_switch", -SWITCH),
    _g("g_minus_switch_below", -np.nextafter(SWITCH, f32(0))),
    _g("g_minus_switch_above", -np.nextafter(SWITCH, f32(1))),
    _g("g_1e-7", f32(1e-7)),
    _g("g_neg_zero", -0.0),                                     # div_(0.5, -0) = -inf in a row nobody may read
    _c("g_one_chromatic", "g", dict(g=1.0), base=CHROMATIC),
    # ---- channels
    _c("albedo_zero", "channel", dict(albedo=(0.0, 0.0, 0.0))),                                # 0 / 0 at the second collision
    _c("albedo_dead_channel", "channel", dict(albedo=(1.0, 1.0, 0.0)), tags=("dead", "long"), base=dict(density=300.0)),
    # one channel's throughput runs through the subnormals (0.02^n: subnormal from n = 23) while the others carry the path on
    _c("albedo_subnormal", "channel", dict(albedo=(0.95, 0.95, 0.02)), base=dict(density=2000.0, g=0.0), tags=("subnormal", "long")),
    _c("albedo_amplifying", "channel", dict(albedo=(1.5, 1.2, 1.0)), base=dict(density=300.0), tags=("amplifying",)),
    # throughputs overflow: 6^n passes 3.4e38, the next collision weight is inf / inf, and the sample is what fmaxf(NaN, 0) leaves
    _c("albedo_overflow", "channel", dict(albedo=(6.0, 6.0, 6.0)), tags=("overflow",)),
    # equal under ==, not in bits: which instance runs is decided by a compare
    _c("albedo_signed_zero", "channel", dict(albedo=(0.0, -0.0, 0.0)), base=dict(sigma_t=(1.0, -0.0 + 1.0, 1.0)), tags=("ach_compare",)),
    _c("albedo_signed_zero_first", "channel", dict(albedo=(-0.0, 0.0, 0.0)), base=dict(sigma_t=(0.5, 0.5, 0.5), density=300.0), tags=("ach_compare",)),
    # ---- sigma_t
    _c("sigma_t_zero_channel", "sigma_t", dict(sigma_t=(1.0, 0.0, 0.5)), base=dict(density=300.0), tags=("long",)),
    _c("sigma_t_wide", "sigma_t", dict(sigma_t=(5.0, 3.0, 0.1)), base=dict(density=100.0)),
    _c("sigma_t_zero", "sigma_t", dict(sigma_t=(0.0, 0.0, 0.0)), tags=("long",)),            # sigma_t' = 0: 0 * inf in the identity checks
    # ---- density
    _c("density_1e-6", "density", dict(density=1e-6), tags=("long",)),
    _c("density_1e-40", "density", dict(density=1e-40), tags=("long",)),        # sigma_t' subnormal, rcp_ overflows to inf
    _c("density_2e4", "density", dict(density=2e4)),
    # ---- brightness
    _c("brightness_zero", "brightness", dict(brightness=0.0)),
]
BY_NAME = {c["name"]: c for c in CASES}
NAMES = [c["name"] for c in CASES]
assert len(BY_NAME) == len(CASES)


def nudged(c):
    """the medium of an `ach_compare` case with the second albedo channel one ulp from its zero: unequal under ==, the chromatic
    instance"""
    a = list(c["kw"]["albedo"])
    a[1] = DENORM_MIN
    return dict(c, name=c["name"] + "_nudged", kw={**c["kw"], "albedo": tuple(a)})


def tagged(tag):
    return [c for c in CASES if tag in c["tags"]]


DEFAULTS = dict(density=800.0, g=0.877, brightness=1.0, albedo=(1.0, 1.0, 1.0), sigma_t=(1.0, 1.0, 1.0))   # make_param's


def full(kw):
    return {**DEFAULTS, **kw}


def check_domain(kw):
    p = full(kw)
    values = np.array([p["density"], p["g"], p["brightness"], *p["albedo"], *p["sigma_t"]], f32)
    assert np.isfinite(values).all(), kw
    st = np.array(p["sigma_t"], f32)
    assert f32(p["density"]) >= 0 and not np.signbit(f32(p["density"])), kw
    assert (st >= 0).all() and not np.signbit(st).any(), kw
    assert abs(f32(p["g"])) <= 1, kw
    assert float(st.max()) * float(f32(p["density"])) * BOX_DIAGONAL <= MAJORANT_CAP, kw


for _case in CASES:
    check_domain(_case["kw"])
    check_domain(_case["base"])
    assert _case["kw"] != _case["base"], _case["name"]
    assert min(_case["frames"]) <= 10 and max(_case["frames"]) >= 11
    if "ach_compare" in _case["tags"]:
        check_domain(nudged(_case)["kw"])
        _p = full(_case["kw"])
        _a, _s = np.array(_p["albedo"], f32), np.array(_p["sigma_t"], f32)
        assert (_a == _a[0]).all() and (_s == _s[0]).all() and len({v.tobytes() for v in _a}) > 1, _case["name"]
assert set(NAMES) >= {"g_one", "g_minus_one"} and len(tagged("long")) == 11


# Frames of the Julia scene at 64x48, g = 1, global-majorant estimator, in which a scatter direction is drawn with a first variate of
# exactly 0: f = (1 - g g) / (1 + g (2 * 0 - 1)) = 0 / 0, and cos(theta) is a NaN before fmaxf(0, fminf(1, .)) makes it 1 (a clamp
# folded into a median would make it 0).  Found by scanning frames with the oracle's counter (vpo_debug_hg_nan_clamp); the
# counter-based stream with the key NAN_CLAMP_KEY.  Keys: the stream modes RNG_SAMPLERH = 0 and RNG_PHILOX7 = 2.
NAN_CLAMP_SIZE = (64, 48)
NAN_CLAMP_KEY = (0x51ED270B, 77)
NAN_CLAMP_FRAMES = {0: (4246, 4339), 2: (1027, 1109)}


# ------------------------------------------------------------------------------------------------------------- restatement
def null_collision_recurrence(sigma_t, density, g, n):
    """vp_get_null_collision_table in numpy binary32, operation by operation (the restatement of
    tests/test_pins_gpu.py::test_null_collision_table_is_the_float32_recurrence, here for media whose answer is not finite): the
    throughput of an unscattered global-majorant path after k null collisions in empty space, from the reference's expressions with
    density +0 (Ps = +0, c = Pn = |s t| + |s t| + |s t|, t *= s * ((c / s') / c))"""
    f = f32
    with np.errstate(all="ignore"):
        st = [f(v) for v in sigma_t]
        s = f(max(f(0), min(f(1), f(-5) * f(0.066666666666666666667))))
        cur = (f(1) - s) * f(density) + s * f(density) * (f(1) - f(g))
        sp = max(st) * cur
        inv = f(1) / sp
        t = f(1)
        ref = np.empty(n, f)
        for k in range(n):
            ref[k] = t
            m = abs(sp * t)
            pn = (m + m) + m
            t = t * (sp * ((inv * pn) / pn))
    return ref


def finite_null_collision_media():
    """(sigma_t, density, g) of the media of the table whose sigma_t' is a normal number (the recurrence stays finite: what
    tests/test_pins_gpu.py::test_null_collision_table_is_the_float32_recurrence asserts of every medium it walks), each once; the
    others -- sigma_t' zero and subnormal -- are walked by tests/test_extreme_media_gpu.py, NaN for NaN"""
    out = []
    for c in CASES:
        p = full(c["kw"])
        m = (tuple(p["sigma_t"]), p["density"], p["g"])
        if f32(max(p["sigma_t"])) * f32(p["density"]) >= np.finfo(f32).tiny and m not in out:
            out.append(m)
    return tuple(out)
