// vp_math.h -- deterministic binary32 elementary functions for the gfx950 kernels.
//
// The integrator's libm calls (reference: logf kernel.cu:2085, powf :602, sinf/cosf :596,
// acosf/atanf :884-891, expf :2186) are pinned to explicit sequences of IEEE add/mul/div/sqrt/fma
// so that results do not depend on which vendor libm (CUDA, ocml, glibc) evaluates them; the
// parity tests compare this path bit for bit against an independent CPU statement of the same
// sequences.  Cephes single-precision kernels (Moshier).  Compile with -ffp-contract=off.
//
// VP_ARITH_FAST (vp_kernels_fast.hip only; include/volpath.h vp_set_arithmetic): the integrator's logarithm, exponential,
// divides, reciprocals, square roots and the phase function's sine and cosine become the hardware's single instructions
// (v_log_f32, v_exp_f32, v_rcp_f32, v_sqrt_f32, v_rsq_f32, v_sin_f32 / v_cos_f32), each substitution written out here -- the
// flags stay those of the exact build (no contraction, no compiler fast math), so every instance of a fast kernel computes the
// same bits for the same sample.  The helpers then live in an inline namespace of their own: the two translation units never
// share a definition of the same name.  Without VP_ARITH_FAST every helper is the expression the integrator has always used.
#pragma once
#include <hip/hip_runtime.h>

#ifdef VP_ARITH_FAST
#define VP_ARITH_BEGIN inline namespace arith_fast {
#define VP_ARITH_END }
#else
#define VP_ARITH_BEGIN
#define VP_ARITH_END
#endif

namespace vp
{
VP_ARITH_BEGIN
__device__ __forceinline__ float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ float u2f(unsigned u) { return __uint_as_float(u); }
__device__ __forceinline__ unsigned f2u(float f) { return __float_as_uint(f); }

// The logarithm's chain on [2^-126, inf) (Cephes logf), without the answer for 0: logf_ and logf_pos_ below.
// The mantissa is folded into (sqrt(2)/2, sqrt(2)] without a select: adding 2^23 - 0x3504f4 to the bit pattern carries into the
// exponent field exactly when the mantissa field exceeds that of fl(sqrt 2) = 0x3fb504f3.  The exponent's bias goes into the same
// constant (0x004afb0c - 0x3f800000 mod 2^32: a multiple of 2^23 less, so the low 23 bits are the same) and an arithmetic shift
// reads the unbiased exponent off: the same integer as (iy >> 23) - 127 of the unfolded sum for every pattern below 0xbf3504f4 --
// all non-negative floats, +inf and the positive NaNs (tests/test_approach_step_cpu.py pins the range; vp_test_log_forms compares
// the chain with the unfolded one on every pattern of it).
__device__ __forceinline__ float logf_chain_(float x)
{
    unsigned ix = f2u(x);
    unsigned iy = ix + 0xc0cafb0cu;
    int      e  = (int)iy >> 23;
    float    m  = u2f((iy & 0x007fffffu) + 0x3f3504f4u);
    float    r  = m - 1.0f;
    float z     = r * r;
    float p     = 7.0376836292E-2f;
    p           = fma_(p, r, -1.1514610310E-1f);
    p           = fma_(p, r, 1.1676998740E-1f);
    p           = fma_(p, r, -1.2420140846E-1f);
    p           = fma_(p, r, 1.4249322787E-1f);
    p           = fma_(p, r, -1.6668057665E-1f);
    p           = fma_(p, r, 2.0000714765E-1f);
    p           = fma_(p, r, -2.4999993993E-1f);
    p           = fma_(p, r, 3.3333331174E-1f);
    float fe    = (float)e;
    float y     = (r * z) * p;
    y           = fma_(fe, -2.12194440e-4f, y);
    y           = fma_(z, -0.5f, y);
    float res   = r + y;
    return fma_(fe, 0.693359375f, res);
}

// natural logarithm on {0} U [2^-126, inf); log(0) = -inf
__device__ __forceinline__ float logf_(float x)
{
#if defined(VP_ARITH_FAST) || defined(VP_EXP_FASTLOG)
    return __builtin_amdgcn_logf(x) * 0.69314718056f;   // v_log_f32 is log2; log(0) = -inf as well
#endif
    const float res = logf_chain_(x);
    return x == 0.0f ? -__builtin_inff() : res;
}

// natural logarithm on [2^-126, inf) ONLY: logf_ without its answer for 0 (a compare and a select less; at 0 the chain returns a
// finite number that means nothing).  For callers that test for 0 themselves: the approach walks (vp_integrator.h approach_walk).
// In the fast arithmetic it is logf_, whose one instruction answers 0 as well.
__device__ __forceinline__ float logf_pos_(float x)
{
#if defined(VP_ARITH_FAST) || defined(VP_EXP_FASTLOG)
    return logf_(x);
#endif
    return logf_chain_(x);
}

// exponential; used on arguments <= 0; results below 2^-126 flush to 0
__device__ __forceinline__ float expf_(float x)
{
    if (x < -87.0f) return 0.0f;
    if (x > 88.0f) return __builtin_inff();
#ifdef VP_ARITH_FAST
    return __builtin_amdgcn_exp2f(x * 1.44269504088896341f);   // v_exp_f32 is 2^x
#endif
    float fn = __builtin_floorf(fma_(x, 1.44269504088896341f, 0.5f));
    float r  = fma_(fn, -0.693359375f, x);
    r        = fma_(fn, 2.12194440e-4f, r);
    float z  = r * r;
    float p  = 1.9875691500E-4f;
    p        = fma_(p, r, 1.3981999507E-3f);
    p        = fma_(p, r, 8.3334519073E-3f);
    p        = fma_(p, r, 4.1665795894E-2f);
    p        = fma_(p, r, 1.6666665459E-1f);
    p        = fma_(p, r, 5.0000001201E-1f);
    float y  = fma_(p, z, r) + 1.0f;
    int   n  = (int)fn;
    return y * u2f((unsigned)(n + 127) << 23);
}

// sine and cosine of an angle in [0, 2*pi]
__device__ __forceinline__ void sincosf_(float a, float& s, float& c)
{
    float fk = __builtin_floorf(fma_(a, 0.636619772367581343f, 0.5f));
    int   k  = (int)fk;
    float r  = fma_(fk, -1.5703125f, a);
    r        = fma_(fk, -4.837512969970703125e-4f, r);
    r        = fma_(fk, -7.54978995489188216e-8f, r);
    float z  = r * r;
    float ps = -1.9515295891E-4f;
    ps       = fma_(ps, z, 8.3321608736E-3f);
    ps       = fma_(ps, z, -1.6666654611E-1f);
    float sn = fma_(ps * z, r, r);
    float pc = 2.443315711809948E-005f;
    pc       = fma_(pc, z, -1.388731625493765E-003f);
    pc       = fma_(pc, z, 4.166664568298827E-002f);
    float cs = fma_(pc * z, z, fma_(z, -0.5f, 1.0f));
    int   q  = k & 3;
    float a0 = (q & 1) ? cs : sn;  // |sin|
    float b0 = (q & 1) ? sn : cs;  // |cos|
    s        = (q & 2) ? -a0 : a0;
    c        = (q == 1 || q == 2) ? -b0 : b0;
}

__device__ __forceinline__ float acosf_(float x)
{
    float ax  = __builtin_fabsf(x);
    ax        = ax > 1.0f ? 1.0f : ax;
    bool  big = ax > 0.5f;
    float z   = big ? 0.5f * (1.0f - ax) : ax * ax;
    float t   = big ? __builtin_sqrtf(z) : ax;
    float p   = 4.2163199048E-2f;
    p         = fma_(p, z, 2.4181311049E-2f);
    p         = fma_(p, z, 4.5470025998E-2f);
    p         = fma_(p, z, 7.4953002686E-2f);
    p         = fma_(p, z, 1.6666752422E-1f);
    float as  = fma_(p * z, t, t);
    if (big)
    {
        float r = 2.0f * as;
        return x < 0.0f ? 3.14159265358979323846f - r : r;
    }
    return x < 0.0f ? 1.57079632679489661923f + as : 1.57079632679489661923f - as;
}

__device__ __forceinline__ float atanf_(float x)
{
    if (x != x) return 0.0f;
    float t = __builtin_fabsf(x);
    float y;
    if (t > 2.414213562373095f) { y = 1.57079632679489661923f; t = -1.0f / t; }
    else if (t > 0.4142135623730950f) { y = 0.785398163397448309616f; t = (t - 1.0f) / (t + 1.0f); }
    else y = 0.0f;
    float z = t * t;
    float p = 8.05374449538e-2f;
    p       = fma_(p, z, -1.38776856032E-1f);
    p       = fma_(p, z, 1.99777106478E-1f);
    p       = fma_(p, z, -3.33329491539E-1f);
    y       = y + fma_(p * z, t, t);
    return x < 0.0f ? -y : y;
}

// the quotient of the collision weights (experiment hook: VP_EXP_FASTDIV replaces the IEEE divide by v_rcp_f32)
__device__ __forceinline__ float wdiv_(float a, float b)
{
#if defined(VP_ARITH_FAST) || defined(VP_EXP_FASTDIV)
    return a * __builtin_amdgcn_rcpf(b);
#else
    return a / b;
#endif
}

// the integrator's other quotients, reciprocals and roots
#ifdef VP_ARITH_FAST
__device__ __forceinline__ float div_(float a, float b) { return a * __builtin_amdgcn_rcpf(b); }
__device__ __forceinline__ float rcp_(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float sqrt_(float x) { return __builtin_amdgcn_sqrtf(x); }
__device__ __forceinline__ float rsqrt_(float x) { return __builtin_amdgcn_rsqf(x); }
// (the in-range forms below belong to the exact mode: here they are the single instructions)
__device__ __forceinline__ float sqrt_inrange_(float x) { return __builtin_amdgcn_sqrtf(x); }
__device__ __forceinline__ float rsqrt_unit_(float x) { return __builtin_amdgcn_rsqf(x); }
#else
__device__ __forceinline__ float div_(float a, float b) { return a / b; }
__device__ __forceinline__ float rcp_(float x) { return 1.0f / x; }
__device__ __forceinline__ float sqrt_(float x) { return __builtin_sqrtf(x); }
__device__ __forceinline__ float rsqrt_(float x) { return 1.0f / __builtin_sqrtf(x); }
// The same root and reciprocal root for operands that are in range BY CONSTRUCTION at the call site (each site derives its range):
// the compiler's own expansion of __builtin_sqrtf and of 1.0f / s without the steps that are identities there.  The square root
// of binary32 is v_sqrt_f32 (1 ulp) and two one-ulp corrections, each decided by the sign of an exact fma residual; around them
// the compiler scales operands below 2^-96 by 2^32 and passes 0, inf and NaN through a class test -- seven of sixteen instructions.
// The quotient 1 / s is v_rcp_f32, one Newton step on the reciprocal, q = 1 * r, two residual corrections of q; around them two
// v_div_scale (identities unless s or 1 / s is near the ends of the exponent range), v_div_fmas (an fma when nothing was scaled)
// and v_div_fixup (passes the quotient through unless an operand is 0, inf or NaN).  A correctly rounded result is unique, so the
// shortened forms return the bits of the general ones wherever their preconditions hold; vp_test_roots (include/volpath.h)
// compares the two on every bit pattern of the stated ranges.
// PRECONDITION: x == 0, or 2^-24 <= x <= 2.  (x = 0: v_sqrt_f32 gives 0; the lower neighbour's pattern is a NaN, whose residual
// compares false; the upper neighbour's residual is fma(-2^-149, 0, 0) = 0, not positive: 0 is returned.)
__device__ __forceinline__ float sqrt_inrange_(float x)
{
    float       s  = __builtin_amdgcn_sqrtf(x);
    const float dn = u2f(f2u(s) - 1u), up = u2f(f2u(s) + 1u);
    const float rd = fma_(-dn, s, x), ru = fma_(-up, s, x);
    s = (rd <= 0.0f) ? dn : s;
    s = (ru > 0.0f) ? up : s;
    return s;
}
// PRECONDITION: 2^-8 <= x <= 2, so the root s lies in [2^-4, 1.42] and 1 / s in [0.70, 16].
__device__ __forceinline__ float rsqrt_unit_(float x)
{
    const float s = sqrt_inrange_(x);
    float       r = __builtin_amdgcn_rcpf(s);
    r             = fma_(fma_(-s, r, 1.0f), r, r);
    float q       = r;                                // the numerator 1 times r
    q             = fma_(fma_(-s, q, 1.0f), r, q);
    return fma_(fma_(-s, q, 1.0f), r, q);
}
#endif

// sine and cosine of 2 pi t, t in [0, 1]: the azimuth of the phase-function sample (v_sin_f32 / v_cos_f32 take revolutions)
__device__ __forceinline__ void sincos_turns_(float t, float& s, float& c)
{
#ifdef VP_ARITH_FAST
    s = __builtin_amdgcn_sinf(t);
    c = __builtin_amdgcn_cosf(t);
#else
    sincosf_((2.0f * 3.14159265358979323846f) * t, s, c);
#endif
}

__device__ __forceinline__ float pow15f_(float x) { return x * sqrt_(x); }
VP_ARITH_END
}  // namespace vp
