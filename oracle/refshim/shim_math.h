/* shim_math.h -- TEST INFRASTRUCTURE (oracle/refshim).  The arithmetic contract, and nothing else.
 *
 * The reference calls CUDA's device libm, whose bits no other platform reproduces.  The project pins each elementary function
 * to one sequence of IEEE-754 binary32 operations (oracle/vpo_math.h; the HIP product carries its own copy).  This header makes
 * the reference's kernel file, compiled for the CPU, call those same sequences, so that every remaining difference between that
 * build and oracle/vp_oracle.c is a difference in control flow, order of draws or order of operations.
 *
 * Include it AFTER every standard header: it renames the unsuffixed functions with macros.
 *   float overloads  -> vpo_logf, vpo_expf, vpo_sincosf, sqrtf; pow(x, 1.5f) = x * sqrtf(x), any other exponent
 *                       exp(log(x) * y) on the same kernels, 0 for x <= 0 (vp_oracle.c's gamma rule)
 *   double overloads -> libm (the camera's tan(fovx * 0.00872664626) is double in the reference and is not touched)
 */
#ifndef REFSHIM_SHIM_MATH_H
#define REFSHIM_SHIM_MATH_H

#include <math.h>

#include "../vpo_math.h"

static inline float shim_powf(float x, float y)
{
    if (y == 1.5f) return vpo_pow15f(x);
    if (x <= 0.0f) return 0.0f;
    return vpo_expf(vpo_logf(x) * y);
}
static inline float shim_log(float x) { return vpo_logf(x); }
static inline float shim_exp(float x) { return vpo_expf(x); }
static inline float shim_sin(float x) { float s, c; vpo_sincosf(x, &s, &c); return s; }
static inline float shim_cos(float x) { float s, c; vpo_sincosf(x, &s, &c); return c; }
static inline float shim_sqrt(float x) { return sqrtf(x); }
static inline float shim_pow(float x, float y) { return shim_powf(x, y); }

static inline double shim_log(double x) { return ::log(x); }
static inline double shim_exp(double x) { return ::exp(x); }
static inline double shim_sin(double x) { return ::sin(x); }
static inline double shim_cos(double x) { return ::cos(x); }
static inline double shim_sqrt(double x) { return ::sqrt(x); }
static inline double shim_pow(double x, double y) { return ::pow(x, y); }

#define log shim_log
#define exp shim_exp
#define sin shim_sin
#define cos shim_cos
#define sqrt shim_sqrt
#define pow shim_pow

#define logf vpo_logf
#define expf vpo_expf
#define atanf vpo_atanf
#define acosf vpo_acosf
#define powf shim_powf

#endif
