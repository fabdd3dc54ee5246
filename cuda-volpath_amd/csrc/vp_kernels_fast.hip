// vp_kernels_fast.hip -- the integrator's kernels in the fast arithmetic mode (VP_ARITH_FAST; include/volpath.h vp_set_arithmetic).
//
// The same render_k and approach kernels as vp_kernels.hip (vp_integrator.h), compiled with vp_math.h's fast helpers: v_log_f32 /
// v_exp_f32 for the logarithm and exponential, v_rcp_f32 for the divides and reciprocals, v_sqrt_f32 / v_rsq_f32 for the roots and
// normalisations, v_sin_f32 / v_cos_f32 for the phase function's azimuth.  The compiler flags are the exact build's (no contraction,
// correctly rounded IEEE divide and sqrt where the code still asks for them): every substitution is explicit, so every instance
// below computes the same bits for the same sample -- LDS forms, look-ahead (CANCEL) instances, achromatic or not -- and a batched,
// staged or sharded render equals a frame-by-frame one in this mode as in the exact one.
//
// What stays exact (vp_kernels.hip alone): every table and certificate the kernels read, the box-missing and light pixel classes
// (miss_fill_k, render_k<LIGHT>), the reduction, scale and gamma; and, inside these kernels, the camera ray and the box tests, whose
// geometry the per-pixel tables are certified on.  What is decided by the arithmetic is decided here: whether a null collision in
// empty space is neutral (light_identity_k below, for the global majorant's approach walk; the kernels' own tests for the exit
// flights and the decomposition walks), so that a staged launch skips exactly what a one-frame launch would compute as a no-op.
//
// Built: what render_built() and approach_built() of vp_dispatch.h say with VP_ARITH_FAST defined -- the counter-based streams
// (Philox2x32-10 and -7), spectral tracking, passive environment, the global-majorant and decomposition estimators, every volume
// format, every LDS form, achromatic and chromatic media, the look-ahead's CANCEL instances.  vp_render.cpp refuses the rest with
// VP_E_STATE (the sampler.h stream, the bounded estimator, MIS, scalar and multi-channel tracking, work counters) before it launches.
#define VP_ARITH_FAST 1

#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <utility>

#include "vp_device.h"
#include "vp_kernels.h"

namespace vp
{
namespace fast
{
#include "vp_integrator.h"
#include "vp_test_kernels.h"

// which render_k instance and which approach kernel a launch runs, and which of them this unit compiles
#include "vp_dispatch.h"
}  // namespace fast

void launch_render_fast(const SceneDev& S, const LaunchDev& L, int est, int rng, bool quant, bool half, bool count, int lds_form, bool mis, int trk,
                        int blocks, hipStream_t st)
{
    fast::dispatch_render(S, L, est, rng, quant, half, count, lds_form, mis, trk, blocks, st);
}

// light_identity_k in this arithmetic (global majorant: the host lets approach_k skip the walk's null collisions only where this says
// that the fast render_k would leave a throughput of 1 as it is -- else the walk is the integrator's, in staged and single-frame
// launches alike)
void launch_light_identity_fast(const ParamDev& P, bool local, const unsigned* mask, unsigned* flag, hipStream_t st)
{
    hipLaunchKernelGGL(fast::light_identity_k, dim3(1), dim3(256), 0, st, P, local ? 1 : 0, mask, flag);
}

void launch_approach_fast(const SceneDev& S, const LaunchDev& L, int est, int rng, bool quant, hipStream_t st) { fast::dispatch_approach(S, L, est, rng, quant, st); }
void census_built_fast(int kind, unsigned char* built, size_t count) { fast::dispatch_census_built(kind, built, count); }

// the test hooks in this arithmetic (vp_test_kernels.h; vp_context.cpp vp_test_math / vp_test_hg in a fast context)
void launch_test_hg_fast(const float* g, const float* r0, const float* r1, const float* nrm, const float* cosq, float* dir, float* ev, int n, hipStream_t st)
{
    hipLaunchKernelGGL(fast::test_hg_k, dim3((n + 255) / 256), dim3(256), 0, st, g, r0, r1, nrm, cosq, dir, ev, n);
}
void launch_test_math_fast(int which, const float* in, float* out, int n, hipStream_t st)
{
    hipLaunchKernelGGL(fast::test_math_k, dim3((n + 255) / 256), dim3(256), 0, st, which, in, out, n);
}
void launch_test_log_forms_fast(int which, unsigned lo, unsigned hi, unsigned long long* mismatches, unsigned* first_bad, hipStream_t st)
{
    hipLaunchKernelGGL(fast::test_log_forms_k, dim3(2048), dim3(256), 0, st, which, lo, hi, mismatches, first_bad);
}
void launch_test_approach_walk_fast(int kind, int n, const float* par, const unsigned* scr, const unsigned* words, unsigned* out_new, unsigned* out_ref,
                                    hipStream_t st)
{
    hipLaunchKernelGGL(fast::test_approach_walk_k, dim3((n + 63) / 64), dim3(64), 0, st, kind, n, par, scr, words, out_new, out_ref);
}
void launch_test_camera_ray_fast(const SceneDev& S, unsigned width, unsigned height, const unsigned* pixels, float* dir, int n, hipStream_t st)
{
    hipLaunchKernelGGL(fast::test_camera_ray_k, dim3((n + 255) / 256), dim3(256), 0, st, S, width, height, pixels, dir, n);
}
void launch_test_sun_start_fast(int n, const float* origin, const float* sun_dir, const float* box, unsigned* out_new, unsigned* out_ref, hipStream_t st)
{
    hipLaunchKernelGGL(fast::test_sun_start_k, dim3((n + 255) / 256), dim3(256), 0, st, n, origin, sun_dir[0], sun_dir[1], sun_dir[2], box, out_new, out_ref);
}
}  // namespace vp
