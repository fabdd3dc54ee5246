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
// Built: the counter-based streams (Philox2x32-10 and -7), spectral tracking, passive environment, the global-majorant and
// decomposition estimators, uchar, float and binary16 volumes, LDS forms 0/1/2, achromatic and chromatic media, the look-ahead's CANCEL
// instances.  Not built (vp_render.cpp refuses them with VP_E_STATE): the sampler.h stream, the bounded estimator, MIS, scalar and
// multi-channel tracking, work counters.
#define VP_ARITH_FAST 1

#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

#include "vp_device.h"
#include "vp_kernels.h"

namespace vp
{
namespace fast
{
#include "vp_integrator.h"
#include "vp_test_kernels.h"

template <int EST, class RNG, bool QUANT, int LDSB, bool ACH, bool HALF>
static void launch_render_t(const SceneDev& S, const LaunchDev& L, int blocks, hipStream_t st)
{
    const dim3 g(blocks), b(LDSB == 1 ? VP_BLOCK_LDS : VP_BLOCK);
    if constexpr (LDSB == 2)
        hipLaunchKernelGGL((render_k<EST, RNG, QUANT, false, 2, ACH, false, 0, false, false, HALF>), g, b, 0, st, S, L);   // timed launches only
    else if (L.cancel)
        hipLaunchKernelGGL((render_k<EST, RNG, QUANT, false, LDSB, ACH, false, 0, false, true, HALF>), g, b, 0, st, S, L);
    else
        hipLaunchKernelGGL((render_k<EST, RNG, QUANT, false, LDSB, ACH, false, 0, false, false, HALF>), g, b, 0, st, S, L);
}
template <int EST, class RNG, bool QUANT, int LDSB, bool HALF = false>
static void launch_render_a(const SceneDev& S, const LaunchDev& L, bool ach, int blocks, hipStream_t st)
{
    if (ach) launch_render_t<EST, RNG, QUANT, LDSB, true, HALF>(S, L, blocks, st);
    else launch_render_t<EST, RNG, QUANT, LDSB, false, HALF>(S, L, blocks, st);
}
template <class RNG>
static void launch_render_r(const SceneDev& S, const LaunchDev& L, int est, bool quant, bool half, int lds_form, bool ach, int blocks, hipStream_t st)
{
    if (est == EST_GLOBAL)
    {
#ifndef VP_DEV_BUILD
        if (half) { launch_render_a<EST_GLOBAL, RNG, false, 0, true>(S, L, ach, blocks, st); return; }
        if (!quant) { launch_render_a<EST_GLOBAL, RNG, false, 0>(S, L, ach, blocks, st); return; }
#endif
        launch_render_a<EST_GLOBAL, RNG, true, 0>(S, L, ach, blocks, st);
        return;
    }
#ifndef VP_DEV_BUILD
    if (half) { launch_render_a<EST_DECOMP, RNG, false, 0, true>(S, L, ach, blocks, st); return; }
    if (!quant) { launch_render_a<EST_DECOMP, RNG, false, 0>(S, L, ach, blocks, st); return; }
#endif
    // (the same choice of LDS form as vp_kernels.hip launch_render: the compact table for timed launches only)
    if (lds_form == 2 && !L.cancel) launch_render_a<EST_DECOMP, RNG, true, 2>(S, L, ach, blocks, st);
    else if (lds_form != 0) launch_render_a<EST_DECOMP, RNG, true, 1>(S, L, ach, blocks, st);
    else launch_render_a<EST_DECOMP, RNG, true, 0>(S, L, ach, blocks, st);
}
}  // namespace fast

void launch_render_fast(const SceneDev& S, const LaunchDev& L, int est, int rng, bool quant, bool half, bool count, int lds_form, bool mis, int trk,
                        int blocks, hipStream_t st)
{
    if (count || mis || trk || (est != EST_GLOBAL && est != EST_DECOMP) || (rng != RNG_PHILOX && rng != RNG_PHILOX7))
    {
        fprintf(stderr, "volpath_hip: the fast arithmetic mode has no kernel for this configuration\n");
        abort();
    }
#ifdef VP_DEV_BUILD
    if (!quant) { fprintf(stderr, "volpath_hip DEV build: this kernel variant is not compiled\n"); abort(); }
#endif
    const ParamDev& P = L.P;
    const bool ach = P.sigma_t[0] == P.sigma_t[1] && P.sigma_t[1] == P.sigma_t[2] && P.albedo[0] == P.albedo[1] && P.albedo[1] == P.albedo[2];
    if (rng == RNG_PHILOX7) fast::launch_render_r<RngPhilox7>(S, L, est, quant, half, lds_form, ach, blocks, st);
    else fast::launch_render_r<RngPhilox>(S, L, est, quant, half, lds_form, ach, blocks, st);
}

// light_identity_k in this arithmetic (global majorant: the host lets approach_k skip the walk's null collisions only where this says
// that the fast render_k would leave a throughput of 1 as it is -- else the walk is the integrator's, in staged and single-frame
// launches alike)
void launch_light_identity_fast(const ParamDev& P, bool local, const unsigned* mask, unsigned* flag, hipStream_t st)
{
    hipLaunchKernelGGL(fast::light_identity_k, dim3(1), dim3(256), 0, st, P, local ? 1 : 0, mask, flag);
}

void launch_approach_fast(const SceneDev& S, const LaunchDev& L, int est, int rng, bool quant, hipStream_t st)
{
    if ((est != EST_GLOBAL && est != EST_DECOMP) || (rng != RNG_PHILOX && rng != RNG_PHILOX7))
    {
        fprintf(stderr, "volpath_hip: the fast arithmetic mode has no approach kernel for this configuration\n");
        abort();
    }
    // (the grid and the choice of kernel: vp_kernels.hip launch_approach)
    const unsigned sh = L.approach_fshift, spb = 256u >> sh;
    const dim3 grid((L.nslots + spb - 1u) / spb, ((unsigned)L.nframes + (1u << sh) - 1u) >> sh);
    const bool p7 = rng == RNG_PHILOX7;
    if (est == EST_GLOBAL)
    {
        if (p7) hipLaunchKernelGGL(fast::approach_k<RngPhilox7>, grid, dim3(256), 0, st, S, L);
        else hipLaunchKernelGGL(fast::approach_k<RngPhilox>, grid, dim3(256), 0, st, S, L);
    }
    else if (quant && L.seg_table && sh == 6u)
    {
        if (p7) hipLaunchKernelGGL(fast::approach_local_tab_k<RngPhilox7>, grid, dim3(256), 0, st, S, L);
        else hipLaunchKernelGGL(fast::approach_local_tab_k<RngPhilox>, grid, dim3(256), 0, st, S, L);
    }
    else if (quant)
    {
        if (p7) hipLaunchKernelGGL((fast::approach_local_k<RngPhilox7, true>), grid, dim3(256), 0, st, S, L);
        else hipLaunchKernelGGL((fast::approach_local_k<RngPhilox, true>), grid, dim3(256), 0, st, S, L);
    }
    else
    {
#ifndef VP_DEV_BUILD
        if (p7) hipLaunchKernelGGL((fast::approach_local_k<RngPhilox7, false>), grid, dim3(256), 0, st, S, L);
        else hipLaunchKernelGGL((fast::approach_local_k<RngPhilox, false>), grid, dim3(256), 0, st, S, L);
#else
        fprintf(stderr, "volpath_hip DEV build: this kernel variant is not compiled\n");
        abort();
#endif
    }
}

// the test hooks in this arithmetic (vp_test_kernels.h; vp_context.cpp vp_test_math / vp_test_hg in a fast context)
void launch_test_hg_fast(const float* g, const float* r0, const float* r1, const float* nrm, const float* cosq, float* dir, float* ev, int n, hipStream_t st)
{
    hipLaunchKernelGGL(fast::test_hg_k, dim3((n + 255) / 256), dim3(256), 0, st, g, r0, r1, nrm, cosq, dir, ev, n);
}
void launch_test_math_fast(int which, const float* in, float* out, int n, hipStream_t st)
{
    hipLaunchKernelGGL(fast::test_math_k, dim3((n + 255) / 256), dim3(256), 0, st, which, in, out, n);
}
}  // namespace vp
