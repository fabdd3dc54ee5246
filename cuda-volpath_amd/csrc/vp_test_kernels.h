// vp_test_kernels.h -- the test hooks of the integrator's arithmetic: vp_test_math (test_math_k) and vp_test_hg (test_hg_k).
// Included INSIDE a namespace by both translation units, like vp_integrator.h: vp_kernels.hip (namespace vp, the exact helpers) and
// vp_kernels_fast.hip (namespace vp::fast, VP_ARITH_FAST).  vp_context.cpp launches the pair of the context's arithmetic mode, so
// the hooks test the helpers the context's renders run.

// the phase-function block of the integrator (kernel.cu:2301-2303 with :557-598) and HGPhaseFunction::evaluate (:600-603)
__global__ void test_hg_k(const float* g, const float* r0, const float* r1, const float* nrm, const float* cosq, float* dir, float* ev, int n)
{
    int i = threadIdx.x + blockIdx.x * blockDim.x;
    if (i >= n) return;
    Frame fr(f3{nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]});
    f3    d = normalize(fr.to_world(hg_sample_local(g[i], r0[i], r1[i])));
    dir[3 * i] = d.x; dir[3 * i + 1] = d.y; dir[3 * i + 2] = d.z;
    ev[i] = hg_eval(g[i], cosq[i]);
}
// one helper of vp_math.h per `which` (include/volpath.h vp_test_math; the host refuses codes outside 0..11)
__global__ void test_math_k(int which, const float* in, float* out, int n)
{
    int i = threadIdx.x + blockIdx.x * blockDim.x;
    if (i >= n) return;
    float x = in[i], s, c, r;
    switch (which)
    {
        case 0: r = logf_(x); break;
        case 1: r = expf_(x); break;
        case 2: sincosf_(x, s, c); r = s; break;
        case 3: sincosf_(x, s, c); r = c; break;
        case 4: r = acosf_(x); break;
        case 5: r = atanf_(x); break;
        case 6: r = pow15f_(x); break;
        case 7: r = rcp_(x); break;
        case 8: r = sqrt_(x); break;
        case 9: r = rsqrt_(x); break;
        case 10: sincos_turns_(x, s, c); r = s; break;
        case 11: sincos_turns_(x, s, c); r = c; break;
        default: r = __builtin_nanf(""); break;
    }
    out[i] = r;
}
