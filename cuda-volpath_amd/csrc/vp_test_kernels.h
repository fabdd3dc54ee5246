// vp_test_kernels.h -- the test hooks of the integrator's arithmetic: vp_test_math (test_math_k), vp_test_hg (test_hg_k),
// vp_test_log_forms (test_log_forms_k), vp_test_approach_walk (test_approach_walk_k), vp_test_sun_start (test_sun_start_k),
// vp_test_camera_ray (test_camera_ray_k) and vp_test_fetch_split (test_fetch_split_k).
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

// ---- vp_test_log_forms, vp_test_approach_walk: the approach walks' step against the forms it had before its instructions were cut
// (profiles/experiments/approach_step.txt).  TEST-ONLY code below: the earlier forms, kept word for word as the reference.

// logf_ as it stood: the exponent's bias taken off after the shift, the answer for 0 selected at the end
__device__ __forceinline__ float logf_ref_(float x)
{
#if defined(VP_ARITH_FAST) || defined(VP_EXP_FASTLOG)
    return __builtin_amdgcn_logf(x) * 0.69314718056f;   // v_log_f32 is log2; log(0) = -inf as well
#endif
    unsigned ix = f2u(x);
    unsigned iy = ix + 0x004afb0cu;
    int      e  = (int)(iy >> 23) - 127;
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
    res         = fma_(fe, 0.693359375f, res);
    return x == 0.0f ? -__builtin_inff() : res;
}
// which = 0: logf_, 1: logf_pos_, against logf_ref_ on every bit pattern in [lo, hi]
__global__ void test_log_forms_k(int which, unsigned lo, unsigned hi, unsigned long long* mismatches, unsigned* first_bad)
{
    const unsigned long long n = (unsigned long long)hi - lo + 1ull;
    unsigned long long bad = 0;
    unsigned           fb  = 0xffffffffu;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * blockDim.x)
    {
        const unsigned b = lo + (unsigned)i;
        const float    x = u2f(b);
        const float    a = which ? logf_pos_(x) : logf_(x);
        if (f2u(a) != f2u(logf_ref_(x))) { bad++; fb = b < fb ? b : fb; }
    }
    if (bad) { atomicAdd(mismatches, bad); atomicMin(first_bad, fb); }
}

// A scripted stream: next_a() returns the caller's words in turn (0 behind the last of them: a draw of exactly 0), counted in pairs
// like Philox, with sub-streams for shadow rays in name (kShadowSubstream: the walks treat it as a counter-based stream).
struct RngScript
{
    const unsigned* words;
    unsigned        count, pair0, pair;   // the script's first word is pair index pair0
    static constexpr bool kShadowSubstream = true;
    __device__ __forceinline__ float next_a()
    {
        const unsigned i = pair - pair0, w = i < count ? words[i] : 0u;
        pair++;
        return draw_to_float(w);
    }
    __device__ __forceinline__ float next_b() { return 0.5f; }
    __device__ __forceinline__ void set_pair(unsigned n) { pair = n; }
    __device__ __forceinline__ void save(unsigned& a, unsigned& b) const { a = pair; b = 0u; }
    __device__ __forceinline__ void load(unsigned a, unsigned) { pair = a; }
};
// approach_k's loop as it stood (two compares, logf_ with its select, the state saved after every step)
template <class RNG>
__device__ __forceinline__ void approach_walk_ref_(float& dist, const float t_empty, const float t_end, const float inv_sigma, const unsigned cap, RNG& rng,
                                                   unsigned& pairs, unsigned& sa, unsigned& sb)
{
    rng.save(sa, sb);
    for (; pairs < cap; pairs++)
    {
        const float d2 = dist + -logf_ref_(rng.next_a()) * inv_sigma;   // kernel.cu:1419
        if (!(d2 < t_empty) || d2 >= t_end) break;                       // the integrator's step: a fetch, or the way out
        dist = d2;
        (void)rng.next_b();   // the collision test's variate: `real` is false whatever it is; a sequential stream moves past it
        rng.save(sa, sb);
    }
}
// the inner loop of approach_local_k / approach_local_tab_k as it stood
template <class RNG>
__device__ __forceinline__ bool approach_segment_walk_ref_(float& dist, const float t_far, const float t_empty, const float inv_sigma, RNG& rng, unsigned& ta,
                                                           unsigned& tb, unsigned& steps)
{
    bool through = false;
    for (;;)
    {
        const float d2 = dist + -logf_ref_(rng.next_a()) * inv_sigma;   // kernel.cu:2085
        if (d2 >= t_far) { through = true; break; }                       // t_end = min(1e20, t_far): `through`, kernel.cu:2145
        if (!(d2 < t_empty) || steps > 60000u) break;                     // a fetch: render_k's
        dist = d2;
        (void)rng.next_b();   // the collision test's variate (`real` is false whatever it is): a sequential stream moves past it
        rng.save(ta, tb);
        steps++;
    }
    return through;
}
// One thread per case.  par[4 i ..] = (distance at the start, t_empty, t_end (kind 0) or t_far (kind 1), inv_sigma); scr[4 i ..] =
// (step cap (kind 0), first word of the case's script, its number of words, the stream's pair index at the start).  out_new /
// out_ref[5 i ..] = the hand-over of the walk as built / as it stood: (bits of the distance reached, steps, the stream's two state
// words before the flight in hand, through).  kind 0: approach_walk (approach_k); kind 1: approach_segment_walk (the local walks).
__global__ void test_approach_walk_k(int kind, int n, const float* par, const unsigned* scr, const unsigned* words, unsigned* out_new, unsigned* out_ref)
{
    const int i = threadIdx.x + blockIdx.x * blockDim.x;
    if (i >= n) return;
    const float    dist0 = par[4 * i], t_empty = par[4 * i + 1], t_box = par[4 * i + 2], inv_sigma = par[4 * i + 3];
    const unsigned cap = scr[4 * i];
    for (int ref = 0; ref < 2; ref++)
    {
        RngScript rng{words + scr[4 * i + 1], scr[4 * i + 2], scr[4 * i + 3], scr[4 * i + 3]};
        float     dist = dist0;
        unsigned  sa = 0, sb = 0, steps = 0, through = 0;
        if (kind == 0)
        {
            if (ref) approach_walk_ref_(dist, t_empty, t_box, inv_sigma, cap, rng, steps, sa, sb);
            else steps = approach_walk(dist, walk_limit(t_box, t_empty), inv_sigma, cap, rng, sa, sb);
        }
        else
        {
            rng.save(sa, sb);
            if (ref) through = approach_segment_walk_ref_(dist, t_box, t_empty, inv_sigma, rng, sa, sb, steps) ? 1u : 0u;
            else
            {
                unsigned long long n_steps = 0;
                through = approach_segment_walk(dist, t_box, t_empty, inv_sigma, rng, sa, sb, n_steps) ? 1u : 0u;
                steps   = (unsigned)n_steps;
            }
        }
        unsigned* o = (ref ? out_ref : out_new) + 5 * (size_t)i;
        o[0] = f2u(dist); o[1] = steps; o[2] = sa; o[3] = sb; o[4] = through;
    }
}

// ---- vp_test_sun_start: the start of a sun shadow ray with the row of its constants (vp_device.h sun_start) against the form it had
// before (profiles/experiments/sun_start_constants.txt).  TEST-ONLY code below: start_shadow's set-up as it stood, word for word.
__device__ __forceinline__ bool sun_start_ref_(f3 ro, f3 end, const SceneDev& S, f3& sd_out, float& len_out, float& tn, float& tf)
{
    // the ray's length |end - ro| is the root normalize() takes: formed once (ro - end is -(end - ro) exactly, so the squares
    // and their left-to-right sum are the same bits), then the reciprocal -- normalize's own v * (1.0f / sqrtf(dot(v, v)))
    const f3    dv = end - ro;
    const float d2 = dot(dv, dv);
    const float len = sqrt_(d2);
#ifdef VP_ARITH_FAST
    f3 sd = dv * rsqrt_(d2);   // (the fast mode keeps its two instructions, v_sqrt_f32 and v_rsq_f32, and its bits)
#else
    f3 sd = dv * rcp_(len);
#endif
    bool  hitv = intersect_box(ro, sd, S, tn, tf);
    sd_out = sd; len_out = len;
    return hitv;
}
// One thread per origin, one sun and one box per launch, as in render_k: thread 0 of a workgroup fills the row in LDS, the waves of
// 64 consecutive origins decide their branches together (lanes behind n are inactive, as lanes outside the collision block are).
// box[0..2] = bmin, box[3..5] = bmax.  out_new / out_ref[8 i ..] = (bits of sd.x, sd.y, sd.z, len, tnear, tfar; hit; the branches the
// lane's wave took -- sun_start's `taken` -- in out_new, 0 in out_ref).
__global__ void test_sun_start_k(int n, const float* origin, float sun_x, float sun_y, float sun_z, const float* box, unsigned* out_new, unsigned* out_ref)
{
    const f3 sun_dir = f3{sun_x, sun_y, sun_z};
    __shared__ float row[SR_WORDS];
    __shared__ float lbox[6];
    if (threadIdx.x == 0) sun_row_fill(row, sun_dir);
    if (threadIdx.x < 6) lbox[threadIdx.x] = box[threadIdx.x];
    __syncthreads();
    const int i = threadIdx.x + blockIdx.x * blockDim.x;
    if (i >= n) return;
    const f3 ro = f3{origin[3 * (size_t)i], origin[3 * (size_t)i + 1], origin[3 * (size_t)i + 2]};
    {
        f3       sd;
        float    len, tn, tf;
        unsigned taken = 0;
        const bool hit = sun_start(row, ro, lbox, lbox + 3, sd, len, tn, tf, &taken);
        unsigned* o = out_new + 8 * (size_t)i;
        o[0] = f2u(sd.x); o[1] = f2u(sd.y); o[2] = f2u(sd.z); o[3] = f2u(len); o[4] = f2u(tn); o[5] = f2u(tf); o[6] = hit ? 1u : 0u; o[7] = taken;
    }
    {
        SceneDev S = {};
        for (int c = 0; c < 3; c++) { S.bmin[c] = lbox[c]; S.bmax[c] = lbox[3 + c]; }
        f3    sd;
        float len, tn, tf;
        const bool hit = sun_start_ref_(ro, sun_dir * 1e10f, S, sd, len, tn, tf);
        unsigned* o = out_ref + 8 * (size_t)i;
        o[0] = f2u(sd.x); o[1] = f2u(sd.y); o[2] = f2u(sd.z); o[3] = f2u(len); o[4] = f2u(tn); o[5] = f2u(tf); o[6] = hit ? 1u : 0u; o[7] = 0u;
    }
}

// vp_test_camera_ray: camera_ray() of pixel (pixels[i] & 0xffff, pixels[i] >> 16) of a width x height image and intersect_box() of that
// ray, as this unit compiles them -- what ray_table_k (vp_kernels.hip, the exact unit) tabulates for render_k in BOTH units.
// out[6 i ..] = (rd.x, rd.y, rd.z, t_near, t_far, hit as 1.0f / 0.0f).
__global__ void test_camera_ray_k(SceneDev S, unsigned width, unsigned height, const unsigned* pixels, float* out, int n)
{
    const int i = threadIdx.x + blockIdx.x * blockDim.x;
    if (i >= n) return;
    const unsigned pix = pixels[i];
    f3 ro, rd;
    camera_ray(S, width, height, pix & 0xffffu, pix >> 16, ro, rd);
    float tn, tf;
    const bool hit = intersect_box(ro, rd, S, tn, tf);
    float* o = out + 6 * (size_t)i;
    o[0] = rd.x; o[1] = rd.y; o[2] = rd.z; o[3] = tn; o[4] = tf; o[5] = hit ? 1.0f : 0.0f;
}

// ---- vp_test_fetch_split: the axis split of sample_density01 in its two forms (vp_device.h fetch_scales) on caller-supplied bit
// patterns of s = p - bmin.  out[5 i ..] = (i, fw bits of axis_split; i, fw bits, low of axis_split_f32).  The exact unit's only:
// the fast unit's kernels do not take the folded form (kFetchFoldUnit) and it has no launcher for this one.
#ifndef VP_ARITH_FAST
__global__ void test_fetch_split_k(float linv, int n, int count, const unsigned* s_bits, unsigned* out_two, unsigned* out_fold)
{
    const int t = threadIdx.x + blockIdx.x * blockDim.x;
    if (t >= count) return;
    const float s = u2f(s_bits[t]);
    const float m = linv * (float)n;
    for (int fold = 0; fold < 2; fold++)
    {
        const float xb = fold ? fma_(s, m, -0.5f) : fma_(s * linv, (float)n, -0.5f);
        int   i, j;
        float fw, gw;
        bool  low;
        axis_split(xb, n, i, fw);
        axis_split_f32(xb, n, j, gw, low);
        unsigned* o = (fold ? out_fold : out_two) + 5 * (size_t)t;
        o[0] = (unsigned)i; o[1] = f2u(fw); o[2] = (unsigned)j; o[3] = f2u(gw); o[4] = low ? 1u : 0u;
    }
}
#endif
