// vp_integrator.h -- the integrator's kernels: render_k (and the per-lane machinery around it) and the approach walks ahead of it
// (approach_k, approach_local_k, approach_local_tab_k).  Included INSIDE a namespace by two translation units: vp_kernels.hip
// (namespace vp: the exact arithmetic of DESIGN.md section 2) and vp_kernels_fast.hip (namespace vp::fast, compiled with
// VP_ARITH_FAST: vp_math.h's fast helpers).  Everything else the kernels read -- the tables, the pixel lists, the light and
// miss-fill kernels -- lives in vp_kernels.hip alone and is the same in both modes.
// per-lane path states.  FAST states advance inside the inner tracking loop; the others are events
// a lane parks in until the wave runs its slow path.
enum : int
{
    ST_DONE    = 0,  // no path: wants a new sample from the queue
    ST_SETUP   = 1,  // needs a segment set-up (FAST for the decomposition estimator)
    ST_TRACK   = 2,  // FAST: free-flight steps of the primary ray
    ST_SHADOW  = 3,  // FAST: free-flight steps of the sun shadow ray (Tr_spectral)
    EV_SCATTER = 4,  // collision found: direct-lighting set-up
    EV_NEE     = 5,  // shadow transmittance known: add sun light, sample the phase function
    EV_BG      = 6,  // ray left the medium: environment lookup
    EV_WRITE   = 7,  // path finished: emit the sample
    EV_MIS     = 8,  // active environment sampling only: draw the one-sample-MIS direction, start its shadow ray
    EV_HG      = 9   // sample the phase function, continue the path
};

// Perturbation profiling (round 5; scripts/r05_pad_profile.sh, profiles/r05_pad_profile.md): no per-PC sampling is to be had on this
// pool, so the marginal cost of a code block is measured by ADDING work to it: -DVP_PAD_<BLOCK>=N puts N dependent v_fma_f32 (the
// cheapest vector instruction: 1.06 ns per wave-instruction per SIMD at saturation) on a scratch register into that block of
// render_k; the launch-time difference against the unpadded build, divided by the block's executions, is what one more
// instruction there costs -- the full issue slot if the vector pipe is the bound, less if the block runs in the shadow of waits.
// All zero in the shipped build: vp_pad<0> is empty.
#ifndef VP_PAD_STEP
#define VP_PAD_STEP 0
#endif
#ifndef VP_PAD_FETCH
#define VP_PAD_FETCH 0
#endif
#ifndef VP_PAD_EOF
#define VP_PAD_EOF 0
#endif
#ifndef VP_PAD_SETUP
#define VP_PAD_SETUP 0
#endif
#ifndef VP_PAD_COLL
#define VP_PAD_COLL 0
#endif
#ifndef VP_PAD_END
#define VP_PAD_END 0
#endif
template <int N>
__device__ __forceinline__ void vp_pad()
{
    if constexpr (N > 0)
    {
#ifdef VP_PAD_INDEPENDENT   // four independent chains: issue cost without the dependent-issue latency of one chain
        float t0 = 1.0f, t1 = 1.0f, t2 = 1.0f, t3 = 1.0f;
#pragma unroll
        for (int i = 0; i < N / 4; i++)
            asm volatile("v_fma_f32 %0, %0, %0, %0\n\tv_fma_f32 %1, %1, %1, %1\n\tv_fma_f32 %2, %2, %2, %2\n\tv_fma_f32 %3, %3, %3, %3" : "+v"(t0), "+v"(t1), "+v"(t2), "+v"(t3));
#else
        float t = 1.0f;
#pragma unroll
        for (int i = 0; i < N; i++) asm volatile("v_fma_f32 %0, %0, %0, %0" : "+v"(t));
#endif
    }
}

__device__ __forceinline__ unsigned lane_rank(unsigned long long mask)
{
    return __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

// Cold per-path state (round 4).  A path's radiance sum, the direction it resumes after a shadow ray, its sample
// coordinates, scatter count, phase-function parameters and the stream position saved across a shadow ray are touched in the event
// blocks and where a shadow ray ends -- never in the free-flight step.  In the plain kernels they live in LDS, one word per lane
// and field (14 words: 14 KB per workgroup; 15 or 17 where the sun's light is summed in the event pass: DEFER in render_k), so that the
// kernel fits SIX waves per SIMD (80 registers) where it held five:
// +4 % on both estimators (profiles/experiments/r04_cold_state_in_lds.txt).  ColdVal / ColdF3 are that word or triple in LDS
// (COLD = true) or an ordinary variable (the LDS-table kernel, whose LDS is the table's, and the light kernels, which fit seven
// or eight waves as they are).
template <class T, bool COLD>
struct ColdVal;
template <class T>
struct ColdVal<T, true>
{
    static_assert(sizeof(T) == sizeof(float), "one LDS word per lane and field");
    float* p;   // the word is a float in LDS whatever T is: values go through __builtin_bit_cast, not through a punned pointer
    __device__ __forceinline__ explicit ColdVal(float* q) : p(q) {}
    __device__ __forceinline__ operator T() const { return __builtin_bit_cast(T, *p); }
    __device__ __forceinline__ ColdVal& operator=(T v) { *p = __builtin_bit_cast(float, v); return *this; }
};
template <class T>
struct ColdVal<T, false>
{
    T v = T();
    __device__ __forceinline__ explicit ColdVal(float*) {}
    __device__ __forceinline__ operator T() const { return v; }
    __device__ __forceinline__ ColdVal& operator=(T w) { v = w; return *this; }
};
template <bool COLD, int STRIDE>
struct ColdF3;
template <int STRIDE>
struct ColdF3<true, STRIDE>
{
    float* p;
    __device__ __forceinline__ explicit ColdF3(float* q) : p(q) {}
    __device__ __forceinline__ operator f3() const { return f3{p[0], p[STRIDE], p[2 * STRIDE]}; }
    __device__ __forceinline__ ColdF3& operator=(f3 v) { p[0] = v.x; p[STRIDE] = v.y; p[2 * STRIDE] = v.z; return *this; }
};
template <int STRIDE>
struct ColdF3<false, STRIDE>
{
    f3 v = {};
    __device__ __forceinline__ explicit ColdF3(float*) {}
    __device__ __forceinline__ operator f3() const { return v; }
    __device__ __forceinline__ ColdF3& operator=(f3 w) { v = w; return *this; }
};
// One null collision of the spectral tracker where the density is +0 (kernel.cu:2107-2134 with sigma_t_den = +0: Ps = +0, c = Pn,
// `real` false for any draw, sigma_null_den = sigma_t'), for a throughput with three equal channels t:
// Pn = (m + m) + m with m = |sigma_t' t|, t *= sigma_t' * ((inv_sigma_t * Pn) / Pn).  The factor is 1 up to rounding, not exactly.
__device__ __forceinline__ float null_collision_in_empty_space(float t, float sigma_t_prime, float inv_sigma_t)
{
    float mn = __builtin_fabsf(sigma_t_prime * t);
    float Pn = (mn + mn) + mn;
    return t * (sigma_t_prime * wdiv_(inv_sigma_t * Pn, Pn));
}
// Does a null collision where the density is +0 leave the throughput (t.x, t.y, t.z) bit for bit as it is, whatever is drawn?  The
// spectral tracker's expressions (kernel.cu:2107-2134; tracking_step below) with sigma_t_den = +0 -- sigma_c = 0: no control
// component where the cells are empty --: Ps = |0 t.x| + |0 t.y| + |0 t.z| must be +0 (then `real`, e * c < Ps, is false for any
// draw e), and the factor every channel is multiplied by, sigma_null * f = sigma_t' * ((inv_sigma_t * c) / Pn), must be exactly 1.
// The one-channel (ACH) form of the step computes the same sums ((m + m) + m) from one product.
__device__ __forceinline__ bool null_collision_is_identity(f3 t, float sigma_t_prime, float inv_sigma_t)
{
    const float Ps = __builtin_fabsf(0.0f * t.x) + __builtin_fabsf(0.0f * t.y) + __builtin_fabsf(0.0f * t.z);
    const float Pn = __builtin_fabsf(sigma_t_prime * t.x) + __builtin_fabsf(sigma_t_prime * t.y) + __builtin_fabsf(sigma_t_prime * t.z);
    const float c  = Ps + Pn;
    return Ps == 0.0f && sigma_t_prime * wdiv_(inv_sigma_t * c, Pn) == 1.0f;
}

// Does a null collision in empty space leave a throughput of 1 as it is?  (The reasons and the mask: vp_kernels.hip bound_bytes_k.)
// Here, beside the integrator, because the answer belongs to the arithmetic: the exact mode asks it for the light class and for
// approach_k; the fast mode (vp_kernels_fast.hip) asks it again, in its own arithmetic, before it lets approach_k skip null
// collisions that its render_k would make.
__global__ void light_identity_k(ParamDev P, int local, const unsigned* mask, unsigned* flag)
{
    const unsigned b = threadIdx.x;   // 256 threads
    if (local && !(mask[b >> 5] >> (b & 31u) & 1u)) return;
    if (!local && b) return;
    const float max_sig = max3(f3{P.sigma_t[0], P.sigma_t[1], P.sigma_t[2]});
    const float s       = hyperion_s(0 - 5);
    float sigma_t_prime;
    if (local)
    {
        const float reduction   = (1.0f - s) + s * (1.0f - P.g);           // segment_medium(), no scatter behind the path
        const float cur_density = reduction * P.density;
        const float d_max       = fmaxf(0.0001f, (float)b * VP_U8_SCALE);   // segment_setup()
        sigma_t_prime           = max_sig * cur_density * d_max;
    }
    else
    {
        const float cur_density = (1.0f - s) * P.density + s * P.density * (1.0f - P.g);   // thr_table_k
        sigma_t_prime           = max_sig * cur_density;
    }
    const float inv_sigma_t = rcp_(sigma_t_prime);
    if (!(null_collision_in_empty_space(1.0f, sigma_t_prime, inv_sigma_t) == 1.0f)) atomicAnd(flag, 0u);
}

// LDSB: the (max,min) brick table of the decomposition estimator is staged through LDS (BASELINE config 3:
// 256^3 / 8^3 bricks = 32768 byte pairs = 64 KiB).  Those workgroups are 512 threads so that two of them
// (2 x 64 KiB of the CU's 160 KiB) keep 16 waves per CU resident.
// ACH: achromatic medium (sigma_t and albedo equal in all three channels): the three throughput channels stay
// bitwise identical (same operations on the same values), so one is carried and the collision sums are
// formed from one product, (m + m) + m, exactly as the three-channel expression evaluates.
// MIS: active environment sampling with one-sample MIS after the sun estimate (the reference's !PASSIVE_ENVMAP
// build, kernel.cu:2220-2297); the shipped configuration is passive (MIS = false).
// TRK: 0 = spectral tracking (SPECTRAL_TRACKING 1, the shipped build); 1 = scalar tracking (SPECTRAL_TRACKING 0);
// 2 = MULTI_CHANNEL 1: scalar tracking of one colour channel drawn per sample (kernel.cu:15-34, :1993-1994, :2311-2313).
// LIGHT: the kernel of the "light" pixel class (spectral tracking): every camera ray of those pixels either misses the box or
// meets certified-empty cells over its whole chord (empty_table_k / crawl_table_k), so a path is: restart segments (local-majorant
// estimators) and free-flight steps whose null collisions have den = +0, then the environment.  No fetch code, no collision,
// shadow or phase states.
#ifndef VP_LOCAL_MIN_WAVES
#define VP_LOCAL_MIN_WAVES 6   // plain achromatic local-majorant kernels, cold state in LDS: 80 registers, no spill.  The chromatic ones would
                               // spill four or five at six waves and run as the LDS-table kernel's helper workgroups, where a fifth wave is
                               // all a SIMD has room for: they keep five
#endif
// Waves per SIMD the register budget of a render_k instance is held to (the second argument of its __launch_bounds__), one case per
// line instead of the nested conditional it used to be; the reasons are in the comment at the kernel:
constexpr int render_min_waves(int est, bool count, int ldsb, bool ach, bool mis, int trk, bool light, bool cancel)
{
    if (VP_MIN_WAVES > 1) return VP_MIN_WAVES;                                            // a build-wide override
    if (light) return count ? 5 : (est != EST_GLOBAL ? VP_LIGHT_LOCAL_MIN_WAVES : VP_LIGHT_MIN_WAVES);
    if (mis || ldsb == 1) return 1;                                                        // the MIS build; the 16-bit LDS table (512-thread workgroups)
    if (count) return 4;                                                                   // counting variants: untimed, no spills
    if (est == EST_GLOBAL && trk == 0) return VP_GLOBAL_MIN_WAVES;
    if (trk) return 4;                                                                     // scalar tracking builds
    return (ach && !cancel) ? VP_LOCAL_MIN_WAVES : 5;                                      // local majorants: achromatic six, chromatic / look-ahead five
}
// LYR: the instance of a layers launch (include/volpath.h vp_render_frames_layers; LaunchDev::layers): vp_dispatch.h names it for the
// subset the feature is built for.  Every other instance carries no code for it.
// GRP: the instance of a light-groups launch (include/volpath.h vp_render_frames_groups; LaunchDev::groups), named by vp_dispatch.h for
// the same subset.  It differs at the path end only: what the environment adds there is not summed into `rad` but staged as a sample
// of its own in the second staging plane.  Every other instance carries no code for it.
// LYR and GRP: the instance of a group-layers launch (include/volpath.h vp_render_frames_group_layers; LaunchDev::layers and
// LaunchDev::groups), named by vp_dispatch.h for the same subset.  An unscattered path ends as in a layers launch (its marked
// throughput in the first plane, nothing in the second), a scattered one as in a groups launch.
#define VP_RENDER_K_HAS_PLANES 1
template <int EST, class RNG, bool QUANT, bool COUNT, int LDSB, bool ACH, bool MIS, int TRK, bool LIGHT = false, bool CANCEL = false, bool HALF = false, bool LYR = false,
          bool GRP = false>
// Occupancy (round 4: the cold per-path state in LDS, ColdVal above; profiles/r04_kernel_resources.txt).  The achromatic
// global-majorant kernel needs 72 registers: SEVEN waves per SIMD (C2 2541 -> 2781 Msamples/s); the chromatic one and the plain
// achromatic local-majorant kernels 80: six (c3ref 2398 -> 2513); the LDS-table kernel keeps its state in registers (its LDS is the
// table's): 98, four waves and the helper workgroup's fifth.  Before, with everything in registers: 91-96, five waves (six cost
// three spilled registers and lost).
// (CANCEL instances of the local-majorant kernels: look-ahead batches are launched with five workgroups per CU -- vp_render.cpp -- so five
// waves are what their registers are budgeted for: no spill.)
__global__ __launch_bounds__(LDSB == 1 ? VP_BLOCK_LDS : VP_BLOCK, render_min_waves(EST, COUNT, LDSB, ACH, MIS, TRK, LIGHT, CANCEL))
void render_k(SceneDev S, LaunchDev L)
{
    __shared__ unsigned short lds_bounds[LDSB == 1 ? VP_LDS_BOUND_ENTRIES : 1];
    // LDSB == 2 (round 5): the table as 2-bit CODES into a palette of at most four distinct (max,min) pairs -- a binary volume has three:
    // (0,0), (255,0), (255,255) -- 8 KiB instead of 64: small enough to sit BESIDE the cold per-path state of a 256-thread workgroup, so
    // this kernel keeps the plain kernel's registers and occupancy (six / five waves per SIMD) where the 16-bit table's costs a third
    // of both (98-102 registers, four waves and a helper workgroup)
    __shared__ unsigned lds_codes[LDSB == 2 ? VP_LDS_BOUND_ENTRIES / 16 : 1];
    if (LDSB == 2)
    {
        const uint4* src = reinterpret_cast<const uint4*>(L.bound_codes);
        uint4*       dst = reinterpret_cast<uint4*>(lds_codes);
        const int    n16 = (S.bnx * S.bny * S.bnz + 63) / 64;   // 64 codes per 16 bytes; the device table is padded
        for (int w = threadIdx.x; w < n16; w += VP_BLOCK) dst[w] = src[w];
        __syncthreads();
    }
    if (LDSB == 1)
    {
        // coalesced 16-byte loads of the table, 16-byte LDS stores
        const uint4* src = reinterpret_cast<const uint4*>(S.bounds_u8);
        uint4*       dst = reinterpret_cast<uint4*>(lds_bounds);
        const int    n16 = (S.bnx * S.bny * S.bnz * 2 + 15) / 16;  // the device table is padded to 16 bytes
        for (int w = threadIdx.x; w < n16; w += VP_BLOCK_LDS) dst[w] = src[w];
        __syncthreads();
    }
    // The kernel arguments once more, in LDS (round 5).  The event section and light_done() read their uniforms -- camera, sun,
    // environment, queue and image descriptors: ~70 scalars the tracking loop never touches -- afresh at every visit instead of holding
    // them in SGPRs across the loop (round 3).  They did so with flat loads of the argument segment: L1/L2 round trips of their own, and
    // every s_waitcnt vmcnt(0) behind one also waits for the wave's density fetches.  An LDS read waits for itself only.
    // VP_EXP_FLAT_KARGS: the flat loads, for the A/B (profiles/experiments/r05_kargs_lds.txt).
    constexpr unsigned KARG_L_   = ((sizeof(SceneDev) + alignof(LaunchDev) - 1) / alignof(LaunchDev)) * alignof(LaunchDev);
    constexpr unsigned KARG_WDS_ = (KARG_L_ + sizeof(LaunchDev) + 3) / 4;
    constexpr unsigned KARG_ROW_ = (KARG_WDS_ + 3u) & ~3u;   // where the sun row starts behind the copy: 16-byte aligned whatever the structs' size (its fill stores four words at a time)
    constexpr bool LOCAL = EST != EST_GLOBAL;  // the two local-majorant estimators share the segment logic
    constexpr bool TAB   = TRK == 0 && LDSB != 1 && !LIGHT && !MIS;   // the instances with the collision block's tables, below
    // SUNROW: the sun ray's row (vp_device.h sun_row_fill) lies behind the copy, so that the event section's opaque offset reaches it
    // too.  The instances with the tables except the bounded estimator's: its achromatic kernels run a wave ABOVE the occupancy their
    // register budget asks for (71 registers: seven waves where six are budgeted) and the second path costs them that wave, so
    // they keep the general start.  Not with VP_EXP_BOX_PARALLEL either: sun_start's box test is the axis-by-axis sequence, and
    // that experiment's build is to run the other form everywhere.
#ifdef VP_EXP_BOX_PARALLEL
    constexpr bool SUNROW = false;
#else
    constexpr bool SUNROW = TAB && EST != EST_BOUNDED;
#endif
    __shared__ __attribute__((aligned(16))) unsigned kargs_lds_[KARG_ROW_ + (SUNROW ? SR_WORDS : 0)];
    {
        const unsigned* src = (const unsigned*)__builtin_amdgcn_kernarg_segment_ptr();
        for (unsigned w = threadIdx.x; w < KARG_WDS_; w += (LDSB == 1 ? VP_BLOCK_LDS : VP_BLOCK)) kargs_lds_[w] = src[w];
    }
    // The collision block's scene constants (vp_device.h coll_row_fill): what a collision, the shadow ray it starts and the segment
    // after it need from the scatter count and Param alone -- the Hyperion-reduced phase parameter with the g-only parts of the phase
    // function, the reduced density, the global majorant and its reciprocal: two IEEE reciprocals, a division and ~25 other
    // instructions per collision -- takes sixteen values per launch.  Thread n fills row n; a collision reads two rows.  Spectral
    // tracking without MIS only; not the 16-bit LDS-table kernel, whose two workgroups per CU leave no byte of LDS over.
    // The sun shadow ray's constants (sun_row_fill): what its start computes from sun_dir alone -- the far end, the length, the
    // direction and the box test's slab reciprocals -- takes one value each per launch wherever the collision point is absorbed by
    // the far end's magnitude.  One more thread fills that row; start_shadow compares operand bits per wave (vp_device.h sun_start).
    __shared__ __attribute__((aligned(16))) float coll_tab_[TAB ? VP_COLL_ROWS : 1][CR_WORDS];
    if (TAB && threadIdx.x < VP_COLL_ROWS)
        coll_row_fill(coll_tab_[threadIdx.x], (int)threadIdx.x, L.P.g, L.P.density, max3(f3{L.P.sigma_t[0], L.P.sigma_t[1], L.P.sigma_t[2]}), LOCAL);
    if (SUNROW && threadIdx.x == VP_COLL_ROWS)
        sun_row_fill(reinterpret_cast<float*>(kargs_lds_ + KARG_ROW_), f3{S.sun_dir[0], S.sun_dir[1], S.sun_dir[2]});
    __syncthreads();
    auto coll_row = [&](int n) __attribute__((always_inline)) -> const float* {
        return TAB ? coll_tab_[n < 0 ? 0 : (n > VP_COLL_ROWS - 1 ? VP_COLL_ROWS - 1 : n)] : nullptr;
    };
    // Counter-based streams, passive environment: ONE event visit per collision.  The shadow ray draws from a sub-stream of its own,
    // so the two phase-function variates -- the path's next draws -- are the same whether they are taken before or after it: the
    // new direction is sampled in the collision block (and, global majorant, the box is intersected for it), the shadow ray is
    // tracked, and where it ends the tracking step itself adds the light and goes on with the new segment.  The sequential
    // sampler.h stream (and the MIS build) keep the reference's order: collision, shadow ray, light, phase function.
    constexpr bool EARLY = RNG::kShadowSubstream && !MIS && !LIGHT;
    // Global majorant, counter-based streams: a new sample's camera ray may have been walked through its certified-empty stretch by
    // approach_k already (L.approach): the path is taken up where that walk stopped -- same draws, same sums, made elsewhere.
    constexpr bool APPR = EST == EST_GLOBAL && TRK == 0 && !LIGHT && !MIS;   // (any stream: the hand-over carries its state)
    // Global majorant, general class: a fresh sample's camera ray and box test are functions of its pixel alone (quirk Q3; the box is the
    // scene's) and come from the per-view ray table where the launch has one (L.ray, vp_kernels.hip ray_table_k); without, or with a
    // sub-pixel factor, they are computed per sample as ever -- the same bits.
    constexpr bool RAYT = EST == EST_GLOBAL && !LIGHT;
    // decomposition estimator: the same for the restart segments that end before the certified-empty distance (approach_local_k)
    constexpr bool APPR_L = EST == EST_DECOMP && TRK == 0 && !LIGHT && !MIS;
    // Exit flights.  A path in empty space that can do nothing but leave the box -- every cell its ray can still meet is certified
    // empty (L.exit_oct: the quarter pyramid of cells that opens from its cell along the direction's dominant axis) and a null collision
    // there leaves its throughput bit for bit as it is (null_collision_is_identity) -- ends with the environment along its direction
    // whatever it draws on the way (no draw is used after a path's end; the heat channel counts scatters): it goes to EV_BG at once
    // instead of walking there at 800 null collisions per unit length (38 % of the lane-steps of BASELINE config 2's general class).
    // A lane counts its null collisions in empty space in `terms` (free while no shadow ray is tracked); whenever its wave is in the
    // event pass anyway, lanes that have counted K are tested: one byte load, no loop, no parking.  Not for the bounded estimator (its
    // heat channel counts the segments of that walk), the scalar builds and MIS.
    constexpr bool EXITC = TRK == 0 && !MIS && !LIGHT && EST != EST_BOUNDED && (QUANT || EST == EST_GLOBAL);
    // A lane whose collision is real parks with ro, rd and dist untouched: the collision point ro + rd * dist is formed where it is
    // used, at the top of the collision block, not under `if (real)` in the tracking step -- where the assignment made the compiler
    // keep two copies of the origin and move between them on every path, in all four unrolled steps.  The control collision of the
    // decomposition estimator parks the same way, with dist = distc.  (The MIS kernels, which also keep the segment origin, do not.)
    constexpr bool PARK = !MIS;
    // DEFER: the sun's light of a shadow ray that ended in the tracking loop is added at the lane's next event visit (see the flush at
    // the top of the event pass).  Spectral tracking only: the scalar builds keep the sum where the ray ends.
    constexpr bool DEFER = EARLY && TRK == 0;
    // Layers launches (LaunchDev::layers) run instances of their own (LYR), built for spectral tracking with the passive environment,
    // without work counters and look-ahead: the host refuses the rest.
    constexpr bool LAYERS = LYR;
    static_assert(!LYR || (TRK == 0 && !MIS && !COUNT && !CANCEL), "layers instances: spectral tracking, passive environment, no counters, no look-ahead");
    // Light-groups launches (LaunchDev::groups) likewise (GRP).  Both: a group-layers launch (include/volpath.h
    // vp_render_frames_group_layers) -- an unscattered path ends as in a layers launch, a scattered one as in a groups launch.
    static_assert(!GRP || (TRK == 0 && !MIS && !COUNT && !CANCEL), "groups instances: spectral tracking, passive environment, no counters, no look-ahead");
    const ParamDev& P = L.P;
    const f3    sig_t     = f3{P.sigma_t[0], P.sigma_t[1], P.sigma_t[2]};
    const f3    sig_s     = sig_t * f3{P.albedo[0], P.albedo[1], P.albedo[2]};
    const float max_sig   = max3(sig_t);
    const float min_sig   = min3(sig_t);
    const float density   = P.density;

    // ---- per-lane path state
    int      st = ST_DONE;
    bool     exhausted = false;
    // cold state: in LDS for the plain kernels (ColdVal / ColdF3 above)
    constexpr bool COLD = LDSB != 1 && !LIGHT;
    constexpr int  CS_  = COLD ? VP_BLOCK : 1;
    // (the occupancy these kernels are budgeted for holds only while that many workgroups' cold state fits the CU's LDS --
    // a workgroup is one wave per SIMD, so waves per SIMD = workgroups per CU; gfx950: 160 KiB)
    // DEFER: the light weight of the shadow ray in flight takes the place of `ph` (one word, achromatic) or that word and two more
    // (chromatic); one more word holds the ended ray's termination bits until the event pass has added its light
    constexpr int NCOLD = 14 + (DEFER ? (ACH ? 1 : 3) : 0);
    static_assert(!COLD || (LOCAL ? VP_LOCAL_MIN_WAVES : VP_GLOBAL_MIN_WAVES) * (NCOLD * VP_BLOCK * 4 + KARG_ROW_ * 4 + VP_COLL_ROWS * CR_WORDS * 4 + (SUNROW ? SR_WORDS * 4 : 0) + (LDSB == 2 ? VP_LDS_BOUND_ENTRIES / 4 : 0)) <= VP_LDS_BYTES_PER_CU,
                  "cold per-path state: more workgroups per CU than the LDS holds -- lower VP_*_MIN_WAVES for this ARCH");
    __shared__ float cold_[COLD ? NCOLD : 1][CS_];
    float* const cold_p = &cold_[0][COLD ? threadIdx.x : 0];
    ColdF3<COLD, CS_>       rad(cold_p), pd(cold_p + 3 * CS_);   // radiance sum; primary direction, kept while the shadow ray is tracked
    ColdVal<float, COLD>    ph(cold_p + 6 * CS_), phase_g(cold_p + 7 * CS_);
    ColdVal<unsigned, COLD> item(cold_p + 8 * CS_);              // where this lane's sample goes in the staging buffer
    ColdVal<unsigned, COLD> px(cold_p + 9 * CS_), py(cold_p + 10 * CS_);
    ColdVal<int, COLD>      frame(cold_p + 11 * CS_);
    ColdVal<int, COLD>      nsc(cold_p + 12 * CS_);              // num_scatters (DECOMP, BOUNDED) / depth i (GLOBAL)
    ColdVal<unsigned, COLD> rng_saved(cold_p + 13 * CS_);        // the path's own stream position while a shadow ray draws from its sub-stream
    // DEFER: lw = (ACH ? thr.x : thr) * ph, the weight of the sun's light at the last collision (lw_x in ph's word); light_bits = the
    // termination bits of a shadow ray that has ended and whose light is not in `rad` yet, LIGHT_NONE otherwise
    constexpr unsigned LIGHT_NONE = 0xffffffffu;
    ColdVal<float, COLD>    lw_x(cold_p + 6 * CS_), lw_y(cold_p + (DEFER && !ACH ? 14 : 6) * CS_), lw_z(cold_p + (DEFER && !ACH ? 15 : 6) * CS_);
    ColdVal<unsigned, COLD> light_bits(cold_p + (DEFER ? NCOLD - 1 : 6) * CS_);
    if (COLD) { rad = f3{0.0f, 0.0f, 0.0f}; pd = f3{0.0f, 0.0f, 0.0f}; ph = 0.0f; phase_g = 0.0f; item = 0u; px = 0u; py = 0u; frame = 0; nsc = 0; rng_saved = 0u; }
    if (DEFER) { lw_x = 0.0f; if (!ACH) { lw_y = 0.0f; lw_z = 0.0f; } light_bits = LIGHT_NONE; }
    RNG      rng;
    f3       ro = {}, rd = {};   // the ray being tracked (primary, or the shadow ray while ST_SHADOW)
    f3       inv_rd = {};        // 1 / rd of the primary ray (decomposition set-up)
    f3       thr = {};
    int      seg = 0;            // BOUNDED only: loop index i, one per tracked segment (kernel.cu:1716)
    float    dist = 0, t_end = 0;  // position on the tracked ray; where the current free flight ends
    float    t_far = 0, distc = 0, inv_sigma = 0, inv_sigma_t = 0, sigma_t_prime = 0, sigma_c = 0;
    float    cur_density = 0, d_max = 0;
    f3       nee_a = {};
    int      terms = 0;
    // MIS only: colour and weight of the light estimate in flight, rad += nee_c * (nee_t * transmittance);
    // 0 = sun, 1 = environment; the shadow majorant of this collision; the ray origin before the collision
    f3       nee_c = {}, nee_t = {}, seg_o = {};
    int      nee_stage = 0;
    float    sh_inv_sigma = 0, sh_density = 0;
    // scalar tracking only: the sample's extinction coefficient (density, or density * sigma_t[chan]) and its channel
    float    sig_base = density;
    int      chan = 0;
    // the unscattered camera ray is certified to run through empty cells (all eight texels of every fetch zero) up to this
    // distance from the current ray / segment origin (empty_table_k, crawl_table_k); 0 once the path has scattered
    float    t_empty = 0.0f;
    // COUNT build only: where the timed kernel ends the current sun shadow ray (it walks on here, so that density_lookups stays
    // the estimator's count, and stops counting loads)
    float    t_clip = 1e30f;
    bool     ex_clear = false;   // COUNT build only: the timed kernel has ended this path (exit flight); it walks on here, counting no loads
    unsigned long long c_load = 0, c_xtest = 0, c_xout = 0, c_xok = 0;
    unsigned zrun = 0;   // COUNT build only: null collisions in empty space of the current flight (c_xout: those of flights that left the box)

    unsigned long long c_den = 0, c_bnd = 0, c_opa = 0, c_env = 0, c_sca = 0, c_smp = 0;
    unsigned long long d_iter = 0, d_act = 0, d_outer = 0, d_shadow = 0;  // debug (lane 0 counts wave events)
    // PROF: the profiling form of the counting build (-DVP_PROFILE_BLOCKS=1: `make dev DEVNAME=prof DEVFLAGS=-DVP_PROFILE_BLOCKS=1`, scripts/
    // block_profile.py): cycle stamps of the two phases, loop statistics and the block tallies below -- 30 64-bit counters per lane that
    // the shipped counting build (the work counters of bench.py's lookups_per_sample) does not carry, nor their spills
    constexpr bool PROF = COUNT && VP_PROFILE_BLOCKS;
    unsigned long long t_slow = 0, t_fast = 0, t_mark = PROF ? __builtin_amdgcn_s_memtime() : 0ull;  // shader cycles
    // PROF build: how often each code block runs (wave executions) and for how many lanes -- where the lane slots go
    enum { B_SETUP, B_HALF, B_LOOK, B_EXIT, B_SCATTER, B_NEE, B_HG, B_BG, B_WRITE, B_REFILL, B_GSETUP, B_FETCH, B_ZERO, B_ZERO_SH, B_EXITT, B_NBLK };
    unsigned long long bw[B_NBLK] = {}, bl[B_NBLK] = {};
    // ... and, for the three blocks a regrouping of work would have to fill (collision, end of flight, restart set-up), the HISTOGRAM of
    // lanes per execution in eight buckets of eight lanes (round 5: profiles/experiments/r05_wavefront_break_even.md)
    unsigned long long hist[3][8] = {};
    unsigned long long ctrl_w = 0, ctrl_l = 0;
    auto tally = [&](int b, bool on) __attribute__((always_inline)) {
        if (PROF)
        {
            unsigned long long m = __ballot(on);
            if (m)
            {
                bw[b] += 1; bl[b] += (unsigned)__popcll(m);
                const int h = b == B_SCATTER ? 0 : b == B_EXIT ? 1 : b == B_SETUP ? 2 : -1;
                if (h >= 0) hist[h][((unsigned)__popcll(m) - 1u) >> 3] += 1;
            }
        }
    };

    const unsigned lane = threadIdx.x & 63u;
    unsigned chunk_s = 0, chunk_n = 0;    // next sample of the current chunk, samples in it (wave-uniform)
    unsigned chunk_q = 0, chunk_f0 = 0;   // its first pixel slot and first frame (wave-uniform)
    bool     queue_empty = false;
    // the queue this wave draws from: its XCD's first (HW_REG_XCC_ID, bits 3:0), then the others in turn
    unsigned q_cur   = __builtin_amdgcn_s_getreg((4 - 1) << 11 | 20) & (VP_NQUEUES - 1);
    unsigned q_tried = 0;
    unsigned end_skipped = 0;   // event visits since the path-end chain last ran (wave-uniform)
    unsigned visits = 0;        // CANCEL: event visits of this wave (wave-uniform)

    for (;;)
    {
        if (PROF && lane == 0) d_outer++;
        // =========================================================== slow path: events
        // The event section reads its uniforms (camera, sun, environment, queue and image descriptors: ~70 scalars that the
        // tracking loop never touches) from the kernel-argument segment afresh in every visit instead of holding them in SGPRs
        // across the tracking loop, whose own scalars then fit without spilling into vector lanes.  The empty asm keeps the
        // compiler from hoisting those loads back out of the loop; it also makes the pointer divergent for it, so the reads are
        // per-lane loads of the fields a visit's branches need, not scalar loads -- which, tried, load the whole structs and spill
        // 35-49 SGPRs: -20...-45 % (profiles/experiments/r03_scalar_kernarg_reload.txt).  Rounds 3-4: flat loads of the argument
        // segment; round 5: reads of its copy in LDS (kargs_lds_, above).
        {
#ifdef VP_EXP_FLAT_KARGS
        const char* kargs_ = (const char*)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(kargs_));
#else
        unsigned ko_ = 0;
        asm volatile("" : "+v"(ko_));   // (an opaque offset: the reads stay LDS reads and stay inside the visit)
        const char* kargs_ = reinterpret_cast<const char*>(kargs_lds_) + ko_;
#endif
        const SceneDev&  S = *reinterpret_cast<const SceneDev*>(kargs_);
        const LaunchDev& L = *reinterpret_cast<const LaunchDev*>(kargs_ + KARG_L_);
        const ParamDev&  P = L.P;
        const f3 sun_dir   = f3{S.sun_dir[0], S.sun_dir[1], S.sun_dir[2]};
        const f3 sun_power = f3{S.sun_power[0], S.sun_power[1], S.sun_power[2]};
        // Tr_spectral set-up kernel.cu:763-780: shadow ray from the collision point ro toward `end`
        // stage: 0 = the sun ray, 1 = the environment ray of the one-sample MIS
        auto start_shadow = [&](f3 end, float inv_s, float den, unsigned stage) __attribute__((always_inline)) {
            // the ray's length |end - ro| is the root normalize() takes: formed once (ro - end is -(end - ro) exactly, so the squares
            // and their left-to-right sum are the same bits), then the reciprocal -- normalize's own v * (1.0f / sqrtf(dot(v, v)))
            f3    sd;
            float len, tn, tf;
            bool  hitv;
            if (SUNROW && stage == 0u)
            {
                // the sun ray, with the row of its constants: the same values, the roots and divisions taken only where a wave's
                // operands differ in a bit from the row's (`end` is the row's first three words)
#ifdef VP_EXP_FLAT_KARGS
                const float* const srow = reinterpret_cast<const float*>(kargs_lds_ + KARG_ROW_);
#else
                const float* const srow = reinterpret_cast<const float*>(kargs_ + KARG_ROW_ * 4u);
#endif
                hitv = sun_start(srow, ro, S.bmin, S.bmax, sd, len, tn, tf);
            }
            else
            {
                const f3    dv = end - ro;
                const float d2 = dot(dv, dv);
                len = sqrt_(d2);
#ifdef VP_ARITH_FAST
                sd = dv * rsqrt_(d2);   // (the fast mode keeps its two instructions, v_sqrt_f32 and v_rsq_f32, and its bits)
#else
                sd = dv * rcp_(len);
#endif
                hitv = intersect_box(ro, sd, S, tn, tf);
            }
            if (!hitv)
            {
                nee_a = f3{1.0f, 1.0f, 1.0f};
                st    = EV_NEE;
            }
            else
            {
                if (tn < 0.0f) tn = 0.0f;
                t_end       = fminf(tf, len);
                dist        = tn;
                terms       = 0;
                rd          = sd;
                inv_sigma   = inv_s;
                cur_density = den;
                st          = ST_SHADOW;
                rng_saved = rng.enter_shadow(2u * (unsigned)(int)nsc + stage);
                if (COUNT) t_clip = 1e30f;
                if (RNG::kShadowSubstream && stage == 0u && L.sun_clip)
                {
                    // Beyond sun_clip[cell of ro] * clip_ds every fetch of this ray filters eight zero texels (sun_clip_k): no
                    // channel can terminate there any more, whatever is drawn, so the ray's result is known when it gets
                    // there.  Its draws come from a sub-stream of their own: nothing else depends on how many it makes.
                    f3    pl = to_local(S, ro);
                    int   ci, cj, ck;
                    float w_;
                    axis_linear(pl.x, S.nx, ci, w_);
                    axis_linear(pl.y, S.ny, cj, w_);
                    axis_linear(pl.z, S.nz, ck, w_);
                    const unsigned n = L.sun_clip[(size_t)((unsigned)ci + __umul24((unsigned)S.nx, (unsigned)cj + __umul24((unsigned)S.ny, (unsigned)ck)))];
                    if (n != 0xffffu)
                    {
                        const float tc = (float)n * L.clip_ds;
                        if (COUNT && !L.count_clips) t_clip = tc;
                        else t_end = fminf(t_end, tc);
                    }
                }
            }
        };
        // the path goes on with a new segment; loop bounds kernel.cu:34 with :2015 / :1332 / :1716
        // Local-majorant estimators: the Hyperion-reduced phase function and density of a segment (kernel.cu:2038-2046)
        // depend on the scatter count only, which restarts do not change: set where the count changes, not per restart.
        auto segment_medium = [&]() __attribute__((always_inline)) {
            if (LOCAL && TAB) cur_density = coll_row(nsc - 5)[CR_DENS];   // (the phase parameter: read from the row at the collision)
            else if (LOCAL)
            {
                float s         = hyperion_s(nsc - 5);
                phase_g         = (1.0f - s) * P.g;
                float reduction = (1.0f - s) + s * (1.0f - P.g);
                cur_density     = TRK ? reduction * sig_base : reduction * density;  // scalar build: the coefficient itself (:2063)
            }
        };
        auto next_segment = [&]() __attribute__((always_inline)) {
            st = ST_SETUP;
            if (LOCAL) dist = -1.0f;
            if (EXITC) terms = L.exit_start;
            if (EST == EST_GLOBAL) nsc = nsc + 1;
            if (EST == EST_BOUNDED) seg++;
            if ((EST == EST_BOUNDED ? seg : nsc) >= 800) st = EV_WRITE;
            segment_medium();
        };
        // EARLY: the light estimate is known without a shadow ray (optical-depth table, or the ray misses the box)
        auto finish_light = [&]() __attribute__((always_inline)) {
            if (DEFER) rad = rad + sun_power * ((ACH ? f3{lw_x, lw_x, lw_x} : f3{lw_x, lw_y, lw_z}) * nee_a);
            else rad = rad + sun_power * (((ACH ? f3{thr.x, thr.x, thr.x} : thr) * ph) * nee_a);
            rd  = pd;
            next_segment();
        };
        // ---- DEFER: the sun's light of a shadow ray that ended in the tracking loop.  light_done() left the ray's termination bits;
        // the sum is made here, for every lane that has one pending (lanes that ride along included), with the expression and the
        // order of operations it had at the ray's end: thr does not change during a shadow ray, so lw holds the bits of the product
        // formed there, and nothing adds to `rad` between the ray's end and this visit.  Before the collision block (whose
        // finish_light() adds to `rad`), the exit-flight test and the path-end chain.  A zero transmittance is not skipped: inf * 0.
        if (DEFER)
        {
            const unsigned lb = light_bits;
            if (lb != LIGHT_NONE)
            {
                const int tb = (int)lb;
                const f3  na = f3{(float)(1 - (tb & 1)), (float)(1 - ((tb >> 1) & 1)), (float)(1 - ((tb >> 2) & 1))};   // kernel.cu:807
                rad          = rad + sun_power * ((ACH ? f3{lw_x, lw_x, lw_x} : f3{lw_x, lw_y, lw_z}) * na);
                light_bits   = LIGHT_NONE;
            }
        }
        // ---- collision: direct lighting set-up (kernel.cu:2161-2217 / :1458-1491)
        tally(B_SCATTER, st == EV_SCATTER);
        if (!LIGHT && st == EV_SCATTER)
        {
            vp_pad<VP_PAD_COLL>();
            if (COUNT) c_sca++;
            if (PROF) zrun = 0;
            if (PARK) ro = ro + rd * dist;   // the collision point: the lane parked with the step's ro, rd and dist (or distc)
            t_empty = 0.0f;  // the certificate is for the unscattered camera ray only
            if (LOCAL) nsc = nsc + 1;  // num_scatters += !through, kernel.cu:2146
            // "to match passive result": post-increment count (DECOMP :2168) / i-4 (GLOBAL :1465)
            // TAB: row n2 is the shadow ray's medium and the next segment's (the global majorant's depth index is one higher then,
            // the local estimators' count is the one just incremented); row n2 - 1 is the one this segment's phase_g was set from
            const int          n2   = LOCAL ? (nsc - 5) : (nsc - 4);
            const float* const row2 = coll_row(n2);
            const float* const rowp = coll_row(n2 - 1);
            float s2 = hyperion_s(n2);
            float dp2, stp2;
            if (TAB)
            {
                dp2  = row2[CR_DENS];
                stp2 = LOCAL ? row2[CR_STP] * d_max : row2[CR_STP];  // quirk Q4: the local majorant for the whole shadow ray
            }
            else if (TRK)
            {
                thr  = thr * f3{P.albedo[0], P.albedo[1], P.albedo[2]};  // kernel.cu:2157-2159
                stp2 = LOCAL ? ((1.0f - s2) + s2 * (1.0f - P.g)) * sig_base : (1.0f - s2) * sig_base + s2 * sig_base * (1.0f - P.g);
                dp2  = stp2;  // Tr(..., inv_sigma, sigma_t_prime, rng): the coefficient is the "density" of the shadow ray
            }
            else if (LOCAL)
            {
                float reduction2 = (1.0f - s2) + s2 * (1.0f - P.g);
                dp2              = reduction2 * density;
                stp2             = max_sig * dp2 * d_max;  // quirk Q4: the local majorant for the whole shadow ray
            }
            else
            {
                dp2  = (1.0f - s2) * density + s2 * density * (1.0f - P.g);
                stp2 = max_sig * dp2;
            }
            const float phv = TAB ? hg_eval_row(rowp, dot(rd, sun_dir)) : hg_eval(phase_g, dot(rd, sun_dir));
            if (DEFER)
            {
                lw_x = thr.x * phv;
                if (!ACH) { lw_y = thr.y * phv; lw_z = thr.z * phv; }
            }
            else ph = phv;
            pd = rd;
            if (EARLY)
            {
                // the direction the path takes up when the light estimate is in (kernel.cu:2301-2303).  In-range roots (vp_math.h):
                // rd is the camera ray's normalize_ieee or an earlier collision's pd, i.e. the output of a normalize -- the frame's
                // tangent has its range from that (vp_device.h Frame); the sampled vector is a unit local vector (sin^2 + cos^2 of
                // hg_sample_local, 1 +- 2e-7) in a frame that is orthonormal to a few 1e-7, so its squared length is 1 +- 1e-5:
                // inside rsqrt_unit_'s [2^-8, 2]
                Frame fr(rd, UnitNormal{});
                float r0 = rng.next_a();
                float r1 = rng.next_b();
                pd       = normalize_unit(fr.to_world(TAB ? hg_sample_local_row(rowp, r0, r1) : hg_sample_local(phase_g, r0, r1)));
                if (LOCAL) { const f3 pdv = pd; inv_rd = f3{rcp_(pdv.x), rcp_(pdv.y), rcp_(pdv.z)}; }
            }
            if (MIS)
            {
                sh_inv_sigma = rcp_(stp2);
                sh_density   = dp2;
                nee_stage    = 0;
                nee_c        = sun_power;
                nee_t        = (ACH ? f3{thr.x, thr.x, thr.x} : thr) * phv;
            }
            // here ro already holds the collision point (set at the top of this block, or by the tracking step)
            if (EST == EST_DECOMP && frame > 10 && nsc > 20)
            {
                // precomputed optical depth kernel.cu:2183-2189 (quirk Q5)
                // (the packed copy always exists: where the device could not hold it -- 8x the table -- it lies in pinned host memory)
                float op = sample_float_cells(S, S.opacity_cells, ro);   // = sample_float_volume(S, S.opacity, ro), from one line of the packed copy
                if (COUNT) c_opa++;
                if (TRK)
                {
                    float a = expf_(-stp2 * op);  // kernel.cu:2190
                    nee_a   = f3{a, a, a};
                }
                else if (ACH)
                {
                    float a = expf_(((-sig_t.x) * dp2) * op);  // the three channels are the same expression
                    nee_a   = f3{a, a, a};
                }
                else
                {
                    f3 tau = (f3{-sig_t.x, -sig_t.y, -sig_t.z} * dp2) * op;
                    nee_a  = f3{expf_(tau.x), expf_(tau.y), expf_(tau.z)};
                }
                st     = EV_NEE;
                if (EARLY) finish_light();
            }
            else
            {
                start_shadow(sun_dir * 1e10f, (TAB && !LOCAL) ? row2[CR_INV] : rcp_(stp2), dp2, 0u);
                if (EARLY && st == EV_NEE) finish_light();   // the ray misses the box
                if (EARLY && EST == EST_GLOBAL && st == ST_SHADOW)
                {
                    // the set-up of the next segment (kernel.cu:1332-1345) for the new direction, while the lane is here anyway:
                    // where it enters (kept in t_empty, which is 0 for a scattered path and not read by shadow steps) and leaves
                    // the box (t_far; negative = it does not: the path ends with the environment)
                    float tn2, tf2;
                    bool  hit2 = intersect_box(ro, pd, S, tn2, tf2);
                    t_empty    = tn2 < 0.0f ? 0.0f : tn2;
                    t_far      = hit2 ? tf2 : -1.0f;
                    // TAB: ... and its medium, which is the shadow ray's (row n2: cur_density and inv_sigma are set by start_shadow);
                    // the two values below are read by primary steps only, so light_done() has nothing left to compute
                    if (TAB) { sigma_t_prime = row2[CR_STP]; inv_sigma_t = row2[CR_INV]; }
                }
            }
        }
#pragma unroll
        for (int pass = 0; pass < (MIS ? 2 : 1); pass++)
        {
            // ---- a light estimate is complete (kernel.cu:2188-2189,:2209-2210 and :2254,:2290)
            tally(B_NEE, st == EV_NEE);
            if (!LIGHT && !EARLY && st == EV_NEE)
            {
                if (MIS)
                {
                    rad = rad + nee_c * (nee_t * nee_a);
                    st  = nee_stage == 0 ? EV_MIS : EV_HG;
                }
                else
                {
                    rad = rad + sun_power * (((ACH ? f3{thr.x, thr.x, thr.x} : thr) * ph) * nee_a);
                    st  = EV_HG;
                }
            }
            // ---- one-sample MIS of the environment (kernel.cu:2220-2297; same block at :1494-1560 and :1855-1932)
            if (MIS && st == EV_MIS)
            {
                const float P_phase = 0.5f, P_envmap = 1.0f - P_phase;
                const f3    thr3    = ACH ? f3{thr.x, thr.x, thr.x} : thr;
                Frame       fr(pd);
                nee_stage = 1;
                if (rng.next_a() < P_phase)
                {
                    float u        = rng.next_a();
                    float v        = rng.next_b();
                    f3    brdf_dir = fr.to_world(hg_sample_local(phase_g, u, v));
                    f3    envc     = eval_envmap(S, brdf_dir);
                    if (COUNT) c_env++;
                    float pdf_brdf        = hg_eval(phase_g, dot(fr.n, brdf_dir));
                    float pdf_env_virtual = luminance(envc) * S.env_pdfnorm_alt;  // pdf_envmap :1009-1034
                    float wa = pdf_brdf * P_phase, wb = pdf_env_virtual * P_envmap;
                    float weight = wa / (wa + wb) / P_phase;
                    nee_c = envc;
                    nee_t = thr3 * weight;
                    start_shadow(brdf_dir * 1e10f, sh_inv_sigma, sh_density, 1u);
                }
                else
                {
                    float u = rng.next_a();
                    float v = rng.next_b();
                    f3    envc;
                    float pdf_env = sample_envmap(S, u, v, envc);
                    if (COUNT) c_env++;
                    if (pdf_env <= 0.0f)
                    {
                        // the reference `continue`s here (:2266): no scattered direction, the OLD ray goes on
                        ro = seg_o;
                        rd = pd;
                        next_segment();
                    }
                    else
                    {
                        f3    envmap_dir       = uv_to_dir(u, v);
                        float pdf_brdf_virtual = hg_eval(phase_g, dot(fr.n, envmap_dir));
                        float wa = pdf_env * P_envmap, wb = pdf_brdf_virtual * P_phase;
                        float weight = wa / (wa + wb) / P_envmap;
                        nee_c = envc;
                        nee_t = ((thr3 * pdf_brdf_virtual) / pdf_env) * weight;
                        start_shadow(envmap_dir * 1e10f, sh_inv_sigma, sh_density, 1u);
                    }
                }
            }
        }
        // ---- phase-function sampling (kernel.cu:2301-2303)
        tally(B_HG, st == EV_HG);
        if (!LIGHT && !EARLY && st == EV_HG)
        {
            Frame fr(pd, UnitNormal{});   // (pd: the colliding ray's direction, the output of a normalize; ranges as in the collision block)
            float r0 = rng.next_a();
            float r1 = rng.next_b();
            // (TAB: the row phase_g was set from -- the count has not moved since the collision)
            rd       = normalize_unit(fr.to_world(TAB ? hg_sample_local_row(coll_row((LOCAL ? (nsc - 5) : (nsc - 4)) - 1), r0, r1) : hg_sample_local(phase_g, r0, r1)));
            if (LOCAL) inv_rd = f3{rcp_(rd.x), rcp_(rd.y), rcp_(rd.z)};
            next_segment();
        }
        // ---- exit flights: can this path do anything but leave the box?  Lanes in flight whose counter has tripped ride along.
        if (EXITC)
        {
            const bool cand = (st == ST_TRACK || (LOCAL && st == ST_SETUP)) && terms >= VP_EXIT_TRIP;
            tally(B_EXITT, cand);
            if (cand)
            {
                if (COUNT) c_xtest++;
                // (1) the cells: every fetch the ray can still make lies in the quarter pyramid of cells that opens from its cell
                // along the dominant axis of its direction, toward the sides the other two components point to; the table says
                // whether every cell of that pyramid is empty with empty neighbours (exit_dir_slice_k)
                const f3 pl = to_local(S, st == ST_TRACK ? ro + rd * dist : ro);
                int   ci, cj, ck;
                float w_;
                axis_linear(pl.x, S.nx, ci, w_);
                axis_linear(pl.y, S.ny, cj, w_);
                axis_linear(pl.z, S.nz, ck, w_);
                // the direction in cell units, its dominant axis A and the signs (A, then the other two in increasing order)
                const float ex = rd.x * (S.linv[0] * (float)S.nx), ey = rd.y * (S.linv[1] * (float)S.ny), ez = rd.z * (S.linv[2] * (float)S.nz);
                const float ax = __builtin_fabsf(ex), ay = __builtin_fabsf(ey), az = __builtin_fabsf(ez);
                const unsigned A   = (ax >= ay && ax >= az) ? 0u : (ay >= az ? 1u : 2u);
                const unsigned cls = A == 0u ? ((ex > 0.0f ? 1u : 0u) | (ey > 0.0f ? 2u : 0u) | (ez > 0.0f ? 4u : 0u))
                                   : A == 1u ? ((ey > 0.0f ? 1u : 0u) | (ex > 0.0f ? 2u : 0u) | (ez > 0.0f ? 4u : 0u))
                                             : ((ez > 0.0f ? 1u : 0u) | (ex > 0.0f ? 2u : 0u) | (ey > 0.0f ? 4u : 0u));
                const size_t   ncell = (size_t)S.nx * (size_t)S.ny * (size_t)S.nz;
                const unsigned bits  = L.exit_oct[(size_t)A * ncell + (size_t)((unsigned)ci + __umul24((unsigned)S.nx, (unsigned)cj + __umul24((unsigned)S.ny, (unsigned)ck)))];
                bool clear = (bits >> cls) & 1u;
                // (2) the throughput: every majorant a null collision can meet on the way must leave it as it is: the segment's own
                // (global majorant); that of every byte that occurs as a maximum in the bound table (local majorants: a segment
                // through empty cells may still lie in a brick with a positive maximum)
                bool unit = true;
                if (clear)
                {
                    const f3 t3 = ACH ? f3{thr.x, thr.x, thr.x} : thr;
                    if (LOCAL)
                    {
                        for (unsigned q = 0; q < L.exit_nbytes; q++)
                        {
                            const float dm  = fmaxf(0.0001f, (float)((L.exit_bytes >> (8u * q)) & 0xffu) * VP_U8_SCALE);   // segment_setup()
                            const float stp = max_sig * cur_density * dm;
                            unit = unit && null_collision_is_identity(t3, stp, rcp_(stp));
                        }
                    }
                    else
                        unit = null_collision_is_identity(t3, sigma_t_prime, inv_sigma_t);
                }
                if (COUNT && clear && unit) c_xok++;
                if (clear && unit && !(COUNT && !L.count_clips)) st = EV_BG;
                else
                {
                    // not (yet): the next test comes after another K null collisions in empty space -- much later where the throughput
                    // was the obstacle (it moves by an ulp per null collision until it meets a fixed point of the factor).  The counting
                    // build walks on (its density_lookups are the estimator's) and stops counting loads.
                    if (COUNT && clear && unit) ex_clear = true;
                    terms = (clear && unit) ? -(1 << 30) : (unit ? L.exit_start : L.exit_start - 4 * VP_EXIT_TRIP);
                }
            }
        }
        // Path ends (environment, write, refill, and the global-majorant set-up of a fresh sample) come one or two lanes at a time:
        // the ~300 instructions of this chain are not run in every visit for them.  They wait -- an idle lane or two -- until
        // end_lanes lanes ask, or four visits have passed, or nothing else is left to do in this wave.
        {
            const unsigned long long wantm = __ballot(st == EV_BG || st == EV_WRITE || (st == ST_DONE && !exhausted) || (EST == EST_GLOBAL && st == ST_SETUP));
            const bool fast_any = __ballot(st == ST_TRACK || st == ST_SHADOW || (LOCAL && st == ST_SETUP)) != 0ull;
            end_skipped++;
            if (wantm == 0ull || (!LIGHT && fast_any && (unsigned)__popcll(wantm) < L.end_lanes && end_skipped < 4u)) goto ends_done;
            end_skipped = 0u;
        }
#pragma unroll 1
        for (int rep = 0; rep < 4; rep++)
        {
            vp_pad<VP_PAD_END>();
            bool fresh = false;   // APPR: this lane took a new sample in this round, `dist` holds where approach_k left its camera ray
            bool trans = false;   // layers launch (LaunchDev::layers): the path that ends in this round is unscattered -- its sample is its throughput
            // groups launch (LaunchDev::groups): what the environment adds to the path that ends in this round -- the sky group's sample;
            // nothing for a path that ends without it (the segment cap) or inside the sun's disc, whose value is the sun group's
            f3   sky    = f3{0.0f, 0.0f, 0.0f};
            bool to_sky = false;
            // RAYT: this lane took a new sample in this round and read its camera ray and box test from the per-pixel table (L.ray:
            // ray_table_k, the bits camera_ray() and intersect_box() compute): the set-up below takes t_near and t_far from there
            bool  tabfed = false;
            float tab_near = 0.0f, tab_far = 0.0f;
            // order: a path that ends here is written, its lane refilled and the new segment set up in ONE round
            // ---- ray left the medium: background() kernel.cu:1258-1267 (quirk Q11)
            tally(B_BG, st == EV_BG);
            if (st == EV_BG)
            {
                // with active environment sampling only unscattered paths see it directly (kernel.cu:2026-2030, :1340-1344)
                if (!MIS || nsc == 0)
                {
                    // (a layers launch: an unscattered path's sample is the transmittance layer's, its throughput -- the sum below with a
                    // background of 1 --, marked for the reduce in EV_WRITE; include/volpath.h vp_render_frames_layers)
                    if (LAYERS) trans = nsc == 0;
                    f3 bg;
                    if (LAYERS && trans) bg = f3{1.0f, 1.0f, 1.0f};
                    else if (nsc == 0 && dot(rd, sun_dir) > S.sun_cos) bg = f3{S.sun_orig[0], S.sun_orig[1], S.sun_orig[2]};
                    else { bg = eval_envmap(S, rd); if (COUNT) c_env++; if (GRP) to_sky = true; }
                    if (LIGHT && !LOCAL)
                    {
                        // throughput after `seg` null collisions in empty space (see tracking_step)
                        const unsigned n = (unsigned)seg, last = L.thr_n - 1u;
                        float t = L.thr_table[n < last ? n : last];
                        for (unsigned k = last; k < n; k++) t = null_collision_in_empty_space(t, sigma_t_prime, inv_sigma_t);
                        thr = f3{t, t, t};
                    }
                    // (a groups launch: the sum a render without the sun makes here, from +0 -- include/volpath.h vp_render_frames_groups)
                    // (the light class, whose path has summed nothing: the sum stays in `rad` and EV_WRITE routes the sample -- two registers
                    // and, local majorants, the eighth wave: profiles/groups_kernel_resources.txt)
                    if (GRP && !LIGHT && to_sky) sky = sky + bg * (ACH ? f3{thr.x, thr.x, thr.x} : thr);
                    else rad = rad + bg * (ACH ? f3{thr.x, thr.x, thr.x} : thr);
                }
                st = EV_WRITE;
            }
            // ---- path end: emit the sample (kernel.cu:2306-2316 / :1579-1589)
            tally(B_WRITE, st == EV_WRITE);
            if (st == EV_WRITE)
            {
                f3     r    = rad * ((LAYERS && trans) ? 1.0f : P.brightness);
#ifdef VP_ARITH_FAST
                // v_rcp_f32 / v_rsq_f32 / v_log_f32 flush denormal inputs: the collision weight of a path whose throughput has sunk
                // below 2^-126 can come out infinite where the IEEE quotient is finite.  Such a path carries ~1e-38 of the light it
                // sees: it is written as 0 rather than poisoning the accumulator (NaN already is, by the fmaxf below).
                r = f3{r.x < __builtin_inff() ? r.x : 0.0f, r.y < __builtin_inff() ? r.y : 0.0f, r.z < __builtin_inff() ? r.z : 0.0f};
#endif
                // heat: num_scatters (:2307) or loop index * 0.001 in double (:1581, :1942)
                float  heat = (EST == EST_DECOMP) ? (float)nsc : (float)((double)(EST == EST_BOUNDED ? seg : nsc) * 0.001);
                // (never negative otherwise: the sign bit, -0.0f included, marks a transmittance sample.  Not in the light kernels: every
                // sample of theirs is one, the reduce knows their slots, and the mark costs the local-majorant ones two registers
                // and their eighth wave: profiles/layers_kernel_resources.txt)
                if (LAYERS && !LIGHT && trans) heat = -heat;
                float4 v    = make_float4(fmaxf(r.x, 0.0f), fmaxf(r.y, 0.0f), fmaxf(r.z, 0.0f), heat);
                if (TRK == 2)  // kernel.cu:2311-2313: the drawn channel only, times three
                    v = make_float4(chan == 0 ? v.x * 3.0f : 0.0f, chan == 1 ? v.y * 3.0f : 0.0f, chan == 2 ? v.z * 3.0f : 0.0f, heat);
                // (a group-layers launch, LYR and GRP: a marked sample and every sample of the light class is a transmittance sample, whose
                // second-plane word the reduce (split_sample) derives -- the light instances are the layers launch's code, the general ones
                // stage the sky group's sample of a scattered path only)
                if (GRP && LIGHT && !LYR)
                {
                    // every sample of the light class is the environment's term alone: it is one group's whole, the other gets (0, 0, 0, heat)
                    // (selects per channel: a select between two float4 objects goes through scratch)
                    L.groups[item] = make_float4(to_sky ? v.x : 0.0f, to_sky ? v.y : 0.0f, to_sky ? v.z : 0.0f, heat);
                    v              = make_float4(to_sky ? 0.0f : v.x, to_sky ? 0.0f : v.y, to_sky ? 0.0f : v.z, heat);
                }
                else if (GRP && !LIGHT && !(LAYERS && trans))
                {
                    // the sky group's sample beside the sun group's: the beauty sample's operations on `sky` (a groups launch is staged)
                    const f3 k = sky * P.brightness;
                    L.groups[item] = make_float4(fmaxf(k.x, 0.0f), fmaxf(k.y, 0.0f), fmaxf(k.z, 0.0f), heat);
                }
                if (L.stage) L.stage[item] = v;
                else
                {
                    size_t idx = (size_t)px + (size_t)py * P.width;
                    float4 a   = L.out[idx];
                    L.out[idx] = make_float4(a.x + v.x, a.y + v.y, a.z + v.z, a.w + v.w);
                }
                st = ST_DONE;
            }
            // ---- refill finished lanes from the queue.  The wave owns a chunk of samples (chunk_s .. chunk_n)
            // of consecutive samples (one atomic per VP_CHUNK samples); idle lanes are compacted
            // with ballot + mbcnt and take the next samples of the chunk.
            {
                bool               need = (st == ST_DONE) && !exhausted;
                unsigned long long m    = __ballot(need);
                tally(B_REFILL, need);
                if (m)
                {
                    while (chunk_s >= chunk_n && !queue_empty)
                    {
                        // queue q_cur: chunk c is frame (c % nframes) of chunk position (c / nframes) of its band -- the waves
                        // running at the same time work on the same few tiles in different frames, i.e. on rays through the
                        // same pencil of the volume
                        // A chunk is (VP_CHUNK >> chunk_fshift) consecutive pixels of the band x (1 << chunk_fshift) consecutive frames
                        // (the host sets chunk_fshift = 0 unless the frame count is a multiple): sample s of it is pixel s >> shift,
                        // frame s & mask -- with shift 6 a wave starts on ONE pixel in 64 frames: the same camera ray in every lane.
                        const unsigned q0 = L.q_start[q_cur], len = L.q_start[q_cur + 1] - q0;
                        static_assert((VP_CHUNK & (VP_CHUNK - 1)) == 0 && VP_CHUNK >= 64, "VP_CHUNK: a power of two, at least a wave");
                        const unsigned sh = L.chunk_fshift, ppc = (unsigned)VP_CHUNK >> sh, fblocks = (unsigned)L.nframes >> sh;   // (the host keeps sh <= log2(VP_CHUNK): ppc >= 1)
                        const unsigned cpf = (len + ppc - 1u) / ppc;
                        unsigned c = 0xffffffffu;
                        if (len)
                        {
                            // (a cancelled look-ahead batch hands out nothing more: an atomic load at agent scope, so that the host's write from
                            // another stream is seen whichever XCD this wave runs on)
                            if (lane == 0 && !(L.cancel && __hip_atomic_load(L.cancel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= L.batch_id)) c = atomicAdd(L.queue + q_cur * VP_QUEUE_STRIDE, 1u);
                            c = __builtin_amdgcn_readfirstlane(c);
                        }
                        if (c < cpf * fblocks)
                        {
                            const unsigned pos = c / fblocks, fb = c - pos * fblocks, off = pos * ppc;
                            chunk_q  = q0 + off;
                            chunk_f0 = fb << sh;
                            chunk_n  = (len - off < ppc ? len - off : ppc) << sh;
                            chunk_s  = 0;
                        }
                        else
                        {
                            // this band is handed out: help with the next one
                            q_cur = (q_cur + 1) & (VP_NQUEUES - 1);
                            if (++q_tried >= VP_NQUEUES) queue_empty = true;
                        }
                    }
                    unsigned cnt   = (unsigned)__popcll(m);
                    unsigned avail = chunk_n - chunk_s;
                    unsigned take  = cnt < avail ? cnt : avail;
                    unsigned rank  = lane_rank(m);
                    if (need)
                    {
                        if (rank >= take) { if (queue_empty) exhausted = true; /* else: next chunk, next round */ }
                        else
                        {
                            const unsigned sn  = chunk_s + rank, sh = L.chunk_fshift;
                            const unsigned rem = chunk_q + (sn >> sh);              // sample slot of this class within the frame
                            const unsigned fl  = chunk_f0 + (sn & ((1u << sh) - 1u));
                            item = fl * L.stage_stride + L.slot_base + rem;
                            unsigned pix = L.pixels[rem];
                            px    = pix & 0xffffu;
                            py    = pix >> 16;
                            frame = L.frame0 + (int)fl;
                            if (px < P.width && py < P.height)
                            {
                                // the pixel the sample is computed for: this one, or with a sub-pixel factor (L.sub_shift) one of the
                                // S x S pixels of the S W x S H image that tile it -- stream, camera ray and table entries are that
                                // pixel's; item, px, py (where the sample is written) stay this one's.  A block of its own, and the table
                                // index recomputed where it is read (a handful of integer instructions per sample), so that the path
                                // without a factor keeps the code it had.  (The counting instances carry no code for it: the host refuses
                                // work counters with a factor, vp_tables.cpp subpixel_check.)
                                auto table_index = [&]() -> size_t
                                {
                                    if (!COUNT && L.sub_shift)
                                    {
                                        unsigned si, sj;
                                        subpixel_offset(px, py, (unsigned)frame, L.sub_shift, si, sj);
                                        return (size_t)((px << L.sub_shift) + si) + (size_t)((py << L.sub_shift) + sj) * (P.width << L.sub_shift);
                                    }
                                    return (size_t)px + (size_t)py * P.width;
                                };
                                // camera ray, kernel.cu:1977-1987 (quirk Q3: the same ray in every frame unless a sub-pixel factor is set)
                                float tab_te = 0.0f;
                                if (!COUNT && L.sub_shift)
                                {
                                    unsigned si, sj;
                                    subpixel_offset(px, py, (unsigned)frame, L.sub_shift, si, sj);
                                    const unsigned fx = (px << L.sub_shift) + si, fy = (py << L.sub_shift) + sj;
                                    rng.init(fx, fy, (unsigned)frame, L.key0, L.key1);
                                    camera_ray(S, P.width << L.sub_shift, P.height << L.sub_shift, fx, fy, ro, rd);
                                }
                                else
                                {
                                    rng.init(px, py, (unsigned)frame, L.key0, L.key1);
                                    const float4* const ray = RAYT ? L.ray : nullptr;
                                    if (RAYT && ray)
                                    {
                                        // the pixel's entries (slot order, as `pixels`): two divisions, a root and nine multiply-adds of
                                        // camera_ray(), and the box test of the set-up below, done once per view instead of per sample
                                        const float4 e0 = ray[2 * (size_t)rem], e1 = ray[2 * (size_t)rem + 1];
                                        ro       = f3{S.cam[3], S.cam[7], S.cam[11]};
                                        rd       = f3{e0.x, e0.y, e0.z};
                                        tab_near = e0.w;
                                        tab_far  = e1.x;
                                        tab_te   = e1.y;
                                        tabfed   = true;
                                    }
                                    else camera_ray(S, P.width, P.height, px, py, ro, rd);
                                }
                                if (TRK == 2)
                                {
                                    chan     = (int)fminf((1.0f - rng.next_a()) * 3.0f, 2.9999998f);  // kernel.cu:1993
                                    sig_base = density * (chan == 0 ? P.sigma_t[0] : chan == 1 ? P.sigma_t[1] : P.sigma_t[2]);
                                }
                                if (LOCAL) inv_rd = f3{1.0f / rd.x, 1.0f / rd.y, 1.0f / rd.z};   // (the camera ray: IEEE in both modes)
                                thr = f3{1.0f, 1.0f, 1.0f};
                                rad = f3{0.0f, 0.0f, 0.0f};
                                nsc = 0;
                                seg = 0;
                                if (EXITC) terms = L.exit_start;
                                if (COUNT) ex_clear = false;
                                if (RAYT && tabfed) t_empty = tab_te;
                                else if (!LIGHT) t_empty = L.crawl ? L.crawl[2 * table_index() + 1].x : 0.0f;
                                if (LOCAL) dist = -1.0f;   // a segment starts where the ray enters it (segment_setup), unless approach_local_k got further
                                if (APPR && L.approach)
                                {
                                    const float4 a = L.stage[item];   // approach_k: distance reached, where the stream stands, steps made
                                    dist  = a.x;
                                    rng.load(f2u(a.y), f2u(a.z));
                                    fresh = true;
                                    if (L.approach == 2u)
                                    {
                                        // a medium whose null collision in empty space is not exactly neutral: the throughput after the
                                        // walk's n of them is the n-th iterate of one function of one float (thr_table_k, as the light
                                        // kernel of this estimator looks it up; beyond the table the recurrence is run)
                                        const unsigned n = f2u(a.w), last = L.thr_n - 1u;
                                        float t = L.thr_table[n < last ? n : last];
                                        if (n > last)
                                        {
                                            const float s0  = hyperion_s(0 - 5);
                                            const float stp = max_sig * ((1.0f - s0) * density + s0 * density * (1.0f - P.g));
                                            const float inv = rcp_(stp);
                                            for (unsigned k = last; k < n; k++) t = null_collision_in_empty_space(t, stp, inv);
                                        }
                                        thr = f3{t, t, t};
                                    }
                                }
                                if (LOCAL && L.crawl)
                                {
                                    // the restart crawl in front of the volume, done once per pixel by crawl_table_k: the path starts
                                    // where that crawl ends, with its draws skipped and its segments counted
                                    float4   c = L.crawl[2 * table_index()];
                                    unsigned k = f2u(c.w);
                                    ro = f3{c.x, c.y, c.z};
                                    if (!(APPR_L && L.approach)) rng.skip(k >> 16);   // (else the hand-over below carries the stream's state)
                                    if (EST == EST_BOUNDED) seg = (int)(k & 0xffffu);
                                    if (COUNT) c_bnd += k & 0xffffu;
                                    if (APPR_L && L.approach)
                                    {
                                        // approach_local_k walked on from there: origin of the first segment it did not finish, pairs used
                                        // so far.  The certificate is measured from the segment origin: less the distance walked (the
                                        // projection on the ray, a margin of 1e-4 against its rounding: a shorter certificate renders the
                                        // same bits, it only fetches a zero it could have skipped)
                                        const float4 a  = L.stage[item];
                                        const uint2  ax = L.approach_aux[item];
                                        const f3     ra = f3{a.x, a.y, a.z};
                                        t_empty = t_empty - dot(ra - ro, rd) - 1e-4f;
                                        ro      = ra;
                                        // how far into the segment at ra the walk got (-1: not at all): the set-up below keeps it
                                        dist    = a.w;
                                        // where the stream stands: the pair index, or sampler.h's two words
                                        rng.load(ax.x, ax.y);
                                    }
                                }
                                st  = ST_SETUP;
                                segment_medium();
                                if (COUNT) c_smp++;
                            }
                            // pixels of a partial edge tile outside the image: nothing to do, stay DONE
                        }
                    }
                    chunk_s += take;
                }
            }
            // ---- global-majorant segment set-up (__d_render kernel.cu:1332-1370); rare, so it lives here
            if (EST == EST_GLOBAL) tally(B_GSETUP, st == ST_SETUP);
            if (EST == EST_GLOBAL && st == ST_SETUP)
            {
                // (a lane fresh from the ray table: the raw outputs of the same call, and its two compares; the others -- no table, or
                // the non-EARLY instances' next_segment() -- compute it.  A branch, not a select: a round whose set-up lanes are all
                // table-fed skips the box test with an empty exec mask)
                float t_near, tf;
                bool  hit;
                if (RAYT && tabfed) { t_near = tab_near; tf = tab_far; hit = tf > t_near && tf >= 1e-3f; }
                else hit = intersect_box(ro, rd, S, t_near, tf);
                if (!hit) st = EV_BG;
                else
                {
                    if (t_near < 0.0f) t_near = 0.0f;
                    t_far         = tf;
                    t_end         = tf;
                    dist          = (APPR && fresh) ? dist : t_near;
                    float s       = hyperion_s(nsc - 5);
                    if (!TAB) phase_g = (1.0f - s) * P.g;
                    if (TAB)
                    {
                        const float* const row = coll_row(nsc - 5);
                        cur_density   = row[CR_DENS];
                        sigma_t_prime = row[CR_STP];
                    }
                    else if (TRK)
                    {
                        sigma_t_prime = (1.0f - s) * sig_base + s * sig_base * (1.0f - P.g);  // kernel.cu:1363
                        cur_density   = sigma_t_prime;  // vol_sigma_t(pos, sigma_t_prime), kernel.cu:1436
                    }
                    else
                    {
                        cur_density   = (1.0f - s) * density + s * density * (1.0f - P.g);
                        sigma_t_prime = max_sig * cur_density;
                    }
                    inv_sigma     = TAB ? coll_row(nsc - 5)[CR_INV] : rcp_(sigma_t_prime);
                    inv_sigma_t   = inv_sigma;
                    st            = ST_TRACK;
                }
            }
            // another round only for lanes this loop can serve: idle ones, and new samples that missed the volume
            if (__ballot((st == ST_DONE && !exhausted) || st == EV_BG || st == EV_WRITE) == 0ull) break;
        }
ends_done:
        // CANCEL: the instance look-ahead batches run (render_kernel's staged frames, LaunchDev::cancel).  A batch the host has dropped --
        // a camera move, a setter -- is of no use to anybody: every wave asks at every eighth event visit (a visit comes every ~15 us)
        // and gives up its paths at once instead of tracing them to their ends, which is what the move would otherwise wait for (the
        // deepest paths in flight: ~10 ms).  Nothing reads what such a batch has staged.  An instance of its own because the test,
        // small as it is, reshuffles the registers of the batched global-majorant kernel to the tune of -4...-5.5 %
        // (profiles/experiments/r04_lookahead_cancel.txt).
        if (CANCEL && L.cancel && (visits++ & 7u) == 0u)
        {
            unsigned w = 0;
            if (lane == 0) w = __hip_atomic_load(L.cancel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (a load at agent scope, not a read-modify-write: ADVICE r4)
            if ((unsigned)__builtin_amdgcn_readfirstlane((int)w) >= L.batch_id) { st = ST_DONE; exhausted = true; queue_empty = true; }
        }
        if (__ballot(st != ST_DONE || !exhausted) == 0ull) break;  // queue drained and every lane idle
        }
        if (PROF) { unsigned long long t = __builtin_amdgcn_s_memtime(); if (lane == 0) t_slow += t - t_mark; t_mark = t; }

        // =========================================================== fast path: tracking
        // one segment set-up (local-majorant estimators) and one tracking step, as lambdas: the loop below runs
        // them twice per pass so that the wave-level bookkeeping (ballots, wait policy) is paid once per two steps
        // Global majorant: which lanes are in which fast state is kept in wave masks while the loop runs -- formed here from `st`, one
        // ballot each; from then on every "is this lane TRACK / SHADOW" is the lane's bit of a mask (lane_in: the branch's exec operand,
        // no vector instruction) and the loop's exit test is scalar arithmetic on them.  `st` stays complete all the while: a lane
        // writes its new code once, where it leaves a state (set_code); a lane that stays writes nothing.
        // The masks are formed anew after each step's divergent body, in UNIFORM control flow, never inside it (there the compiler
        // keeps them per lane, in vector registers): by one compare of `st` per mask.  Without any -- flags set where a lane leaves
        // and balloted after the body, or the step's blocks side by side under masks of compares made between them -- was tried:
        // this compiler widens a branch-carried flag to 0 / 1 and compares it again (two vector instructions per ballot), and the
        // side-by-side form costs the achromatic instance seven registers and its eighth wave.  The local-majorant estimators keep
        // the enum (MASKS false: their code is what it was): with masks 23 of their instances need 2-8 registers more and lose a wave
        // (profiles/experiments/fast_state_masks.txt).
        constexpr bool MASKS = !LOCAL;
        unsigned long long m_track = MASKS ? __ballot(st == ST_TRACK) : 0ull, m_shadow = MASKS ? __ballot(st == ST_SHADOW) : 0ull;
        // lanes that hold or want a sample (no lane becomes ST_DONE in the loop): those of them in no fast state wait for the event pass
        const unsigned long long m_live = MASKS ? __ballot(!(st == ST_DONE && exhausted)) : 0ull;
        auto in_track  = [&]() __attribute__((always_inline)) { return MASKS ? lane_in(m_track) : st == ST_TRACK; };
        auto in_shadow = [&]() __attribute__((always_inline)) { return MASKS ? lane_in(m_shadow) : st == ST_SHADOW; };
        auto in_flight = [&]() __attribute__((always_inline)) { return MASKS ? lane_in(m_track | m_shadow) : (st == ST_TRACK || st == ST_SHADOW); };
        auto segment_setup = [&]() __attribute__((always_inline)) {
            if (LOCAL) tally(B_SETUP, st == ST_SETUP);
            if (LOCAL && st == ST_SETUP)
            {
                vp_pad<VP_PAD_SETUP>();
                // intersectSuperVolume kernel.cu:1626-1661 (quirks Q6, Q10): the bound is fetched before the hit test
                float t_near, tf;
                bool  hit = intersect_box_inv(ro, inv_rd, S, t_near, tf);
                t_near    = fmaxf(t_near, 0.0f);
                t_far     = fminf(tf, 0.05f);
                float bx, by;
                if (LDSB)
                {
                    f3  pl = to_local(S, ro + rd * t_near);
                    int bi = axis_point(pl.x, S.nx) >> S.brick_shift;
                    int bj = axis_point(pl.y, S.ny) >> S.brick_shift;
                    int bk = axis_point(pl.z, S.nz) >> S.brick_shift;
                    const unsigned bidx = (unsigned)bi + __umul24((unsigned)S.bnx, (unsigned)bj + __umul24((unsigned)S.bny, (unsigned)bk));
                    unsigned v;
                    if (LDSB == 2)
                    {
                        // sixteen 2-bit codes per word; the palette's four byte pairs come with the launch
                        const unsigned code = (lds_codes[bidx >> 4] >> ((bidx & 15u) << 1)) & 3u;
                        const unsigned pal  = (code & 2u) ? L.bound_pal[1] : L.bound_pal[0];
                        v = (code & 1u) ? pal >> 16 : pal & 0xffffu;
                    }
                    else
                        v = lds_bounds[bidx];
                    bx = (float)(v & 0xffu) * VP_U8_SCALE;
                    by = (float)(v >> 8) * VP_U8_SCALE;
                }
                else
                    sample_bound<QUANT>(S, ro + rd * t_near, bx, by);
                if (COUNT) c_bnd++;
                float d_min = by;
                d_max       = fmaxf(0.0001f, bx);
                if (!hit) set_code<EV_BG, MASKS>(st);
                else
                {
                    // (where the free flight of this segment starts: where the ray enters it -- or, in the one segment approach_local_k
                    // handed over half-walked, where that walk got; every other set-up finds dist = -1)
                    dist          = fmaxf(dist, t_near);
                    // phase_g and cur_density of this scatter count: segment_medium().  Scalar build: no local bound (:2063 / :1745)
                    sigma_t_prime = TRK ? cur_density : max_sig * cur_density * d_max;
                    inv_sigma_t   = rcp_(sigma_t_prime);
                    if (PROF)
                    {
                        // (how often the control component's 65 instructions -- a draw, a logarithm, two divisions -- run, and for how many lanes)
                        const unsigned long long cm = __ballot(TRK == 0 && EST == EST_DECOMP && d_min > 0.0f);
                        if (cm) { ctrl_w += 1; ctrl_l += (unsigned)__popcll(cm); }
                    }
                    if (TRK == 0 && EST == EST_DECOMP && d_min > 0.0f)
                    {
                        // analog decomposition tracking kernel.cu:2048-2054 (quirk Q7)
                        sigma_c       = min_sig * cur_density * d_min;
                        distc         = dist - div_(logf_(rng.next_a()), fmaxf(sigma_c, 1e-20f));
                        float sigma_r = fmaxf(sigma_t_prime - sigma_c, 1e-20f);
                        inv_sigma     = rcp_(sigma_r);
                    }
                    else
                    {
                        distc     = 1e20f;
                        sigma_c   = 0.0f;
                        inv_sigma = inv_sigma_t;
                    }
                    t_end = fminf(distc, t_far);  // dist >= distc || dist >= t_far  (kernel.cu:2086)
                    set_code<ST_TRACK, MASKS>(st);
                }
            }
        };
        // EARLY: a shadow ray has ended (nee_a known): add the light and go on with the segment prepared in the collision block
        // (DEFER: it leaves the termination bits for the event pass, which adds the light -- no conversion, no read of the sun's power,
        // no sum here, where 5-10 of 64 lanes are active -- and goes on)
        auto light_done = [&]() __attribute__((always_inline)) {
#ifdef VP_EXP_FLAT_KARGS
            const char* ka_ = (const char*)__builtin_amdgcn_kernarg_segment_ptr();
            asm volatile("" : "+s"(ka_));   // the sun's power is read here, not held in scalar registers across the loop
#else
            unsigned ko2_ = 0;
            asm volatile("" : "+v"(ko2_));
            const char* ka_ = reinterpret_cast<const char*>(kargs_lds_) + ko2_;
#endif
            if (DEFER) light_bits = (unsigned)terms;
            else
            {
                const SceneDev& S2 = *reinterpret_cast<const SceneDev*>(ka_);
                const f3 sunp = f3{S2.sun_power[0], S2.sun_power[1], S2.sun_power[2]};
                rad = rad + sunp * (((ACH ? f3{thr.x, thr.x, thr.x} : thr) * ph) * nee_a);
            }
            rd  = pd;
            if (EXITC) terms = reinterpret_cast<const LaunchDev*>(ka_ + KARG_L_)->exit_start;
            if (EST == EST_GLOBAL)
            {
                nsc = nsc + 1;
                if (nsc >= 800) set_code<EV_WRITE, MASKS>(st);
                else if (t_far < 0.0f) { set_code<EV_BG, MASKS>(st); t_empty = 0.0f; }
                else
                {
                    // __d_render's segment set-up kernel.cu:1355-1370 for the depth index just reached
                    t_end         = t_far;
                    dist          = t_empty;
                    t_empty       = 0.0f;
                    float s       = hyperion_s(nsc - 5);
                    if (!TAB) phase_g = (1.0f - s) * P.g;
                    if (TAB)
                    {
                        // the medium of depth index nsc is the shadow ray's (cur_density, inv_sigma: still in place); sigma_t_prime
                        // and inv_sigma_t were set beside it in the collision block
                    }
                    else if (TRK)
                    {
                        sigma_t_prime = (1.0f - s) * sig_base + s * sig_base * (1.0f - P.g);
                        cur_density   = sigma_t_prime;
                    }
                    else
                    {
                        cur_density   = (1.0f - s) * density + s * density * (1.0f - P.g);
                        sigma_t_prime = max_sig * cur_density;
                    }
                    if (!TAB)
                    {
                        inv_sigma   = rcp_(sigma_t_prime);
                        inv_sigma_t = inv_sigma;
                    }
                    set_code<ST_TRACK, MASKS>(st);
                }
            }
            else
            {
                set_code<ST_SETUP, MASKS>(st);
                dist = -1.0f;
                if (EST == EST_BOUNDED) seg++;
                if ((EST == EST_BOUNDED ? seg : nsc) >= 800) set_code<EV_WRITE, MASKS>(st);
                if (TAB) cur_density = coll_row(nsc - 5)[CR_DENS];
                else
                {
                    float s         = hyperion_s(nsc - 5);
                    phase_g         = (1.0f - s) * P.g;
                    float reduction = (1.0f - s) + s * (1.0f - P.g);
                    cur_density     = TRK ? reduction * sig_base : reduction * density;
                }
            }
        };
        auto tracking_step = [&]() __attribute__((always_inline)) {
            tally(B_HALF, in_flight());
            if (LIGHT && !LOCAL)
            {
                // Every fetch of this path would filter eight zero texels (certified: the whole chord): the general expressions
                // below with den = +0 reduce exactly to sigma_t_den = +0, Ps = +0, c = Pn, `real` false for any draw and
                // sigma_null_den = sigma_t_prime -- no position, fetch or filter.  (A throughput that is not
                // finite stays NaN either way and the sample is written as 0.)
                if (in_track())
                {
                    dist += -logf_(rng.next_a()) * inv_sigma;  // kernel.cu:1419
                    if (dist >= t_end) set_code<EV_BG, MASKS>(st);   // transmitted through the box kernel.cu:1444-1452
                    else
                    {
                        // the collision test's variate is not needed (`real` is false whatever it is), but a sequential stream
                        // (sampler.h) must still move past it; for the counter-based streams this is nothing
                        (void)rng.next_b();
                        if (COUNT) c_den++;
                        // The throughput update of this null collision, thr *= sigma_t' * ((inv_sigma_t * Pn) / Pn) with
                        // Pn = |sigma_t' thr.x| + |sigma_t' thr.y| + |sigma_t' thr.z|, draws nothing and starts from (1,1,1) with the
                        // same sigma_t' in every sample: after n null collisions the throughput is the n-th iterate of one
                        // function of one float (three equal channels), tabulated by thr_table_k.  Count here, look up at the exit.
                        seg++;
                    }
                }
                if (MASKS) m_track &= __ballot(st == ST_TRACK);
                return;
            }
            if (in_flight())
            {
                const bool shadow = in_shadow();
                vp_pad<VP_PAD_STEP>();
                dist += -logf_(rng.next_a()) * inv_sigma;  // kernel.cu:2085 / :784
                tally(B_EXIT, dist >= t_end || (shadow && terms == 7));
                tally(B_LOOK, !(dist >= t_end || (shadow && terms == 7)));
                if (dist >= t_end || (shadow && terms == 7))
                {
                    vp_pad<VP_PAD_EOF>();
                    if (shadow)
                    {
                        // Tr_spectral returns 1 - terminated flags (kernel.cu:807)
                        if (!DEFER) nee_a = f3{(float)(1 - (terms & 1)), (float)(1 - ((terms >> 1) & 1)), (float)(1 - ((terms >> 2) & 1))};
                        if (!EARLY) set_code<EV_NEE, MASKS>(st);   // (EARLY: light_done writes the code)
                        rng.leave_shadow(rng_saved);
                        if (EARLY) light_done();
                    }
                    else if (LOCAL)
                    {
                        bool through = fminf(distc, dist) >= t_far;  // kernel.cu:2145
                        if (through)
                        {
                            ro = ro + rd * t_far;  // tracking restart kernel.cu:2151-2155 / :1809-1813
                            t_empty -= t_far;      // the certified-empty distance is measured from the segment origin
                            set_code<ST_SETUP, MASKS>(st);
                            dist = -1.0f;
                            if (EXITC) terms += d_max <= 0.0001f ? VP_EXIT_TRIP : 0;   // exit flights: a segment through a brick with maximum zero
                            if (EST == EST_BOUNDED && ++seg >= 800) set_code<EV_WRITE, MASKS>(st);  // `continue` still counts, :1716
                        }
                        else
                        {
                            if (MIS) seg_o = ro;
                            if (PARK) dist = distc;  // control collision kernel.cu:2088: ro + rd * distc, formed in the collision block
                            else ro = ro + rd * distc;
                            set_code<LIGHT ? EV_WRITE : EV_SCATTER, MASKS>(st);  // (LIGHT: excluded by the pixel class, which checks the brick minima)
                        }
                    }
                    else
                    {
                        set_code<EV_BG, MASKS>(st);  // transmitted through the box kernel.cu:1444-1452
                        if (PROF) { c_xout += zrun; zrun = 0; }
                    }
                }
                else
                {
                    vp_pad<VP_PAD_FETCH>();
                    f3    p   = ro + rd * dist;
                    float den;
                    tally(B_FETCH, !LIGHT && (shadow || !(dist < t_empty)));
                    if (LIGHT) den = 0.0f;  // light class of a local-majorant estimator: every fetch is certified to return +0
                    else if (EST == EST_GLOBAL)
                    {
                        // Before t_empty every texel this fetch would filter is zero (empty_table_k): the product is +0 without
                        // position, address, load or filter.  Whole waves of background rays take this branch together.
                        den = 0.0f;
                        if (shadow || !(dist < t_empty))
                        {
                            // (uchar volumes, exact arithmetic: the fetch with the scene's folded scales, vp_device.h fetch_scales)
                            den = sample_density01<QUANT, HALF, QUANT && kFetchFoldUnit>(S, p) * cur_density;  // vol_sigma_t kernel.cu:682-695
                            if (COUNT && !(shadow && dist >= t_clip) && !(!shadow && ex_clear)) c_load++;
                        }
                    }
                    else
                    {
                        // local-majorant estimators: the same certificate, measured from the current segment origin
                        den = 0.0f;
                        if (shadow || !(dist < t_empty))
                        {
                            den = sample_density01<QUANT, HALF>(S, p) * cur_density;  // vol_sigma_t kernel.cu:682-695
                            if (COUNT && !(shadow && dist >= t_clip) && !(!shadow && ex_clear)) c_load++;
                        }
                    }
                    float e   = rng.next_b();
                    if (COUNT) c_den++;
                    tally(B_ZERO, !LIGHT && !shadow && !(dist < t_empty) && den == 0.0f);
                    tally(B_ZERO_SH, !LIGHT && shadow && den == 0.0f && !(COUNT && dist >= t_clip));
                    if (TRK)
                    {
                        // scalar delta tracking: kernel.cu:2137-2142 / :745-748 (Tr stops AT its collision, no further draw)
                        if (e < den * inv_sigma)
                        {
                            if (shadow) { nee_a = f3{0.0f, 0.0f, 0.0f}; if (!EARLY) set_code<EV_NEE, MASKS>(st); rng.leave_shadow(rng_saved); if (EARLY) light_done(); }
                            else { if (!PARK) ro = p; set_code<EV_SCATTER, MASKS>(st); }
                        }
                    }
                    else if (shadow)
                    {
                        // kernel.cu:791-805
                        if (ACH) terms = (e < sig_t.x * den * inv_sigma) ? 7 : terms;
                        else
                        {
                            int t = terms;
                            t |= (e < sig_t.x * den * inv_sigma) ? 1 : 0;
                            t |= (e < sig_t.y * den * inv_sigma) ? 2 : 0;
                            t |= (e < sig_t.z * den * inv_sigma) ? 4 : 0;
                            terms = t;
                        }
                    }
                    else if (ACH)
                    {
                        // history-aware collision probabilities kernel.cu:2107-2134 (quirk Q8), one channel carried
                        float a_t = sig_t.x * den, a_s = sig_s.x * den;
                        if (LOCAL) { a_t = a_t - sigma_c; a_s = a_s - sigma_c; }
                        float a_n  = sigma_t_prime - a_t;
                        float mt   = __builtin_fabsf(a_t * thr.x), mn = __builtin_fabsf(a_n * thr.x);
                        float Ps   = (mt + mt) + mt;
                        float Pn   = (mn + mn) + mn;
                        float c    = Ps + Pn;
                        // (MASKS: one compare -- "not real" is the complement of this mask within the block's exec: !(a < b), NaN included)
                        const bool real = MASKS ? lane_in(__ballot(e * c < Ps)) : e * c < Ps;
                        float f    = wdiv_(inv_sigma_t * c, real ? Ps : Pn);
                        thr.x      = thr.x * ((real ? a_s : a_n) * f);
                        if (real)
                        {
                            if (MIS) seg_o = ro;
                            if (!PARK) ro = p;
                            set_code<LIGHT ? EV_WRITE : EV_SCATTER, MASKS>(st);  // (LIGHT: den = +0 makes `real` false)
                        }
                        else if (EXITC && den == 0.0f)
                        {
                            terms++;   // exit flights: a null collision in empty space
                            if (PROF) zrun++;
                        }
                    }
                    else
                    {
                        // history-aware collision probabilities kernel.cu:2107-2134 (quirk Q8)
                        f3 sigma_t_den = sig_t * den;
                        f3 sigma_s_den = sig_s * den;
                        if (LOCAL)
                        {
                            f3 sc       = f3{sigma_c, sigma_c, sigma_c};
                            sigma_t_den = sigma_t_den - sc;
                            sigma_s_den = sigma_s_den - sc;
                        }
                        f3    sigma_null_den = f3{sigma_t_prime, sigma_t_prime, sigma_t_prime} - sigma_t_den;
                        float Ps = __builtin_fabsf(sigma_t_den.x * thr.x) + __builtin_fabsf(sigma_t_den.y * thr.y) +
                                   __builtin_fabsf(sigma_t_den.z * thr.z);
                        float Pn = __builtin_fabsf(sigma_null_den.x * thr.x) + __builtin_fabsf(sigma_null_den.y * thr.y) +
                                   __builtin_fabsf(sigma_null_den.z * thr.z);
                        float c    = Ps + Pn;
                        // (MASKS: one compare -- "not real" is the complement of this mask within the block's exec: !(a < b), NaN included)
                        const bool real = MASKS ? lane_in(__ballot(e * c < Ps)) : e * c < Ps;
                        float f    = wdiv_(inv_sigma_t * c, real ? Ps : Pn);
                        f3    sel  = real ? sigma_s_den : sigma_null_den;
                        thr        = thr * (sel * f);
                        if (real)
                        {
                            if (MIS) seg_o = ro;
                            if (!PARK) ro = p;
                            set_code<LIGHT ? EV_WRITE : EV_SCATTER, MASKS>(st);  // (LIGHT: den = +0 makes `real` false)
                        }
                        else if (EXITC && den == 0.0f)
                        {
                            terms++;   // exit flights: a null collision in empty space
                            if (PROF) zrun++;
                        }
                    }
                }
            }
            // the masks after the step, from the codes, where the wave is whole: two compares for everything the step and the loop
            // ask about the lanes' states
            if (MASKS)
            {
                const unsigned long long actm = m_track | m_shadow;
                m_track  = __ballot(st == ST_TRACK) & actm;
                m_shadow = __ballot(st == ST_SHADOW) & actm;
            }
        };
        // the light kernel of the global-majorant estimator has the shortest step (a draw, a logarithm, an add and a compare):
        // more of them per round of wave-level bookkeeping
        constexpr int STEPS = (LIGHT && !LOCAL) ? VP_LIGHT_STEPS_PER_PASS : VP_STEPS_PER_PASS;
#pragma unroll 1
        for (int iter = 0;; iter += STEPS)
        {
            // lanes in a fast state; lanes that wait for the event pass
            bool active = true;
            unsigned long long am, wm;
            if (MASKS) { am = m_track | m_shadow; wm = m_live & ~am; }
            else
            {
                active = (st == ST_TRACK) || (st == ST_SHADOW) || (LOCAL && st == ST_SETUP);
                am     = __ballot(active);
                wm     = __ballot(!active && !(st == ST_DONE && exhausted));
            }
            unsigned nwait = (unsigned)__popcll(wm);
            if (am == 0ull || nwait >= L.wait_lanes || (nwait > 0u && iter >= (int)L.wait_iters)) break;
            if (PROF)
            {
                const unsigned long long sm = MASKS ? m_shadow : __ballot(st == ST_SHADOW);   // (a ballot under `lane == 0` would see lane 0 only)
                if (lane == 0) { d_iter++; d_act += (unsigned)__popcll(am); d_shadow += (unsigned)__popcll(sm); }
            }
            // (MASKS: no branch around the pass for the other lanes -- each step runs under its own mask, and the masks are formed
            // between the steps, where the wave is whole)
            if (!MASKS && !active) continue;
            segment_setup();
            tracking_step();
#pragma unroll
            for (int u = 1; u < STEPS; u++)
            {
                if (PROF)
                {
                    unsigned long long am2 = MASKS ? (m_track | m_shadow) : __ballot((st == ST_TRACK) || (st == ST_SHADOW) || (LOCAL && st == ST_SETUP));
                    const unsigned long long sm2 = MASKS ? m_shadow : __ballot(st == ST_SHADOW);
                    if (lane == 0) { d_iter++; d_act += (unsigned)__popcll(am2); d_shadow += (unsigned)__popcll(sm2); }
                }
                // a restart segment is set up at once while many lanes ask for one (the crawl toward and through empty bricks,
                // quirk Q6); a few stragglers -- a dense region ends a 0.05 segment every ~40 steps per lane -- wait for the
                // first step of the next pass, so that the ~100 instructions of the set-up are not run for one or two lanes
                if (LOCAL && (unsigned)__popcll(__ballot(st == ST_SETUP)) >= L.setup_lanes) segment_setup();
                tracking_step();
            }
        }
        if (PROF) { unsigned long long t = __builtin_amdgcn_s_memtime(); if (lane == 0) t_fast += t - t_mark; t_mark = t; }
    }

    if (COUNT)
    {
        // wave reduction, one atomic per counter per wave
        unsigned long long vals[12] = {c_smp, c_den, c_bnd, c_opa, c_env, c_sca, d_iter, d_act, d_outer, d_shadow, t_slow, t_fast};
#pragma unroll
        for (int q = 0; q < (PROF ? 12 : 6); q++)
        {
            unsigned long long v = vals[q];
            for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
            if (lane == 0) atomicAdd(&L.counters[q], v);
        }
        {
            unsigned long long v = c_load;
            for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
            if (lane == 0) atomicAdd(&L.counters[12], v);
        }
        {
            // exit flights: tests, hops through the distance field (one byte loaded each), paths ended
            unsigned long long xv[3] = {c_xtest, c_xout, c_xok};
#pragma unroll
            for (int q = 0; q < 3; q++)
            {
                unsigned long long v = xv[q];
                for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
                if (lane == 0) atomicAdd(&L.counters[13 + q], v);
            }
        }
        // block tallies are wave-uniform: lane 0 adds them
        if (PROF && lane == 0)
        {
#pragma unroll
            for (int b = 0; b < B_NBLK; b++) { atomicAdd(&L.counters[16 + 2 * b], bw[b]); atomicAdd(&L.counters[17 + 2 * b], bl[b]); }
#pragma unroll
            for (int h = 0; h < 3; h++)
#pragma unroll
                for (int q = 0; q < 8; q++) atomicAdd(&L.counters[48 + 8 * h + q], hist[h][q]);
            atomicAdd(&L.counters[72], ctrl_w); atomicAdd(&L.counters[73], ctrl_l);
        }
    }
}

// ---- the camera rays' way to the medium, ahead of the integrator (global-majorant estimator, counter-based streams).
// A general pixel's camera ray is the same in every frame (quirk Q3) and certified to run through empty cells up to t_empty
// (empty_table_k): until its free flight passes that distance a path does nothing but draw a pair, take the logarithm of its first
// word, add and compare -- the collision there is a null collision with density +0 that leaves a throughput of exactly 1 unchanged
// (light_identity_k has checked that for this medium; the host asks for this kernel only then).  About 500 such steps per sample at
// the default camera, 44 % of the lane-steps of the integrator's tracking loop on BASELINE config 2 -- where the lanes that make
// them sit beside lanes that fetch and collide, and wait while those do.  Here a thread per sample makes them and nothing else:
// slot s of the launch's pixel list in frame f, 64 neighbouring pixels per wave (their walks have about the same length).  It
// stops BEFORE the first flight that would pass t_empty or leave the box and leaves (distance reached, pairs used) in the sample's
// staging slot; render_k takes the sample up from there and makes that flight itself (its own test `dist < t_empty` is still in
// place: any prefix of the walk is a valid hand-over, so the step cap below costs nothing but the steps left over).
// a look-ahead batch that was cancelled before its walk began (LaunchDev::cancel): one atomic read per wave; render_k, which then
// hands out no sample, never reads the slots this walk would have written
__device__ __forceinline__ bool approach_cancelled(const LaunchDev& L)
{
    if (!L.cancel) return false;
    unsigned w = 0;
    if ((threadIdx.x & 63u) == 0u) w = __hip_atomic_load(L.cancel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return (unsigned)__builtin_amdgcn_readfirstlane((int)w) >= L.batch_id;
}
// The walks themselves: free flights from `dist` for as long as they end in front of a limit.  Per step a counter-based stream
// pays for the draw, the logarithm, the flight and ONE compare of the distance (profiles/experiments/approach_step.txt):
//  - the two limits of a walk are folded into their minimum before the loop (a NaN limit makes the minimum NaN or leaves the other
//    compare to decide: the walk stops where the two compares stopped it);
//  - a draw of exactly 0 (a word below 512: one step in 2^23) is a flight of +inf * inv_sigma, which passes every limit or is NaN --
//    where inv_sigma does not carry a minus sign (-0 included).  The loop tests the draw itself and takes logf_pos_, the logarithm
//    without its answer for 0; what the flight would have been is formed behind the loop where a caller needs it.  A majorant with a
//    minus sign (a negative density or extinction: the flights run backwards, whatever is rendered means nothing) keeps the loop
//    that asks logf_ -- one branch in front of the walk, the same way for every lane: the sign is the medium's -- so that the bits
//    stay what they were even there;
//  - the state of a counter-based stream is its pair index, the steps made: it is formed once behind the loop, not saved per step.
// A sequential stream (RngSamplerH) moves past the collision test's variate and saves its two words after every step, as before.
// The walks' loops leave through their exits: an empty statement the compiler may not move keeps it from turning the few
// instructions behind a `break` into selects that every lane executes at every step (and the loop's uniform counter into a vector).
#define VP_KEEP_BRANCH() asm volatile("")
#define VP_WALK_UNROLL 2   // steps per iteration of the counter-based walks below, written out (scripts/approach_step_isa.py divides by it)
// the one limit of a walk: the nearer of the segment's (or the box's) end, which is no NaN, and the certified-empty distance
__device__ __forceinline__ float walk_limit(float t_box, float t_empty) { return t_box < t_empty ? t_box : t_empty; }
__device__ __forceinline__ bool walks_backwards(float inv_sigma) { return (f2u(inv_sigma) >> 31) != 0u; }

// approach_k's walk: steps of at most `cap` (a bound on the loop's uniform counter) from `dist`, each ending in front of t_lim.
// Out: the distance reached in `dist`, the steps made (returned), the stream's state before the flight in hand in (sa, sb).
template <class RNG>
__device__ __forceinline__ unsigned approach_walk(float& dist, const float t_lim, const float inv_sigma, const unsigned cap, RNG& rng, unsigned& sa,
                                                  unsigned& sb)
{
    unsigned steps = 0;
    rng.save(sa, sb);
    if (!RNG::kShadowSubstream || walks_backwards(inv_sigma))
    {
        for (; steps < cap; steps++)
        {
            const float d2 = dist + -logf_(rng.next_a()) * inv_sigma;   // kernel.cu:1419
            if (!(d2 < t_lim)) break;                                    // the integrator's step: a fetch, or the way out
            dist = d2;
            (void)rng.next_b();   // the collision test's variate: `real` is false whatever it is; a sequential stream moves past it
            rng.save(sa, sb);
        }
        return steps;
    }
    // Two steps per iteration, the distance in turn in `a` and in `b`: each flight is summed straight into the other variable
    // BEFORE its test, so a lane that stops leaves its own distance where it was and a lane that goes on copies nothing.  After an
    // even number of steps the distance reached is in `a`, after an odd number in `b`, wherever the lane left the loop.
    const unsigned base = sa;
    float          a = dist, b = dist;
    unsigned       twos = 0;       // iterations the lane has completed: the loop's one per-lane counter
    bool           odd  = false;   // ... and whether it left in the middle of one, behind the first of its two steps
    for (unsigned i = 0; i < cap; i += 2u)
    {
        rng.set_pair(base + i);   // (the pair index from the uniform counter: its first Philox round stays scalar)
        const float ua = rng.next_a();
        b              = a + -logf_pos_(ua) * inv_sigma;   // kernel.cu:1419
        if (ua == 0.0f || !(b < t_lim)) break;
        VP_KEEP_BRANCH();
        odd = true;
        if (i + 1u == cap) break;
        rng.set_pair(base + i + 1u);
        const float ub = rng.next_a();
        a              = b + -logf_pos_(ub) * inv_sigma;
        if (ub == 0.0f || !(a < t_lim)) break;
        VP_KEEP_BRANCH();
        odd = false;
        twos++;
    }
    dist  = odd ? b : a;
    steps = 2u * twos + (odd ? 1u : 0u);
    rng.set_pair(base + steps);
    rng.save(sa, sb);
    return steps;
}

// The inner loop of approach_local_k and approach_local_tab_k: flights inside one restart segment, from `dist`, until one passes the
// segment's end t_far (returns true: `through`, kernel.cu:2145) or the certified-empty distance (false: a fetch, render_k's).  In: the
// stream's state in (ta, tb).  Out: the distance reached, the steps made added to `n_steps`, (ta, tb) the state before the flight that
// ended the walk, `rng` behind that flight.  VP_WALK_GUARD bounds the flights of one segment (a majorant of 1e-4 * 0.05 needs a
// handful; the guard is for a broken one): a bound on the loop's uniform counter, which ends the walk as a fetch does.
#define VP_WALK_GUARD 60002u   // (even: the loop makes two steps per iteration)
template <class RNG>
__device__ __forceinline__ bool approach_segment_walk(float& dist, const float t_far, const float t_empty, const float inv_sigma, RNG& rng, unsigned& ta,
                                                      unsigned& tb, unsigned long long& n_steps)
{
    if (!RNG::kShadowSubstream || walks_backwards(inv_sigma))
    {
        unsigned steps   = 0;
        bool     through = false;
        for (;;)
        {
            const float d2 = dist + -logf_(rng.next_a()) * inv_sigma;   // kernel.cu:2085
            if (d2 >= t_far) { through = true; break; }                   // t_end = min(1e20, t_far): `through`, kernel.cu:2145
            if (!(d2 < t_empty) || steps > 60000u) break;                 // a fetch: render_k's
            dist = d2;
            (void)rng.next_b();   // the collision test's variate (`real` is false whatever it is): a sequential stream moves past it
            rng.save(ta, tb);
            steps++;
        }
        n_steps += steps;
        return through;
    }
    // two steps per iteration, the distance in turn in `a` and `b`, as in approach_walk; the loop's one per-lane counter is the
    // stream's own pair index (the lanes of a wave stand at different indices behind their first segment)
    const float    t_stop = walk_limit(t_far, t_empty);
    const unsigned base   = ta;
    float          a = dist, b = dist, ua = 1.0f, ub = 1.0f;
    bool           odd = false;   // the lane left behind the first of an iteration's two steps
    for (unsigned k = 0; k < VP_WALK_GUARD; k += 2u)
    {
        ua = rng.next_a();
        b  = a + -logf_pos_(ua) * inv_sigma;   // kernel.cu:2085
        if (ua == 0.0f || !(b < t_stop)) break;
        VP_KEEP_BRANCH();
        odd = true;
        ub  = rng.next_a();
        a   = b + -logf_pos_(ub) * inv_sigma;
        if (ub == 0.0f || !(a < t_stop)) break;
        VP_KEEP_BRANCH();
        odd = false;
    }
    // a flight that ended the walk has been drawn and counted by the stream; the guard (behind a whole iteration) draws nothing
    const float u       = odd ? ub : ua;
    float       d2      = odd ? a : b;
    dist                = odd ? b : a;
    const bool  stopped = odd || ua == 0.0f || !(b < t_stop);
    if (u == 0.0f) d2 = dist + __builtin_inff() * inv_sigma;   // the flight of a zero draw, as logf_ has it
    unsigned at, unused;
    rng.save(at, unused);
    const unsigned steps = at - base - (stopped ? 1u : 0u);
    n_steps += steps;
    RNG before = rng;
    before.set_pair(base + steps);
    before.save(ta, tb);
    return stopped && d2 >= t_far;
}

template <class RNG>
__global__ __launch_bounds__(256) void approach_k(SceneDev S, LaunchDev L)
{
    if (approach_cancelled(L)) return;
    // a wave = ONE pixel in 64 consecutive frames where the launch has that many (fewer frames: 2^k frames x 64 / 2^k pixels): the
    // lanes share the ray, its certificate and the bricks it crosses, and differ only in what they draw -- their walks have
    // the same length up to the noise of a sum of exponentials
    const unsigned sh   = L.approach_fshift;
    const unsigned slot = blockIdx.x * (256u >> sh) + (threadIdx.x >> sh), fl = (blockIdx.y << sh) + (threadIdx.x & ((1u << sh) - 1u));
    if (slot >= L.nslots || fl >= (unsigned)L.nframes) return;
    const ParamDev& P = L.P;
    const unsigned pix = L.pixels[slot], px = pix & 0xffffu, py = pix >> 16;
    if (px >= P.width || py >= P.height) return;   // a partial edge tile: render_k skips the slot as well
    f3 ro, rd;
    camera_ray(S, P.width, P.height, px, py, ro, rd);
    float    t_near, tf, dist = 0.0f;
    unsigned pairs = 0, sa = 0, sb = 0;   // steps made; the stream's state before the step in hand
    RNG      rng;
    if (intersect_box(ro, rd, S, t_near, tf))
    {
        // the set-up of render_k's first segment (kernel.cu:1332-1370, depth index 0)
        if (t_near < 0.0f) t_near = 0.0f;
        dist                      = t_near;
        const float t_end         = tf;
        const float t_empty       = L.crawl[2 * ((size_t)px + (size_t)py * P.width) + 1].x;
        const float s             = hyperion_s(0 - 5);
        const float cur_density   = (1.0f - s) * P.density + s * P.density * (1.0f - P.g);
        const float sigma_t_prime = max3(f3{P.sigma_t[0], P.sigma_t[1], P.sigma_t[2]}) * cur_density;
        const float inv_sigma     = rcp_(sigma_t_prime);
        rng.init(px, py, (unsigned)(L.frame0 + (int)fl), L.key0, L.key1);
        // a flight that passes t_empty is the integrator's step (a fetch), one that passes t_end its way out (t_end is no NaN here)
        pairs = approach_walk(dist, walk_limit(t_end, t_empty), inv_sigma, L.approach_steps, rng, sa, sb);
    }
    L.stage[(size_t)fl * L.stage_stride + L.slot_base + slot] = make_float4(dist, u2f(sa), u2f(sb), u2f(pairs));
    if (L.counters && pairs) atomicAdd(&L.counters[1], (unsigned long long)pairs);   // density lookups the estimator makes on these steps
}

// The same for the decomposition estimator (uchar bound table): behind the crawl in front of the box (crawl_table_k) the camera ray
// walks restart segments of 0.05 through bricks whose cells it is certified not to meet non-empty (t_empty): a bound fetch, and free
// flights with the brick's majorant whose null collisions change nothing (checked per segment), until the flight leaves the segment.  A thread per sample walks every segment that ENDS before the certified distance -- no fetch can
// fall into it -- and then INTO the first one that does not, up to the flight that would need a fetch (round 4): (origin of that
// segment, distance reached in it) in the sample's staging slot, the stream's state beside it.  A segment whose brick has a positive
// minimum (the control distance is the integrator's business) or a non-neutral majorant is handed over at its origin.
template <class RNG, bool QUANT>
__global__ __launch_bounds__(256) void approach_local_k(SceneDev S, LaunchDev L)
{
    if (approach_cancelled(L)) return;
    const unsigned sh   = L.approach_fshift;   // (a wave = one pixel in 2^sh frames, as in approach_k)
    const unsigned slot = blockIdx.x * (256u >> sh) + (threadIdx.x >> sh), fl = (blockIdx.y << sh) + (threadIdx.x & ((1u << sh) - 1u));
    if (slot >= L.nslots || fl >= (unsigned)L.nframes) return;
    const ParamDev& P = L.P;
    const unsigned pix = L.pixels[slot], px = pix & 0xffffu, py = pix >> 16;
    if (px >= P.width || py >= P.height) return;
    f3 ro, rd;
    camera_ray(S, P.width, P.height, px, py, ro, rd);
    const f3     inv_rd = f3{1.0f / rd.x, 1.0f / rd.y, 1.0f / rd.z};   // (IEEE in both modes: approach_segments_k's)
    const size_t idx    = (size_t)px + (size_t)py * P.width;
    const float4 c      = L.crawl[2 * idx];
    float        t_empty = L.crawl[2 * idx + 1].x;
    ro                  = f3{c.x, c.y, c.z};
    // segment_medium() of render_k for an unscattered path
    const float s           = hyperion_s(0 - 5);
    const float reduction   = (1.0f - s) + s * (1.0f - P.g);
    const float cur_density = reduction * P.density;
    const float max_sig     = max3(f3{P.sigma_t[0], P.sigma_t[1], P.sigma_t[2]});
    RNG rng;
    rng.init(px, py, (unsigned)(L.frame0 + (int)fl), L.key0, L.key1);
    rng.skip(f2u(c.w) >> 16);   // the crawl's draws
    unsigned sa, sb;            // where the stream stands: at the origin of the segment in hand, or before the flight it stopped at
    rng.save(sa, sb);
    float    d_reached = -1.0f; // how far into the segment at `ro` the walk got (free-flight distance from its origin); -1: not at all
    unsigned long long n_steps = 0, n_segs = 0;
    for (unsigned n = 0; n < L.approach_steps; n++)
    {
        // segment_setup() of render_k (intersectSuperVolume kernel.cu:1626-1661)
        float t_near, tf;
        const bool hit = intersect_box_inv(ro, inv_rd, S, t_near, tf);
        t_near         = fmaxf(t_near, 0.0f);
        const float t_far = fminf(tf, 0.05f);
        float bx, by;
        sample_bound<QUANT>(S, ro + rd * t_near, bx, by);
        if (!hit || by > 0.0f) break;
        const float d_max         = fmaxf(0.0001f, bx);
        const float sigma_t_prime = max_sig * cur_density * d_max;
        const float inv_sigma     = rcp_(sigma_t_prime);
        // a null collision in empty space must leave the throughput of 1 as it is for THIS majorant (most do; the constant light class
        // asks it of every majorant in the table, light_identity_k): where it does not, the integrator goes on from here
        if (!(null_collision_in_empty_space(1.0f, sigma_t_prime, inv_sigma) == 1.0f)) break;
        float    dist = t_near;
        unsigned ta = sa, tb = sb;   // the stream before the flight in hand
        const bool through = approach_segment_walk(dist, t_far, t_empty, inv_sigma, rng, ta, tb, n_steps);
        if (!through)
        {
            // the flight in hand needs a fetch: render_k takes the path up INSIDE this segment -- its own set-up of the segment at `ro`
            // (the same bound, majorant and t_far), then the flight from `dist` with the stream as it stood before that flight
            // (round 4; before, the whole segment was handed back and walked again, ~38 steps per path of the decomposition workloads)
            d_reached = dist; sa = ta; sb = tb;
            break;
        }
        rng.save(sa, sb);
        n_segs++;
        ro      = ro + rd * t_far;   // tracking restart kernel.cu:2151-2155
        t_empty -= t_far;
    }
    const size_t item = (size_t)fl * L.stage_stride + L.slot_base + slot;
    L.stage[item] = make_float4(ro.x, ro.y, ro.z, d_reached);
    L.approach_aux[item] = make_uint2(sa, sb);   // where the stream stands: the pair index, or sampler.h's two words
    if (L.counters)
    {
        if (n_steps) atomicAdd(&L.counters[1], n_steps);   // density lookups and bound lookups the estimator makes on this stretch
        if (n_segs) atomicAdd(&L.counters[2], n_segs);
    }
}

// ---- The approach walk of the decomposition estimator, with what depends on the PIXEL alone tabulated per pixel (round 5).
// approach_local_k above sets every restart segment up per SAMPLE: box intersection, bound fetch, majorant, reciprocal, the neutrality
// test -- ~75 of its ~130 vector instructions per segment -- although the camera ray, hence the chain of segment origins
// ro_(n+1) = ro_n + rd * t_far_n and everything the set-up computes from them, is the same in every frame (quirk Q3); a wave of that
// kernel is ONE pixel in 64 frames computing the same 75 instructions in 64 lanes.  approach_segments_k walks the chain once per pixel
// of the general class (the identical binary32 operations, in the same order) and writes per segment (t_near, t_far, the brick's
// bytes, a stop flag; the segment's origin, the certified-empty distance left at its start); approach_local_tab_k reads the records --
// one 32-byte broadcast load per segment -- looks the majorant's reciprocal and its neutrality up by the byte (a 256-entry table in LDS,
// computed per launch with the integrator's own expressions: they depend on Param), and makes what is left: the draws, the
// logarithms, the sums and the compares.  Same hand-over, same bits (uchar bound tables; float tables keep approach_local_k).
#define VP_SEG_CAP 96   // records per pixel: a box diagonal of 4.7 at 0.05 per segment; a longer chain is handed over where the table ends
// (chains that reach the cap, inside a long box and in front of a far one: tests/test_long_rays_gpu.py, record by record through vp_get_segment_table)
// layout per pixel slot, 2 * VP_SEG_CAP float4: [n] = (t_near, t_far, bound byte | stop << 8, t_empty at the segment's start),
// [VP_SEG_CAP + n] = the segment's origin (read once per sample, at the hand-over)

// A wave = one pixel in 64 frames (launched only with approach_fshift 6): it copies its pixel's chain into LDS with two coalesced loads
// and walks it from there -- what a sample waits for per segment is an LDS read, not a dependent read of global memory (the first form,
// records read from global memory segment by segment, took 17.0 of approach_local_k's 18.3 ms on C3 although it executes half the
// instructions: profiles/experiments/r05_segment_table.txt).
template <class RNG>
__global__ __launch_bounds__(256) void approach_local_tab_k(SceneDev S, LaunchDev L)
{
    // per launch: for every byte a brick maximum can be, the reciprocal of the segment's majorant and whether a null collision in
    // empty space leaves a throughput of 1 as it is under it -- approach_local_k's expressions, once per workgroup instead of per segment
    __shared__ float4 chain[4][VP_SEG_CAP];
    __shared__ float inv_tab[256];
    __shared__ unsigned char ok_tab[256];
    const unsigned wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const unsigned slot = blockIdx.x * 4u + wv, fl = (blockIdx.y << 6) + lane;
    {
        const ParamDev& P = L.P;
        const float s           = hyperion_s(0 - 5);
        const float reduction   = (1.0f - s) + s * (1.0f - P.g);
        const float cur_density = reduction * P.density;
        const float max_sig     = max3(f3{P.sigma_t[0], P.sigma_t[1], P.sigma_t[2]});
        const unsigned b = threadIdx.x;   // 256 threads
        const float d_max         = fmaxf(0.0001f, (float)b * VP_U8_SCALE);
        const float sigma_t_prime = max_sig * cur_density * d_max;
        const float inv_sigma     = rcp_(sigma_t_prime);
        inv_tab[b] = inv_sigma;
        ok_tab[b]  = null_collision_in_empty_space(1.0f, sigma_t_prime, inv_sigma) == 1.0f ? 1 : 0;
        if (slot < L.nslots)
        {
            // (records behind the chain's stop record were never written: read, never used)
            const float4* rec = L.seg_table + (size_t)slot * (2 * VP_SEG_CAP);
            chain[wv][lane] = rec[lane];
            if (lane < VP_SEG_CAP - 64u) chain[wv][64u + lane] = rec[64u + lane];
        }
    }
    __syncthreads();
    if (approach_cancelled(L)) return;
    if (slot >= L.nslots || fl >= (unsigned)L.nframes) return;
    const ParamDev& P = L.P;
    const unsigned pix = L.pixels[slot], px = pix & 0xffffu, py = pix >> 16;
    if (px >= P.width || py >= P.height) return;
    const size_t idx = (size_t)px + (size_t)py * P.width;
    RNG rng;
    rng.init(px, py, (unsigned)(L.frame0 + (int)fl), L.key0, L.key1);
    rng.skip(f2u(L.crawl[2 * idx].w) >> 16);   // the crawl's draws
    unsigned sa, sb;
    rng.save(sa, sb);
    float    d_reached = -1.0f;
    unsigned n = 0;
    unsigned long long n_steps = 0, n_segs = 0;
    for (;; n++)
    {
        const float4 A = chain[wv][n];
        const unsigned bits = f2u(A.z);
        if ((bits & 0x100u) || n >= L.approach_steps || !ok_tab[bits & 0xffu]) break;   // handed over at this segment's origin
        const float inv_sigma = inv_tab[bits & 0xffu], t_far = A.y, t_empty = A.w;
        float    dist = A.x;
        unsigned ta = sa, tb = sb;   // the stream before the flight in hand
        const bool through = approach_segment_walk(dist, t_far, t_empty, inv_sigma, rng, ta, tb, n_steps);
        if (!through) { d_reached = dist; sa = ta; sb = tb; break; }
        rng.save(sa, sb);
        n_segs++;
    }
    const float4 O = L.seg_table[(size_t)slot * (2 * VP_SEG_CAP) + VP_SEG_CAP + n];
    const size_t item = (size_t)fl * L.stage_stride + L.slot_base + slot;
    L.stage[item] = make_float4(O.x, O.y, O.z, d_reached);
    L.approach_aux[item] = make_uint2(sa, sb);
    if (L.counters)
    {
        if (n_steps) atomicAdd(&L.counters[1], n_steps);
        if (n_segs) atomicAdd(&L.counters[2], n_segs);
    }
}

