// vp_dispatch.h -- which render_k instance and which approach kernel a launch runs: the one place that decides it.
//
// Included INSIDE the namespace, after the kernels (vp_integrator.h), by vp_kernels.hip (namespace vp) and by vp_kernels_fast.hip
// (namespace vp::fast, VP_ARITH_FAST defined).  It names render_k, approach_k, approach_local_k and approach_local_tab_k and compiles
// against whatever declaration of them precedes it: tests/render_variants_probe.cpp puts host stand-ins there and tabulates the choice
// for every request the API admits (tests/test_render_variants_cpu.py, tests/golden/render_variants.txt).
//
// A launch goes request -> instance -> kernel:
//   RenderRequest      what the host knows about the launch
//   render_instance()  the rules that turn it into render_k's eleven template arguments (light_instance(): the light pixel class)
//   render_built()     which instances this translation unit compiles -- its truth set IS the set of render_k kernels in the object,
//                      because launch_instance() names a kernel only under `if constexpr (render_built(...))`
//   launch_instance()  the run-time instance lifted to template arguments; kernel_not_built() (vp_kernels.h) for the rest
//   launch_plane_instance()  the same for a launch with planes (LaunchDev::layers and / or LaunchDev::groups): render_k's twelfth and
//                      thirteenth arguments, LYR and GRP, for the subset planes_built() states, one table per plane mode -- only where
//                      the kernels above have the two arguments (VP_RENDER_K_HAS_PLANES)
// and the same, smaller, for the approach walk (approach_built(), launch_approach_walk()).  dispatch_render(), dispatch_light() and
// dispatch_approach() are what the launch_* functions of vp_kernels.h call.  Each launcher counts the launch under its table index
// (census_record(), vp_kernels.h: the launch census, a test hook) just before it calls through the table.

// ---- the build
#ifdef VP_DEV_BUILD
constexpr bool kDevBuild = true;    // make dev: the bench workloads' kernels only
#else
constexpr bool kDevBuild = false;
#endif
#ifdef VP_ARITH_FAST
constexpr bool kFastArith = true;
#else
constexpr bool kFastArith = false;
#endif

template <int R> struct RngOf;
template <> struct RngOf<RNG_SAMPLERH> { using type = RngSamplerH; };
template <> struct RngOf<RNG_PHILOX> { using type = RngPhilox; };
template <> struct RngOf<RNG_PHILOX7> { using type = RngPhilox7; };

// ---- render_k
struct RenderRequest
{
    int  est, rng;        // EST_*, RNG_*
    bool quant, half;     // uchar volume / binary16 volume (neither: float)
    bool count;           // work counters
    int  lds_form;        // how the host wants the brick table read (vp_kernels.h): a wish, granted where an instance exists
    bool mis;             // active environment sampling
    int  trk;             // 0 spectral, 1 scalar, 2 multi-channel tracking
    bool cancel;          // the launch can be told to stop (LaunchDev::cancel)
    bool ach;             // achromatic(L.P)
};
inline RenderRequest render_request(const LaunchDev& L, int est, int rng, bool quant, bool half, bool count, int lds_form, bool mis, int trk)
{
    RenderRequest r{};
    r.est = est; r.rng = rng; r.quant = quant; r.half = half; r.count = count; r.lds_form = lds_form; r.mis = mis; r.trk = trk;
    r.cancel = L.cancel != nullptr;
    r.ach    = achromatic(L.P);
    return r;
}
// the template arguments of render_k (vp_integrator.h), by name
struct RenderInst { int est, rng; bool quant, count; int ldsb; bool ach, mis; int trk; bool light, cancel, half; };

constexpr RenderInst render_instance(const RenderRequest& r)
{
    RenderInst v{};
    v.est = r.est; v.rng = r.rng; v.quant = r.quant; v.half = r.half; v.trk = r.trk;
    // scalar and multi-channel tracking (the reference's compiled-out SPECTRAL_TRACKING 0 / MULTI_CHANNEL 1): three-channel throughput,
    // no LDS / MIS / counting / look-ahead specialisations
    if (r.trk) return v;
    v.ach = r.ach; v.mis = r.mis;
    v.count = r.count;
    // look-ahead batches of the shipped configuration -- passive environment -- run the instance that can be stopped at once; a
    // counting launch is never one
    v.cancel = r.cancel && !r.count && !r.mis;
    // the brick table through LDS: decomposition estimator, uchar volume, passive environment.  Form 2 (2-bit codes beside the cold
    // state) for timed launches of the counter-based streams only; where it cannot be had, form 1 (512-thread workgroups)
    if (r.lds_form != 0 && r.est == EST_DECOMP && r.quant && !r.mis)
        v.ldsb = (r.lds_form == 2 && r.rng != RNG_SAMPLERH && !v.count && !v.cancel) ? 2 : 1;
    return v;
}
// The light pixel class (camera rays that meet empty cells only).  A light path never collides with matter: its throughput starts at
// (1,1,1) and every null collision in empty space multiplies the three channels by the same factor (sigma_t' - 0 in each), so they
// stay bitwise equal whatever the medium -- the one-channel (ACH) instance computes exactly what the three-channel one would.
// The light kernels fetch no cells: QUANT only selects how the bound table of the local-majorant estimators is read.
constexpr RenderInst light_instance(int est, int rng, bool quant, bool count)
{
    RenderInst v{};
    v.est = est; v.rng = rng; v.count = count;
    v.quant = quant || est == EST_GLOBAL;
    v.ach   = true;
    v.light = true;
    return v;
}

// the instances render_instance() / light_instance() can return for a request the API admits (vp_render.cpp check_render)
constexpr bool render_selectable(const RenderInst& v)
{
    if (v.quant && v.half) return false;
    if (v.light) return v.ach && !v.mis && !v.trk && !v.ldsb && !v.cancel && !v.half && (v.quant || v.est != EST_GLOBAL);
    if (v.trk) return v.rng != RNG_PHILOX7 && !v.count && !v.ldsb && !v.ach && !v.mis && !v.cancel;
    if (v.mis && (v.rng == RNG_PHILOX7 || v.ldsb || v.cancel)) return false;
    if (v.count && v.cancel) return false;
    if (v.ldsb && !(v.est == EST_DECOMP && v.quant)) return false;
    if (v.ldsb == 2 && (v.rng == RNG_SAMPLERH || v.count || v.cancel)) return false;
    return true;
}
// ... and of those, the ones this translation unit compiles
constexpr bool render_built(const RenderInst& v)
{
    if (!render_selectable(v)) return false;
    // the development build: Philox streams, spectral tracking, passive environment, the global-majorant and decomposition estimators,
    // the uchar volume (QUANT of a light instance names a bound table, not a volume: both stay)
    if (kDevBuild && (v.rng == RNG_SAMPLERH || v.trk || v.mis || v.est == EST_BOUNDED || (!v.quant && !v.light))) return false;
    // the fast arithmetic: the counter-based streams' shipped configuration; the light class is the exact build's
    if (kFastArith && (v.rng == RNG_SAMPLERH || v.trk || v.mis || v.est == EST_BOUNDED || v.count || v.light)) return false;
    return true;
}

// instances <-> indices into launch_instance()'s table: mixed radix, the fields in the order of the template parameters
constexpr unsigned kRenderInsts = 3u * 3u * 2u * 2u * 3u * 2u * 2u * 3u * 2u * 2u * 2u;
constexpr unsigned render_index(const RenderInst& v)
{
    if ((unsigned)v.est > 2u || (unsigned)v.rng > 2u || (unsigned)v.ldsb > 2u || (unsigned)v.trk > 2u) return kRenderInsts;
    unsigned i = (unsigned)v.est;
    i = i * 3u + (unsigned)v.rng;
    i = i * 2u + v.quant;
    i = i * 2u + v.count;
    i = i * 3u + (unsigned)v.ldsb;
    i = i * 2u + v.ach;
    i = i * 2u + v.mis;
    i = i * 3u + (unsigned)v.trk;
    i = i * 2u + v.light;
    i = i * 2u + v.cancel;
    i = i * 2u + v.half;
    return i;
}
constexpr RenderInst render_at(unsigned i)
{
    RenderInst v{};
    v.half   = i % 2u; i /= 2u;
    v.cancel = i % 2u; i /= 2u;
    v.light  = i % 2u; i /= 2u;
    v.trk    = (int)(i % 3u); i /= 3u;
    v.mis    = i % 2u; i /= 2u;
    v.ach    = i % 2u; i /= 2u;
    v.ldsb   = (int)(i % 3u); i /= 3u;
    v.count  = i % 2u; i /= 2u;
    v.quant  = i % 2u; i /= 2u;
    v.rng    = (int)(i % 3u); i /= 3u;
    v.est    = (int)i;
    return v;
}

using RenderLaunchFn = void (*)(const SceneDev&, const LaunchDev&, int, hipStream_t);
template <unsigned I>
static void launch_instance_at(const SceneDev& S, const LaunchDev& L, int blocks, hipStream_t st)
{
    constexpr RenderInst v = render_at(I);
    using RNG = typename RngOf<v.rng>::type;
    constexpr unsigned block = v.ldsb == 1 ? VP_BLOCK_LDS : VP_BLOCK;
    hipLaunchKernelGGL((render_k<v.est, RNG, v.quant, v.count, v.ldsb, v.ach, v.mis, v.trk, v.light, v.cancel, v.half>), dim3(blocks), dim3(block), 0, st, S, L);
}
template <unsigned I>
constexpr RenderLaunchFn render_launcher()
{
    if constexpr (render_built(render_at(I))) return &launch_instance_at<I>;
    else return nullptr;
}
template <unsigned... I>
static void launch_instance(const RenderInst& v, std::integer_sequence<unsigned, I...>, const SceneDev& S, const LaunchDev& L, int blocks, hipStream_t st)
{
    static constexpr RenderLaunchFn table[kRenderInsts] = {render_launcher<I>()...};
    const unsigned i = render_index(v);
    if (i >= kRenderInsts || !table[i]) kernel_not_built();
    census_record(kFastArith, CENSUS_RENDER, i);
    table[i](S, L, blocks, st);
}
// ---- the instances of a launch with planes (vp_kernels.h PLANES_*: LaunchDev::layers -> render_k's LYR argument, LaunchDev::groups ->
// its GRP argument, both for a group-layers launch).  Compiled where the kernels that precede this file have the two arguments
// (vp_integrator.h defines VP_RENDER_K_HAS_PLANES).  The subset, the same for every mode: spectral tracking, passive environment, the
// three estimators, the three streams, the three volume formats, every LDS form, general and light class; no work counters, no
// look-ahead (a plane call quiesces it), the exact translation unit only -- vp_render.cpp refuses everything else first.  One table
// per mode, each with a census of its own (census_of_planes).
#ifdef VP_RENDER_K_HAS_PLANES
constexpr bool planes_built(const RenderInst& v)
{
    return render_built(v) && !kFastArith && !v.trk && !v.mis && !v.count && !v.cancel;
}
template <unsigned I, bool LYR, bool GRP>
static void launch_plane_instance_at(const SceneDev& S, const LaunchDev& L, int blocks, hipStream_t st)
{
    constexpr RenderInst v = render_at(I);
    using RNG = typename RngOf<v.rng>::type;
    constexpr unsigned block = v.ldsb == 1 ? VP_BLOCK_LDS : VP_BLOCK;
    hipLaunchKernelGGL((render_k<v.est, RNG, v.quant, v.count, v.ldsb, v.ach, v.mis, v.trk, v.light, v.cancel, v.half, LYR, GRP>), dim3(blocks), dim3(block), 0, st, S, L);
}
template <unsigned I, bool LYR, bool GRP>
constexpr RenderLaunchFn plane_launcher()
{
    if constexpr (planes_built(render_at(I))) return &launch_plane_instance_at<I, LYR, GRP>;
    else return nullptr;
}
template <bool LYR, bool GRP, unsigned... I>
static void launch_plane_instance(const RenderInst& v, std::integer_sequence<unsigned, I...>, const SceneDev& S, const LaunchDev& L, int blocks, hipStream_t st)
{
    static constexpr RenderLaunchFn table[kRenderInsts] = {plane_launcher<I, LYR, GRP>()...};
    const unsigned i = render_index(v);
    if (i >= kRenderInsts || !table[i]) kernel_not_built();
    census_record(kFastArith, census_of_planes(plane_mode(LYR, GRP)), i);
    table[i](S, L, blocks, st);
}
#endif
static void launch_instance_of(const RenderInst& v, const SceneDev& S, const LaunchDev& L, int blocks, hipStream_t st)
{
    constexpr std::make_integer_sequence<unsigned, kRenderInsts> all{};
    switch (plane_mode(L.layers != 0, L.groups != nullptr))
    {
    case PLANES_ONE: launch_instance(v, all, S, L, blocks, st); return;
#ifdef VP_RENDER_K_HAS_PLANES
    case PLANES_LAYERS: launch_plane_instance<true, false>(v, all, S, L, blocks, st); return;
    case PLANES_GROUPS: launch_plane_instance<false, true>(v, all, S, L, blocks, st); return;
    case PLANES_GROUP_LAYERS: launch_plane_instance<true, true>(v, all, S, L, blocks, st); return;
#endif
    }
    kernel_not_built();
}
// what launch_render / launch_render_fast and launch_render_light are
static void dispatch_render(const SceneDev& S, const LaunchDev& L, int est, int rng, bool quant, bool half, bool count, int lds_form, bool mis, int trk,
                            int blocks, hipStream_t st)
{
    launch_instance_of(render_instance(render_request(L, est, rng, quant, half, count, lds_form, mis, trk)), S, L, blocks, st);
}
static void dispatch_light(const SceneDev& S, const LaunchDev& L, int est, int rng, bool quant, bool count, int blocks, hipStream_t st)
{
    launch_instance_of(light_instance(est, rng, quant, count), S, L, blocks, st);
}

// ---- the approach walk: the camera rays' free flights through certified-empty cells, ahead of the integrator
constexpr int WALK_GLOBAL = 0, WALK_LOCAL = 1, WALK_LOCAL_TAB = 2;   // approach_k, approach_local_k<QUANT>, approach_local_tab_k
struct ApproachInst { int walk, rng; bool quant; };                  // (quant: approach_local_k's alone, set for the other two)
constexpr bool approach_built(const ApproachInst& v)
{
    if (v.walk != WALK_LOCAL && !v.quant) return false;
    if (kFastArith && v.rng == RNG_SAMPLERH) return false;
    if (kFastArith && kDevBuild && v.walk == WALK_LOCAL && !v.quant) return false;   // (no non-uchar local walk)
    return true;
}
constexpr unsigned kApproachInsts = 3u * 3u * 2u;
constexpr unsigned approach_index(const ApproachInst& v)
{
    return (unsigned)v.rng > 2u ? kApproachInsts : ((unsigned)v.walk * 3u + (unsigned)v.rng) * 2u + v.quant;
}
constexpr ApproachInst approach_at(unsigned i)
{
    ApproachInst v{};
    v.quant = i % 2u; i /= 2u;
    v.rng   = (int)(i % 3u); i /= 3u;
    v.walk  = (int)i;
    return v;
}

using ApproachLaunchFn = void (*)(const SceneDev&, const LaunchDev&, dim3, hipStream_t);
template <unsigned I>
static void launch_approach_at(const SceneDev& S, const LaunchDev& L, dim3 grid, hipStream_t st)
{
    constexpr ApproachInst v = approach_at(I);
    using RNG = typename RngOf<v.rng>::type;
    if constexpr (v.walk == WALK_GLOBAL) hipLaunchKernelGGL(approach_k<RNG>, grid, dim3(256), 0, st, S, L);
    else if constexpr (v.walk == WALK_LOCAL_TAB) hipLaunchKernelGGL(approach_local_tab_k<RNG>, grid, dim3(256), 0, st, S, L);
    else hipLaunchKernelGGL((approach_local_k<RNG, v.quant>), grid, dim3(256), 0, st, S, L);
}
template <unsigned I>
constexpr ApproachLaunchFn approach_launcher()
{
    if constexpr (approach_built(approach_at(I))) return &launch_approach_at<I>;
    else return nullptr;
}
template <unsigned... I>
static void launch_approach_walk(const SceneDev& S, const LaunchDev& L, int est, int rng, bool quant, hipStream_t st, std::integer_sequence<unsigned, I...>)
{
    static constexpr ApproachLaunchFn table[kApproachInsts] = {approach_launcher<I>()...};
    static_assert(VP_SEG_CAP > 64 && VP_SEG_CAP <= 128, "approach_local_tab_k copies a chain with two loads per lane");
    const unsigned sh = L.approach_fshift, spb = 256u >> sh;   // pixel slots per workgroup
    const dim3 grid((L.nslots + spb - 1u) / spb, ((unsigned)L.nframes + (1u << sh) - 1u) >> sh);
    ApproachInst v{};
    v.rng = rng;
    // (uchar bound table, the per-pixel segment table built: the set-up of every restart segment comes from it)
    v.walk  = est == EST_GLOBAL ? WALK_GLOBAL : (quant && L.seg_table && sh == 6u) ? WALK_LOCAL_TAB : WALK_LOCAL;
    v.quant = quant || v.walk == WALK_GLOBAL;
    const unsigned i = approach_index(v);
    if (i >= kApproachInsts || !table[i]) kernel_not_built();
    census_record(kFastArith, CENSUS_APPROACH, i);
    table[i](S, L, grid, st);
}
// what launch_approach / launch_approach_fast are
static void dispatch_approach(const SceneDev& S, const LaunchDev& L, int est, int rng, bool quant, hipStream_t st)
{
    launch_approach_walk(S, L, est, rng, quant, st, std::make_integer_sequence<unsigned, kApproachInsts>{});
}

// ---- the launch census (vp_kernels.h census_record; include/volpath.h vp_test_launch_census): which of the table entries above hold
// a kernel in this translation unit, evaluated at run time from the functions the tables are built from.  what census_built /
// census_built_fast are
static void dispatch_census_built(int kind, unsigned char* built, size_t count)
{
    for (size_t i = 0; i < count; i++)
    {
        bool b = false;
        if (kind == CENSUS_RENDER) b = i < kRenderInsts && render_built(render_at((unsigned)i));
        else if (kind == CENSUS_APPROACH) b = i < kApproachInsts && approach_built(approach_at((unsigned)i));
#ifdef VP_RENDER_K_HAS_PLANES
        else b = i < kRenderInsts && planes_built(render_at((unsigned)i));   // (the tables of the plane modes: one subset)
#endif
        built[i] = b;
    }
}
