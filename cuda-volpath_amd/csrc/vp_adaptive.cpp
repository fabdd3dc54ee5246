// vp_adaptive.cpp -- per-pixel statistics and adaptive sampling (include/volpath.h vp_pixel_stats): vp_render_frames_stats, a uniform
// render whose reduce also takes the statistics; vp_render_adaptive, serial rounds of do_render on the ACTIVE pixels -- a compaction of
// the context's cached lists by the FROZEN bit of the caller's records, before the first round and after each --; the output stage.
// The integrator kernels are the plain calls', on shorter lists; the frozen set lives in the caller's buffer and nowhere else.
// vp_render_adaptive_groups / vp_render_adaptive_layers: the same rounds on the two planes of a groups or layers render -- active means
// frozen in neither plane's record, and a round freezes both records of a pixel when both meet their plane's criterion.
// vp_render_adaptive_group_layers: the same on the three planes of a group-layers render, with three records per pixel.
// vp_render_adaptive_halves / vp_render_adaptive_planes_halves: the same rounds into the two halves of a half-buffer render -- active means
// frozen in none of the 2 N records; the halves reduces never freeze, so a round ends with a pass of its own (freeze_halves_k) that decides
// on the pooled records of the two halves, plane by plane.
// vp_denoise: the filter of the output stage that reads the records (vp_denoise.hip); vp_denoise_guided: the same with feature planes.
// vp_halves_variance, vp_filter_variance, vp_denoise_var: the variance stage of the cross-filter.  The three
// colour filter calls are one function, denoise_call, with the feature list and the variance plane as its optional parts.
// vp_cross_error, vp_select: per-pixel selection among filtered candidates by cross-buffer error estimates.
#include <climits>

#include "vp_state.h"

static_assert(sizeof(vp_pixel_stats) == 24 && sizeof(vp::PixelStatsDev) == sizeof(vp_pixel_stats), "vp_pixel_stats layout (include/volpath.h)");
static_assert(offsetof(vp_pixel_stats, sum_y2) == 8 && offsetof(vp_pixel_stats, n) == 16 && offsetof(vp_pixel_stats, flags) == 20, "vp_pixel_stats layout");
static_assert(sizeof(vp_adaptive_planes) == 24, "vp_adaptive_planes layout (include/volpath.h)");
static_assert(sizeof(vp_adaptive_planes3) == 32 && offsetof(vp_adaptive_planes3, floor_y) == 12, "vp_adaptive_planes3 layout (include/volpath.h)");
static_assert(offsetof(vp_adaptive_planes3, min_frames) == 24 && offsetof(vp_adaptive_planes3, round_frames) == 28, "vp_adaptive_planes3 layout");
static_assert(sizeof(vp_denoise_feature) == 16 && offsetof(vp_denoise_feature, channel) == 8 && offsetof(vp_denoise_feature, sigma) == 12, "vp_denoise_feature layout");
static_assert(VP_DENOISE_MAX_FEATURES == sizeof(vp::DenoiseFeaturesDev::chan) / sizeof(const float*), "DenoiseFeaturesDev holds VP_DENOISE_MAX_FEATURES features");
static_assert(offsetof(vp::PixelStatsDev, n) == 16 && offsetof(vp::PixelStatsDev, flags) == 20, "PixelStatsDev mirrors vp_pixel_stats");

namespace vph __attribute__((visibility("hidden")))
{
// the active pixels of the cached lists into G.d_act, their three counts into cnt: one small synchronisation (active: frozen in none of
// the records of S's planes)
static int compact_active(const Param* p, const PlaneSet& S, unsigned cnt[3])
{
    const unsigned n[3] = {G.n_general, G.n_light, G.n_miss};
    const unsigned nblocks = compact_blocks(n[0] + n[1] + n[2]);
    unsigned* d_totals = G.d_act_scratch + (size_t)3 * nblocks;
    launch_compact_active(G.d_tiles, n, p->width, S, G.d_act_scratch, d_totals, G.d_act, G.stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(cnt, d_totals, 3 * sizeof(unsigned), hipMemcpyDeviceToHost, G.stream));
    HIPCHK(hipStreamSynchronize(G.stream));
    if (cnt[0] > n[0] || cnt[1] > n[1] || cnt[2] > n[2]) return fail(VP_E_STATE, "active lists hold more pixels than the lists they come from");
    return VP_OK;
}
// the context's buffers for a list of n pixels: grown on demand, freed with the context
static int reserve_active(size_t n)
{
    const size_t words = (size_t)3 * compact_blocks((unsigned)n) + 4;
    if (n * sizeof(unsigned) <= G.d_act.bytes && words * sizeof(unsigned) <= G.d_act_scratch.bytes) return VP_OK;
    HIPCHK(hipStreamSynchronize(G.stream));
    HIPCHK(G.d_act.grow(n * sizeof(unsigned)));
    HIPCHK(G.d_act_scratch.grow(words * sizeof(unsigned)));
    return VP_OK;
}
// What the adaptive calls share once their arguments are checked: the rounds.  S carries the planes, their records and the criterion.
// Rounds are serial and run on the caller's stream: look-ahead batches stop, pipelined launches are waited for.
static int adaptive_rounds(const PlaneSet& S, int first_frame, int max_frames, int round_frames, const Param* p, vp_adaptive_result* result)
{
    int rc = la_quiesce();
    if (rc) return rc;
    if ((rc = vp_prepare(p))) return rc;   // the cached lists of p: what is compacted
    const size_t n_all = (size_t)G.n_general + G.n_light + G.n_miss;
    if (n_all == 0) return VP_OK;          // a shard without a tile
    if ((rc = reserve_active(n_all))) return rc;
    unsigned cnt[3] = {0, 0, 0};
    if ((rc = compact_active(p, S, cnt))) return rc;
    int done = 0;
    unsigned rounds = 0;
    unsigned long long samples = 0;
    while (done < max_frames && (size_t)cnt[0] + cnt[1] + cnt[2] > 0)
    {
        const int f = std::min(round_frames, max_frames - done);
        const PixelLists PL = {G.d_act, cnt[0], cnt[1], cnt[2]};
        if ((rc = do_render((vp_float4*)S.acc[0], first_frame + done, f, p, false, nullptr, &PL, &S))) return rc;
        if (S.halves)
        {
            // (the halves reduces never freeze: the round's decision, on the round's own list, before the list is compacted again)
            launch_freeze_halves(G.d_act, cnt[0] + cnt[1] + cnt[2], p->width, S, G.stream);
            HIPCHK(hipGetLastError());
        }
        samples += ((unsigned long long)cnt[0] + cnt[1] + cnt[2]) * (unsigned long long)f;   // (one per pixel and frame, not per plane)
        done += f; rounds++;
        if (result) { result->samples = samples; result->rounds = rounds; result->frames_used = (uint32_t)done; }
        if ((rc = compact_active(p, S, cnt))) return rc;   // round k + 1 needs round k's decisions
    }
    if (result) result->active_left = cnt[0] + cnt[1] + cnt[2];
    return VP_OK;
}
// vp_adaptive_planes / vp_adaptive_planes3 by their fields (all null / zero: the caller gave no struct)
struct AdaptiveArgs { const float *rel_tol, *floor_y; int min_frames, round_frames; };
template <class A> static AdaptiveArgs adaptive_args(const A* a) { return a ? AdaptiveArgs{a->rel_tol, a->floor_y, a->min_frames, a->round_frames} : AdaptiveArgs{}; }
// vp_render_adaptive_groups / _layers / _group_layers: the refusals of the definition, in its order, then the rounds
static int render_adaptive_planes(const char* fn, PlaneSet S, int first_frame, int max_frames, const Param* p, const AdaptiveArgs& a, vp_adaptive_result* result)
{
    static const char* const kCount[] = {"", "one", "two", "three"};
    if (result) memset(result, 0, sizeof *result);
    const int bad = plane_buffers_check(S, true);
    if (bad == 1 || !p || !a.rel_tol) return fail(VP_E_ARG, "%s: null pointer", fn);
    if (bad) return fail(VP_E_ARG, "%s: the %s accumulators, and the %s record buffers, are different buffers", fn, kCount[S.n()], kCount[S.n()]);
    if (max_frames <= 0 || first_frame < 0) return fail(VP_E_ARG, "%s: frames [%d, %d + %d) out of range", fn, first_frame, first_frame, max_frames);
    if (a.min_frames < 2) return fail(VP_E_ARG, "%s: min_frames %d (a variance estimate needs two samples)", fn, a.min_frames);
    if (a.round_frames < 1) return fail(VP_E_ARG, "%s: round_frames %d", fn, a.round_frames);
    for (int k = 0; k < S.n(); k++)
        if (!(a.rel_tol[k] >= 0.0f) || !(a.floor_y[k] >= 0.0f)) return fail(VP_E_ARG, "%s: rel_tol and floor_y must be numbers >= 0 (plane %d)", fn, k);
    int rc = plane_state_check(fn, S.groups());
    if (rc) return rc;
    if ((rc = ensure_device())) return rc;
    if ((rc = check_render(CHK_STATE | CHK_OPACITY, p, (long long)first_frame + max_frames - 1))) return rc;
    S.adaptive = true; S.min_frames = (unsigned)a.min_frames;
    for (int k = 0; k < S.n(); k++) { S.tol[k] = (double)a.rel_tol[k]; S.fl[k] = (double)a.floor_y[k]; }
    return adaptive_rounds(S, first_frame, max_frames, a.round_frames, p, result);
}
// vp_render_adaptive_halves / vp_render_adaptive_planes_halves: S holds the 2 N buffers of each kind as the caller handed them in (halves
// set); `planes`: the plane modes' state check, else the beauty call's.  The refusals of the definition, in its order, then the rounds.
static int render_adaptive_halves(const char* fn, PlaneSet S, bool planes, int first_frame, int max_frames, const Param* p, const AdaptiveArgs& a,
                                  vp_adaptive_result* result)
{
    const int bad = plane_buffers_check(S, true);
    if (bad == 1 || !p || !a.rel_tol) return fail(VP_E_ARG, "%s: null pointer", fn);
    if (bad) return fail(VP_E_ARG, "%s: the accumulators of the two halves, and their record buffers, are all different buffers", fn);
    if (max_frames <= 0 || first_frame < 0) return fail(VP_E_ARG, "%s: frames [%d, %d + %d) out of range", fn, first_frame, first_frame, max_frames);
    if (a.min_frames < 2) return fail(VP_E_ARG, "%s: min_frames %d (a variance estimate needs two samples)", fn, a.min_frames);
    if (a.round_frames < 1) return fail(VP_E_ARG, "%s: round_frames %d", fn, a.round_frames);
    for (int k = 0; k < S.n(); k++)
        if (!(a.rel_tol[k] >= 0.0f) || !(a.floor_y[k] >= 0.0f)) return fail(VP_E_ARG, "%s: rel_tol and floor_y must be numbers >= 0 (plane %d)", fn, k);
    int rc = VP_OK;
    if (planes && (rc = plane_state_check(fn, S.groups()))) return rc;
    if ((rc = ensure_device())) return rc;
    if (!planes && G.count) return fail(VP_E_STATE, "%s is not built for work counters", fn);
    if ((rc = check_render(CHK_STATE | CHK_OPACITY, p, (long long)first_frame + max_frames - 1))) return rc;
    S.adaptive = true; S.min_frames = (unsigned)a.min_frames;
    for (int k = 0; k < S.n(); k++) { S.tol[k] = (double)a.rel_tol[k]; S.fl[k] = (double)a.floor_y[k]; }
    return adaptive_rounds(S, first_frame, max_frames, a.round_frames, p, result);
}
// what the filter calls refuse alike, in the definition's order; fn is the call's name in the message
static int denoise_params_check(const char* fn, int width, int height, const vp_denoise_params* dp)
{
    if (width < 1 || height < 1 || (long long)width * height > INT_MAX) return fail(VP_E_ARG, "%s: image %d x %d", fn, width, height);
    if (dp->radius < 0 || dp->radius > VP_DENOISE_MAX_RADIUS) return fail(VP_E_ARG, "%s: radius %d outside 0..%d", fn, dp->radius, VP_DENOISE_MAX_RADIUS);
    if (dp->patch < 0 || dp->patch > VP_DENOISE_MAX_PATCH) return fail(VP_E_ARG, "%s: patch %d outside 0..%d", fn, dp->patch, VP_DENOISE_MAX_PATCH);
    if (!std::isfinite(dp->k) || !(dp->k > 0.0f)) return fail(VP_E_ARG, "%s: k must be a finite number > 0", fn);
    return VP_OK;
}
static int denoise_args_check(const char* fn, const vp_float4* dst, const vp_float4* src, const vp_pixel_stats* d_stats, const vp_float4* guide,
                              const vp_pixel_stats* d_guide_stats, int width, int height, const vp_denoise_params* dp)
{
    if (!dst || !src || !d_stats || !dp) return fail(VP_E_ARG, "%s: null pointer", fn);
    if (!guide != !d_guide_stats) return fail(VP_E_ARG, "%s: guide and d_guide_stats are given together or not at all", fn);
    if (dst == src || dst == guide) return fail(VP_E_ARG, "%s: in place is not possible (the call reads neighbours)", fn);
    return denoise_params_check(fn, width, height, dp);
}
// the feature list of a call into what the kernels take: each channel's address and g = 1 / (2 sigma^2) as the host rounds it
static int denoise_features_check(const char* fn, const vp_float4* dst, const vp_denoise_feature* features, int n_features, DenoiseFeaturesDev& fd)
{
    if (n_features < 0 || n_features > VP_DENOISE_MAX_FEATURES) return fail(VP_E_ARG, "%s: %d features outside 0..%d", fn, n_features, VP_DENOISE_MAX_FEATURES);
    if (n_features > 0 && !features) return fail(VP_E_ARG, "%s: %d features and no array of them", fn, n_features);
    for (int j = 0; j < n_features; j++)
    {
        const vp_denoise_feature& f = features[j];
        if (!f.plane) return fail(VP_E_ARG, "%s: feature %d has no plane", fn, j);
        if (f.plane == dst) return fail(VP_E_ARG, "%s: feature %d is dst (the call reads neighbours)", fn, j);
        if (f.channel < 0 || f.channel > 3) return fail(VP_E_ARG, "%s: feature %d: channel %d outside 0..3", fn, j, f.channel);
        if (!std::isfinite(f.sigma) || !(f.sigma > 0.0f)) return fail(VP_E_ARG, "%s: feature %d: sigma must be a finite number > 0", fn, j);
        const float g = 1.0f / ((2.0f * f.sigma) * f.sigma);
        if (!std::isfinite(g) || !(g > 0.0f)) return fail(VP_E_ARG, "%s: feature %d: 1 / (2 sigma^2) of sigma %g is not a finite number > 0", fn, j, (double)f.sigma);
        fd.chan[j] = (const float*)f.plane + f.channel;
        fd.g[j] = g;
    }
    fd.n = n_features;
    return VP_OK;
}
static int denoise_lds_check(const char* fn, const vp_denoise_params* dp, int n_features)
{
    if (G.denoise_form == 0 && denoise_guided_lds_bytes(dp->radius, dp->patch, n_features) > DENOISE_LDS_LIMIT)
        return fail(VP_E_STATE, "%s: radius %d, patch %d, %d features need %zu bytes of LDS, a workgroup has %zu", fn, dp->radius, dp->patch, n_features,
                    denoise_guided_lds_bytes(dp->radius, dp->patch, n_features), DENOISE_LDS_LIMIT);
    return VP_OK;
}
// vp_denoise, vp_denoise_guided and vp_denoise_var: fn is the name the call reports under, d_sample_var and features what it has of
// the two optional parts.  vp_denoise_var without its plane is vp_denoise_guided in all it does and reports, and that one without
// features is vp_denoise, once the feature count has been checked under the name it was given to
static int denoise_call(const char* fn, vp_float4* dst, const vp_float4* src, const vp_pixel_stats* d_stats, const vp_float4* guide,
                        const vp_pixel_stats* d_guide_stats, const float* d_sample_var, const vp_denoise_feature* features, int n_features, int width, int height,
                        const vp_denoise_params* dp)
{
    DenoiseFeaturesDev fd = {};
    int rc = denoise_features_check(fn, dst, features, n_features, fd);
    if (rc) return rc;
    if (!d_sample_var && n_features == 0) fn = "vp_denoise";
    if ((rc = denoise_args_check(fn, dst, src, d_stats, guide, d_guide_stats, width, height, dp))) return rc;
    if (d_sample_var && (const void*)d_sample_var == (const void*)dst) return fail(VP_E_ARG, "%s: d_sample_var is dst (the call reads neighbours)", fn);
    if ((d_sample_var || n_features) && (rc = denoise_lds_check(fn, dp, n_features))) return rc;
    if ((rc = ensure_device())) return rc;
    if (!guide) { guide = src; d_guide_stats = d_stats; }
    launch_denoise((float4*)dst, (const float4*)src, (const PixelStatsDev*)d_stats, (const float4*)guide, (const PixelStatsDev*)d_guide_stats, d_sample_var, fd, width,
                   height, dp->radius, dp->patch, dp->k * dp->k, G.denoise_form, G.stream);
    HIPCHK(hipGetLastError());
    G.last_denoise_form = G.denoise_form;
    return VP_OK;
}
}  // namespace vph

using namespace vph;

extern "C" {
int vp_render_frames_stats(vp_float4* d_output, vp_pixel_stats* d_stats, int first_frame, int n_frames, const Param* p)
{
    if (!d_output || !d_stats || !p || n_frames <= 0 || first_frame < 0) return fail(VP_E_ARG, "vp_render_frames_stats: bad arguments");
    const PlaneSet S = plane_set(PLANES_ONE, d_output, nullptr, nullptr, d_stats);
    return do_render(d_output, first_frame, n_frames, p, false, nullptr, nullptr, &S);
}
int vp_render_adaptive(vp_float4* d_output, vp_pixel_stats* d_stats, int first_frame, int max_frames, const Param* p, const vp_adaptive* a,
                       vp_adaptive_result* result)
{
    if (result) memset(result, 0, sizeof *result);
    if (!d_output || !d_stats || !p || !a) return fail(VP_E_ARG, "vp_render_adaptive: null pointer");
    if (max_frames <= 0 || first_frame < 0) return fail(VP_E_ARG, "vp_render_adaptive: frames [%d, %d + %d) out of range", first_frame, first_frame, max_frames);
    if (a->min_frames < 2) return fail(VP_E_ARG, "vp_render_adaptive: min_frames %d (a variance estimate needs two samples)", a->min_frames);
    if (a->round_frames < 1) return fail(VP_E_ARG, "vp_render_adaptive: round_frames %d", a->round_frames);
    if (!(a->rel_tol >= 0.0f) || !(a->floor_y >= 0.0f)) return fail(VP_E_ARG, "vp_render_adaptive: rel_tol and floor_y must be numbers >= 0");
    int rc = ensure_device();
    if (rc) return rc;
    if (G.count) return fail(VP_E_STATE, "vp_render_adaptive is not built for work counters");
    if ((rc = check_render(CHK_STATE | CHK_OPACITY, p, (long long)first_frame + max_frames - 1))) return rc;
    PlaneSet S = plane_set(PLANES_ONE, d_output, nullptr, nullptr, d_stats);
    S.adaptive = true; S.min_frames = (unsigned)a->min_frames;
    S.tol[0] = (double)a->rel_tol; S.fl[0] = (double)a->floor_y;
    return adaptive_rounds(S, first_frame, max_frames, a->round_frames, p, result);
}
int vp_render_adaptive_groups(vp_float4* d_sun, vp_float4* d_sky, vp_pixel_stats* d_sun_stats, vp_pixel_stats* d_sky_stats, int first_frame, int max_frames,
                              const Param* p, const vp_adaptive_planes* a, vp_adaptive_result* result)
{
    return render_adaptive_planes("vp_render_adaptive_groups", plane_set(PLANES_GROUPS, d_sun, d_sky, nullptr, d_sun_stats, d_sky_stats), first_frame, max_frames, p,
                                  adaptive_args(a), result);
}
int vp_render_adaptive_layers(vp_float4* d_fg, vp_float4* d_trans, vp_pixel_stats* d_fg_stats, vp_pixel_stats* d_trans_stats, int first_frame, int max_frames,
                              const Param* p, const vp_adaptive_planes* a, vp_adaptive_result* result)
{
    return render_adaptive_planes("vp_render_adaptive_layers", plane_set(PLANES_LAYERS, d_fg, d_trans, nullptr, d_fg_stats, d_trans_stats), first_frame, max_frames, p,
                                  adaptive_args(a), result);
}
int vp_render_adaptive_group_layers(vp_float4* d_sun, vp_float4* d_sky, vp_float4* d_trans, vp_pixel_stats* d_sun_stats, vp_pixel_stats* d_sky_stats,
                                    vp_pixel_stats* d_trans_stats, int first_frame, int max_frames, const Param* p, const vp_adaptive_planes3* a,
                                    vp_adaptive_result* result)
{
    return render_adaptive_planes("vp_render_adaptive_group_layers", plane_set(PLANES_GROUP_LAYERS, d_sun, d_sky, d_trans, d_sun_stats, d_sky_stats, d_trans_stats),
                                  first_frame, max_frames, p, adaptive_args(a), result);
}
int vp_render_adaptive_halves(vp_float4* d_h0, vp_float4* d_h1, vp_pixel_stats* d_h0_stats, vp_pixel_stats* d_h1_stats, int first_frame, int max_frames,
                              const Param* p, const vp_adaptive* a, vp_adaptive_result* result)
{
    static const char fn[] = "vp_render_adaptive_halves";
    if (result) memset(result, 0, sizeof *result);
    if (!a) return fail(VP_E_ARG, "%s: null pointer", fn);
    PlaneSet S = plane_set(PLANES_ONE, d_h0, d_h1, nullptr, d_h0_stats, d_h1_stats);
    S.halves = true;
    return render_adaptive_halves(fn, S, false, first_frame, max_frames, p, AdaptiveArgs{&a->rel_tol, &a->floor_y, a->min_frames, a->round_frames}, result);
}
int vp_render_adaptive_planes_halves(int mode, const vp_plane_bufs* h0, const vp_plane_bufs* h1, int first_frame, int max_frames, const Param* p,
                                     const vp_adaptive_planes3* a, vp_adaptive_result* result)
{
    static const char fn[] = "vp_render_adaptive_planes_halves";
    if (result) memset(result, 0, sizeof *result);
    if (mode != VP_PLANES_LAYERS && mode != VP_PLANES_GROUPS && mode != VP_PLANES_GROUP_LAYERS) return fail(VP_E_ARG, "%s: unknown mode %d", fn, mode);
    if (!h0 || !h1 || !a) return fail(VP_E_ARG, "%s: null pointer", fn);
    PlaneSet S = {};
    S.mode = mode; S.halves = true;
    for (int h = 0; h < 2; h++)
        for (int k = 0; k < S.n(); k++)
        {
            S.acc[h * S.n() + k] = (float4*)(h ? h1 : h0)->acc[k];
            S.rec[h * S.n() + k] = (PixelStatsDev*)(h ? h1 : h0)->rec[k];
        }
    return render_adaptive_halves(fn, S, true, first_frame, max_frames, p, adaptive_args(a), result);
}
int vp_scale_by_count(vp_float4* dst, const vp_float4* src, const vp_pixel_stats* d_stats, int size, float scale)
{
    if (!dst || !src || !d_stats || size < 0) return fail(VP_E_ARG, "vp_scale_by_count: bad arguments");
    int rc = ensure_device();
    if (rc) return rc;
    if (size) launch_scale_by_count((float4*)dst, (const float4*)src, (const PixelStatsDev*)d_stats, size, scale, G.stream);
    HIPCHK(hipGetLastError());
    return VP_OK;
}
int vp_stats_rel_error(float* dst, const vp_pixel_stats* d_stats, int size, float floor_y)
{
    if (!dst || !d_stats || size < 0 || !(floor_y >= 0.0f)) return fail(VP_E_ARG, "vp_stats_rel_error: bad arguments");
    int rc = ensure_device();
    if (rc) return rc;
    if (size) launch_stats_rel_error(dst, (const PixelStatsDev*)d_stats, size, floor_y, G.stream);
    HIPCHK(hipGetLastError());
    return VP_OK;
}
int vp_merge_halves(vp_float4* dst, float* d_resid, const vp_float4* a, const vp_pixel_stats* a_stats, const vp_float4* b, const vp_pixel_stats* b_stats,
                    int size, float floor_y)
{
    if (!dst || !a || !b || !a_stats || !b_stats) return fail(VP_E_ARG, "vp_merge_halves: null pointer");
    if (size < 0) return fail(VP_E_ARG, "vp_merge_halves: size %d", size);
    if (d_resid && (!std::isfinite(floor_y) || !(floor_y > 0.0f))) return fail(VP_E_ARG, "vp_merge_halves: floor_y must be a finite number > 0");
    int rc = ensure_device();
    if (rc) return rc;
    if (size)
        launch_merge_halves((float4*)dst, d_resid, (const float4*)a, (const PixelStatsDev*)a_stats, (const float4*)b, (const PixelStatsDev*)b_stats, size, floor_y,
                            G.stream);
    HIPCHK(hipGetLastError());
    return VP_OK;
}
int vp_accumulate_stats(vp_pixel_stats* dst, const vp_pixel_stats* src, size_t n)
{
    if (!dst || !src) return fail(VP_E_ARG, "vp_accumulate_stats: null pointer");
    int rc = ensure_device();
    if (rc) return rc;
    if (n) launch_accumulate_stats((PixelStatsDev*)dst, (const PixelStatsDev*)src, n, G.stream);
    HIPCHK(hipGetLastError());
    return VP_OK;
}
int vp_denoise(vp_float4* dst, const vp_float4* src, const vp_pixel_stats* d_stats, const vp_float4* guide, const vp_pixel_stats* d_guide_stats,
               int width, int height, const vp_denoise_params* dp)
{
    return denoise_call("vp_denoise", dst, src, d_stats, guide, d_guide_stats, nullptr, nullptr, 0, width, height, dp);
}
int vp_denoise_guided(vp_float4* dst, const vp_float4* src, const vp_pixel_stats* d_stats, const vp_float4* guide, const vp_pixel_stats* d_guide_stats,
                      const vp_denoise_feature* features, int n_features, int width, int height, const vp_denoise_params* dp)
{
    return denoise_call("vp_denoise_guided", dst, src, d_stats, guide, d_guide_stats, nullptr, features, n_features, width, height, dp);
}
int vp_denoise_var(vp_float4* dst, const vp_float4* src, const vp_pixel_stats* d_stats, const vp_float4* guide, const vp_pixel_stats* d_guide_stats,
                   const float* d_sample_var, const vp_denoise_feature* features, int n_features, int width, int height, const vp_denoise_params* dp)
{
    return denoise_call(d_sample_var ? "vp_denoise_var" : "vp_denoise_guided", dst, src, d_stats, guide, d_guide_stats, d_sample_var, features, n_features, width, height, dp);
}
int vp_halves_variance(float* d_u, float* d_q, const vp_pixel_stats* a_stats, const vp_pixel_stats* b_stats, int size)
{
    if (!d_u || !a_stats || !b_stats) return fail(VP_E_ARG, "vp_halves_variance: null pointer");
    if (size < 0) return fail(VP_E_ARG, "vp_halves_variance: size %d", size);
    int rc = ensure_device();
    if (rc) return rc;
    if (size) launch_halves_variance(d_u, d_q, (const PixelStatsDev*)a_stats, (const PixelStatsDev*)b_stats, size, G.stream);
    HIPCHK(hipGetLastError());
    return VP_OK;
}
int vp_filter_variance(float* dst, const float* u, const float* q, int width, int height, const vp_denoise_params* vp)
{
    if (!dst || !u || !q || !vp) return fail(VP_E_ARG, "vp_filter_variance: null pointer");
    if (dst == u || dst == q) return fail(VP_E_ARG, "vp_filter_variance: in place is not possible (the call reads neighbours)");
    int rc = denoise_params_check("vp_filter_variance", width, height, vp);
    if (rc) return rc;
    if ((rc = ensure_device())) return rc;
    launch_filter_variance(dst, u, q, width, height, vp->radius, vp->patch, vp->k * vp->k, G.denoise_form, G.stream);
    HIPCHK(hipGetLastError());
    G.last_denoise_form = G.denoise_form;
    return VP_OK;
}
int vp_cross_error(float* d_err, const vp_float4* fa, const vp_float4* fb, const vp_float4* h0, const vp_pixel_stats* s0, const vp_float4* h1,
                   const vp_pixel_stats* s1, int size)
{
    if (!d_err || !fa || !fb || !h0 || !s0 || !h1 || !s1) return fail(VP_E_ARG, "vp_cross_error: null pointer");
    for (const void* in : {(const void*)fa, (const void*)fb, (const void*)h0, (const void*)s0, (const void*)h1, (const void*)s1})
        if (in == (const void*)d_err) return fail(VP_E_ARG, "vp_cross_error: d_err is one of the inputs");
    if (size < 0) return fail(VP_E_ARG, "vp_cross_error: size %d", size);
    int rc = ensure_device();
    if (rc) return rc;
    if (size)
        launch_cross_error(d_err, (const float4*)fa, (const float4*)fb, (const float4*)h0, (const PixelStatsDev*)s0, (const float4*)h1, (const PixelStatsDev*)s1, size,
                           G.stream);
    HIPCHK(hipGetLastError());
    return VP_OK;
}
int vp_select(vp_float4* dst, uint8_t* d_index, const vp_float4* const* images, const float* const* errors, int n, int width, int height,
              const vp_select_params* sp)
{
    if (!dst || !images || !errors || !sp) return fail(VP_E_ARG, "vp_select: null pointer");
    if (n < 1 || n > VP_SELECT_MAX_CANDIDATES) return fail(VP_E_ARG, "vp_select: %d candidates outside 1..%d", n, VP_SELECT_MAX_CANDIDATES);
    static_assert(VP_SELECT_MAX_CANDIDATES == SELECT_MAX, "the kernels' argument block holds VP_SELECT_MAX_CANDIDATES pointers of each kind");
    SelectDev S = {};
    for (int c = 0; c < n; c++)
    {
        if (!images[c] || !errors[c]) return fail(VP_E_ARG, "vp_select: candidate %d has no %s", c, images[c] ? "error plane" : "image");
        if ((const void*)errors[c] == (const void*)dst) return fail(VP_E_ARG, "vp_select: error plane %d is dst (the call reads its neighbours)", c);
        S.img[c] = (const float4*)images[c];
        S.err[c] = errors[c];
    }
    S.n = n;
    if (d_index && (const void*)d_index == (const void*)dst) return fail(VP_E_ARG, "vp_select: d_index is dst");
    if (width < 1 || height < 1 || (long long)width * height > INT_MAX) return fail(VP_E_ARG, "vp_select: image %d x %d", width, height);
    if (sp->smooth_radius < 0 || sp->smooth_radius > VP_SELECT_MAX_RADIUS)
        return fail(VP_E_ARG, "vp_select: smooth_radius %d outside 0..%d", sp->smooth_radius, VP_SELECT_MAX_RADIUS);
    if (sp->blend_radius < 0 || sp->blend_radius > VP_SELECT_MAX_RADIUS)
        return fail(VP_E_ARG, "vp_select: blend_radius %d outside 0..%d", sp->blend_radius, VP_SELECT_MAX_RADIUS);
    int rc = ensure_device();
    if (rc) return rc;
    launch_select((float4*)dst, d_index, S, width, height, sp->smooth_radius, sp->blend_radius, G.denoise_form, G.stream);
    HIPCHK(hipGetLastError());
    G.last_denoise_form = G.denoise_form;
    return VP_OK;
}
int vp_set_denoise_form(int form)
{
    if (form != 0 && form != 1) return fail(VP_E_ARG, "vp_set_denoise_form: unknown form %d", form);
    G.denoise_form = form;
    return VP_OK;
}
int vp_last_denoise_form(void) { return G.last_denoise_form; }
}  // extern "C"
