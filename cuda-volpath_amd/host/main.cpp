// main.cpp -- volpath_render: headless driver in place of the reference's GLUT shell (host.cpp:1284-1403).
// It performs main()'s set-up sequence against the SAME entry points (init_cuda, set_texture_filter_mode,
// copy_inv_model_matrix, copy_inv_view_matrix, init_envmap, set_sun, precompute_opacity, render_kernel,
// scale / gamma_correct) and writes what the 'c' key captures (host.cpp:585-610): a .ppm of the
// gamma-corrected image or a .hdr of the scaled accumulator.
#include <chrono>
#include <cstdarg>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "camera.h"
#include "image.h"
#include "param.h"  // before volpath.h: the host spells Param with float3 members (same 44 bytes)
#include "multigpu.h"
#include "sky.h"
#include "volume_io.h"
#include "volpath.h"

static void usage()
{
    printf("volpath_render [--julia N | --bin file.bin | --vdb file.vdb] [--size W H] [--spp N] [--preset 0..12]\n"
           "               [--volume-format u8|f32|f16]     how --bin / --vdb densities are stored on the device (vp_init_volume): u8, the\n"
           "                                                default, quantises to bytes (8-byte cells); f32 keeps the floats (32-byte cells);\n"
           "                                                f16 rounds them to IEEE binary16 (16-byte cells, rendered as the widened floats).\n"
           "                                                --julia voxelises to bytes: u8 only\n"
           "               [--density D] [--g G] [--estimator decomp|global|bounded] [--brick B] [--rng samplerh|philox|philox7]\n"
           "               [--tracking spectral|scalar|multichannel] [--env passive|mis]\n"
           "               [--arith exact|fast]             fast: hardware log/exp/rcp/sqrt/sin/cos in the integrator, within the\n"
           "                                                tolerance of include/volpath.h (--rng philox|philox7, spectral, passive)\n"
           "               [--aa 1|2|4|8]                   anti-aliasing: stratified sub-pixel camera rays on an S x S lattice per pixel\n"
           "                                                (vp_set_subpixel: a box-filtered pixel; default 1, or VP_SUBPIXEL)\n"
           "               [--noise TOL [--min-spp N] [--round N] [--noise-out FILE.hdr]]\n"
           "                                                adaptive sampling (vp_render_adaptive): a pixel is sampled in rounds of --round\n"
           "                                                frames (default 32) until the estimated standard error of its mean luminance is\n"
           "                                                at most TOL x max(mean, 1e-3), from --min-spp frames (default 16) on; --spp is the\n"
           "                                                maximum.  The image is sum / n per pixel; --noise-out writes the noise map\n"
           "                                                (vp_stats_rel_error) as HDR.  One GPU: statistics are not reduced across ranks\n"
           "               [--denoise [--denoise-radius R] [--denoise-patch F] [--denoise-k K]]\n"
           "                                                --out receives the NL-means filtered mean image (vp_denoise: weights from the\n"
           "                                                per-pixel luminance variance; search window (2R+1)^2, R <= 10, default 5; patch\n"
           "                                                (2F+1)^2, F <= 3, default 1; strength K > 0, default 0.45).  The frames then go\n"
           "                                                through vp_render_frames_stats (or --noise).  One GPU, like --noise\n"
           "               [--denoise-features [--denoise-sigma-alpha SA] [--denoise-sigma-depth SZ]]\n"
           "                                                with --denoise: the filter is vp_denoise_guided, its weights cut by the feature\n"
           "                                                pass's planes (vp_render_features at --feature-step / --depth-tau, run first):\n"
           "                                                the green opacity alpha.y with sigma SA (default 0.2), the depth at which the\n"
           "                                                optical depth reaches TAU with sigma SZ (default 0.2, in scene units) and the\n"
           "                                                cover flag with SA.  One GPU; not with --aa above 1\n"
           "               [--denoise-cross [--resid-out FILE.hdr]]\n"
           "                                                implies --denoise; the frames go through vp_render_frames_halves_stats into\n"
           "                                                two half-buffers (even and odd frames; with --aa S blocks of S^2 frames), each\n"
           "                                                half is filtered with the weights of the OTHER (two vp_denoise_guided calls,\n"
           "                                                roles swapped) and --out is their vp_merge_halves.  --denoise-radius, -patch, -k\n"
           "                                                and --denoise-features apply.  --resid-out writes the residual-error map: half\n"
           "                                                the disagreement of the two filtered halves over max(mean, 1e-3), as HDR.\n"
           "                                                One GPU; not with --noise or any plane output or plane filter\n"
           "               [--denoise-var [--denoise-var-radius R] [--denoise-var-patch F] [--denoise-var-k K] [--var-out FILE.hdr]]\n"
           "                                                implies --denoise-cross, with the variance stage in front: the per-sample\n"
           "                                                luminance variance pooled from both halves (vp_halves_variance), smoothed by a\n"
           "                                                small NL-means pass of its own (vp_filter_variance; R default 1, F default 3, K\n"
           "                                                default 0.45), and both halves filtered with that one plane as their guide's\n"
           "                                                variance (vp_denoise_var).  --var-out writes the filtered plane as HDR.  The\n"
           "                                                refusals of --denoise-cross apply\n"
           "               [--denoise-select [--denoise-select-radius R] [--denoise-select-patch F] [--denoise-select-smooth S]\n"
           "                [--denoise-select-blend B] [--select-out FILE.hdr]]\n"
           "                                                implies --denoise-var, at TWO windows with a per-pixel choice between them:\n"
           "                                                candidate 0 is (--denoise-radius, --denoise-patch), candidate 1 is (R default 10,\n"
           "                                                F default 3), --denoise-k is shared.  Each candidate's error is estimated per\n"
           "                                                pixel from the half-buffers (vp_cross_error), the error maps are box-smoothed at\n"
           "                                                radius S (default 1), the smaller wins, and the picks are blended over radius B\n"
           "                                                (default 1) (vp_select; S and B 0..3).  --select-out writes the index map as HDR.\n"
           "                                                --denoise-features applies to both candidates.  The refusals of --denoise-var\n"
           "                                                apply; not with --resid-out\n"
           "               [--layers-out PREFIX] [--over R G B]\n"
           "                                                compositing layers (vp_render_frames_layers): the frames are rendered as a\n"
           "                                                foreground F and a per-channel transmittance T, pixel = F + T o B for any\n"
           "                                                background B.  --layers-out writes the two mean layers as PREFIX_fg.hdr and\n"
           "                                                PREFIX_trans.hdr (trans.w: the fraction of unscattered samples); --over writes\n"
           "                                                the composite over the constant colour (R, G, B) to --out (vp_composite; its w is\n"
           "                                                coverage).  Without --over no --out image is written: the context's own sky is in\n"
           "                                                neither layer.  One GPU; not with --noise or --denoise; spectral, --env passive, --arith exact\n"
           "               [--groups-out PREFIX] [--sun-gain R G B] [--sky-gain R G B]\n"
           "                                                light groups (vp_render_frames_groups): the frames are rendered once, what the\n"
           "                                                sun lights and what the sky lights in accumulators of their own.  --groups-out\n"
           "                                                writes the two mean images as PREFIX_sun.hdr and PREFIX_sky.hdr; --out receives\n"
           "                                                sun * sun-gain + sky * sky-gain per channel (vp_relight; gains default to 1 1 1).\n"
           "                                                One GPU; not with --noise, --denoise or --layers-out / --over; spectral, --env\n"
           "                                                passive, --arith exact\n"
           "               [--groups-denoise] [--layers-denoise]\n"
           "                                                with --groups-out / a gain flag, or with --layers-out / --over: the frames go\n"
           "                                                through vp_render_frames_groups_stats / vp_render_frames_layers_stats (the same\n"
           "                                                accumulator bits, one record buffer per plane) and each plane is filtered by\n"
           "                                                vp_denoise with its own records as guide (--denoise-radius, --denoise-patch and\n"
           "                                                --denoise-k apply).  The PREFIX files are then the denoised means, --out their\n"
           "                                                vp_relight / vp_composite; w is never filtered, so coverage stays exact.  One GPU;\n"
           "                                                not with --noise or --denoise\n"
           "               [--plane-noise TOL0 TOL1 [--min-spp N] [--round N] [--plane-noise-out PREFIX]]\n"
           "                                                with --groups-out / a gain flag, or with --layers-out / --over: adaptive sampling\n"
           "                                                on the two planes (vp_render_adaptive_groups / vp_render_adaptive_layers).  A pixel\n"
           "                                                is sampled, in both planes, until the estimated standard error of EACH plane's mean\n"
           "                                                luminance is at most TOLk x max(mean, floor): TOL0 and a floor of 1e-3 for sun / fg,\n"
           "                                                TOL1 for sky (floor 1e-3) / trans (floor 1e-2); --min-spp and --round as for\n"
           "                                                --noise, --spp the maximum.  Each plane is written as sum / n per pixel, --out is\n"
           "                                                their vp_relight / vp_composite; with --groups-denoise / --layers-denoise the means\n"
           "                                                are vp_denoise's from the adaptive records.  --plane-noise-out writes one noise map\n"
           "                                                per plane (PREFIX_sun.hdr ...).  One GPU; not with --noise or --denoise\n"
           "               [--planes-out PREFIX] [--planes-denoise]\n"
           "                                                light groups and layers of the same paths in one render\n"
           "                                                (vp_render_frames_group_layers): --planes-out writes the three mean planes as\n"
           "                                                PREFIX_sun.hdr, PREFIX_sky.hdr and PREFIX_trans.hdr.  --sun-gain, --sky-gain and\n"
           "                                                --over (default 0 0 0) are then its parameters and --out receives\n"
           "                                                sun * sun-gain + sky * sky-gain + trans * over (vp_relight_composite; w: coverage).\n"
           "                                                --planes-denoise: the frames go through vp_render_frames_group_layers_stats and each\n"
           "                                                plane is filtered by vp_denoise with its own records.  One GPU; not with --noise,\n"
           "                                                --denoise, --groups-out, --layers-out or --plane-noise; spectral, --env passive,\n"
           "                                                --arith exact\n"
           "               [--planes-noise TOL_SUN TOL_SKY TOL_TRANS [--min-spp N] [--round N] [--planes-noise-out PREFIX]]\n"
           "                                                with --planes-out: adaptive sampling on the three planes\n"
           "                                                (vp_render_adaptive_group_layers).  A pixel is sampled, in all three planes, until\n"
           "                                                the estimated standard error of EACH plane's mean luminance is at most\n"
           "                                                TOLk x max(mean, floor), with floors 1e-3 (sun), 1e-3 (sky) and 1e-2 (trans);\n"
           "                                                --min-spp and --round as for --noise, --spp the maximum.  Each plane is written as\n"
           "                                                sum / n per pixel, --out is their vp_relight_composite; with --planes-denoise the\n"
           "                                                means are vp_denoise's from the adaptive records.  --planes-noise-out writes one\n"
           "                                                noise map per plane (PREFIX_sun.hdr, PREFIX_sky.hdr, PREFIX_trans.hdr).  One GPU;\n"
           "                                                not with --noise or --denoise\n"
           "               [--layers-denoise-cross] [--groups-denoise-cross] [--planes-denoise-cross]\n"
           "               [--plane-denoise-var] [--plane-resid-out PREFIX]\n"
           "                                                the cross-filter on planes: each implies the mode's --layers-denoise /\n"
           "                                                --groups-denoise / --planes-denoise and needs what that flag needs.  The frames go\n"
           "                                                through vp_render_frames_planes_halves_stats into two halves of every plane (even\n"
           "                                                and odd frames; with --aa S blocks of S^2 frames); each plane's mean is the\n"
           "                                                vp_merge_halves of its two halves, each filtered by vp_denoise with the OTHER\n"
           "                                                half as guide (--denoise-radius, -patch, -k apply; no features, as for the\n"
           "                                                mode's -denoise flag); --out is their vp_composite / vp_relight /\n"
           "                                                vp_relight_composite as before.  --plane-denoise-var puts the variance stage in\n"
           "                                                front of each plane's pair of filters (vp_halves_variance, vp_filter_variance,\n"
           "                                                vp_denoise_var; --denoise-var-radius, -patch, -k apply).  --plane-resid-out\n"
           "                                                writes one residual map per plane (PREFIX_sun.hdr ...), with the plane's floor\n"
           "                                                (1e-3; trans 1e-2).  One GPU; not with --noise, --plane-noise, --planes-noise or\n"
           "                                                --denoise-cross / -var / -select\n"
           "               [--cross-noise TOL [--min-spp N] [--round N] [--cross-noise-out FILE.hdr]]\n"
           "                                                adaptive sampling into the two half-buffers (vp_render_adaptive_halves): implies\n"
           "                                                --denoise-cross and composes with --denoise-var, --denoise-select,\n"
           "                                                --denoise-features and --resid-out.  A pixel is sampled in rounds of --round frames,\n"
           "                                                frame f into its half alone, until each half holds two samples, both together\n"
           "                                                --min-spp and the estimated standard error of their POOLED mean luminance is at\n"
           "                                                most TOL x max(mean, 1e-3); --spp is the maximum.  With --aa S the round is rounded\n"
           "                                                up to a multiple of 2 S^2, so that every round feeds both halves equally.\n"
           "                                                --cross-noise-out writes the noise map of the pooled records (vp_accumulate_stats\n"
           "                                                of the two halves, vp_stats_rel_error) as HDR.  One GPU; not with --noise\n"
           "               [--plane-cross-noise TOL0 TOL1] [--planes-cross-noise TOL_SUN TOL_SKY TOL_TRANS] [--plane-cross-noise-out PREFIX]\n"
           "                                                the same on the halves of every plane (vp_render_adaptive_planes_halves):\n"
           "                                                --plane-cross-noise with --layers-denoise-cross or --groups-denoise-cross,\n"
           "                                                --planes-cross-noise with --planes-denoise-cross.  Each plane's two records are\n"
           "                                                pooled and held to its own tolerance, with the floors of --plane-noise /\n"
           "                                                --planes-noise; a pixel is sampled until every plane meets its own.\n"
           "                                                --plane-cross-noise-out writes one pooled noise map per plane (PREFIX_sun.hdr ...).\n"
           "                                                One GPU; not with --noise, --plane-noise or --planes-noise\n"
           "               [--features-out PREFIX [--feature-step DT] [--depth-tau TAU]]\n"
           "                                                the feature pass (vp_render_features), a deterministic march along every pixel's\n"
           "                                                camera ray with step DT (default 0.001), after the render and beside every other\n"
           "                                                output: PREFIX_alpha.hdr = the expected per-channel opacity, PREFIX_depth.hdr =\n"
           "                                                (first matter, where the luminance optical depth reaches TAU (default ln 2), last\n"
           "                                                matter) as distances along the ray.  RGBE cannot hold inf: a depth that does not\n"
           "                                                exist (no matter on the ray, TAU never reached) is written as 0 here; the library\n"
           "                                                call keeps +inf.  Pixel-centre rays whatever --aa says; rank 0 marches the whole\n"
           "                                                image with --gpus\n"
           "               [--sun X Y] [--batch F] [--out name(.ppm|.hdr)]\n"
           "               [--gpus N [--devices a,b,...]]   N contexts, pixel tiles dealt by vp_set_shard, one RCCL reduce;\n"
           "                                                a repeated device (e.g. --gpus 2 --devices 0,0) shares one GPU\n"
           "                                                (distinct devices: the RCCL path has run with one rank only so far -- UNVERIFIED\n"
           "                                                between GPUs; --rccl-selftest checks that RCCL loads and reduces here)\n"
           "               [--rccl-selftest [device]]       load RCCL, one-rank communicator, one reduce: the calls of the N > 1 path\n");
}

// ---- the two ways a run ends early
enum Hint { PLAIN, USAGE };
// a refused command line: the message, usage() where the refusal is about a flag's operand, status 2
[[noreturn]] static void refuse(Hint hint, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
    if (hint == USAGE) usage();
    exit(2);
}
// a failed library call: its message, status 1 (exit() flushes what was printed; files already written stay; nothing is freed)
static void must(bool failed)
{
    if (!failed) return;
    fprintf(stderr, "%s\n", vp_last_error());
    exit(1);
}

static void need(int argc, int i, int n) { if (i + n >= argc) { usage(); exit(2); } }
// the n floats behind flag argv[i], each passing ok(): else "FLAG OPERAND: what", usage(), status 2
static void parse_floats(int argc, char** argv, int& i, int n, float* dst, bool (*ok)(float), const char* what)
{
    const char* flag = argv[i];
    need(argc, i, n);
    for (int c = 0; c < n; c++)
    {
        char* end = nullptr;
        dst[c] = strtof(argv[++i], &end);
        if (end == argv[i] || *end || !ok(dst[c])) refuse(USAGE, "%s %s: %s", flag, argv[i], what);
    }
}

// ---- what the flags say, with the defaults
struct Options
{
    int         julia = 128, W = 400, H = 300, spp = 16, preset = 12, brick = 1, batch = 0;
    float       density = 800.0f, g = 0.877f, sunx = 0.5f, suny = 0.2f;
    int         philox = 0;   // 0 sampler.h, 1 Philox2x32-10, 2 Philox2x32-7
    int         est = VP_EST_DECOMP, tracking = VP_TRACK_SPECTRAL, env_mode = VP_ENV_PASSIVE, arith = VP_ARITH_EXACT;
    std::string bin, vdb, out = "output0.ppm", devlist;
    int         vol_format = VP_VOL_U8;
    int         gpus = 1, aa = 0;   // (0: not given -- the contexts keep their default, VP_SUBPIXEL)
    bool        adaptive = false;
    float       noise_tol = 0.0f;
    int         min_spp = 16, round_frames = 32;   // (the round: not measured yet)
    std::string noise_out;
    bool        denoise = false;
    vp_denoise_params dn = {5, 1, 0.45f};   // (from a 64 x 48 table, not tuned: DESIGN.md section 2.4)
    bool        denoise_features = false;
    bool        denoise_cross = false;   // --denoise-cross: two half-buffers, each filtered with the other's weights, merged
    std::string resid_out;
    bool        denoise_var = false;     // --denoise-var: --denoise-cross with the pooled, pre-filtered variance plane
    vp_denoise_params dnv = {1, 3, 0.45f};   // (the paper's window; wider ones lost at (10, 3): DESIGN.md section 2.17)
    std::string var_out;
    bool        denoise_select = false;  // --denoise-select: --denoise-var at two windows, the better one picked per pixel
    vp_denoise_params dns = {10, 3, 0.45f};   // candidate 1's window (its k is dn's: --denoise-k is shared)
    vp_select_params  sel = {1, 1};
    std::string select_out;
    float       dn_sigma_alpha = 0.2f, dn_sigma_depth = 0.2f;   // (the best cell of a 3 x 3 grid on that scene: DESIGN.md section 2.13)
    std::string layers_out;
    bool        over = false;
    float       over_rgb[3] = {0.0f, 0.0f, 0.0f};
    std::string groups_out;
    bool        relit = false;
    float       sun_gain[3] = {1.0f, 1.0f, 1.0f}, sky_gain[3] = {1.0f, 1.0f, 1.0f};
    bool        groups_denoise = false, layers_denoise = false;
    bool        plane_adaptive = false;
    float       plane_tol[2] = {0.0f, 0.0f};
    std::string plane_noise_out;
    std::string planes_out;
    bool        planes_denoise = false;
    bool        planes_adaptive = false;
    float       planes_tol[3] = {0.0f, 0.0f, 0.0f};
    std::string planes_noise_out;
    bool        layers_cross = false, groups_cross = false, planes_cross = false;   // --*-denoise-cross: the mode's filter flag, on two halves of every plane
    bool        plane_denoise_var = false;   // --plane-denoise-var: the variance stage in front of each plane's pair of filters
    std::string plane_resid_out;
    bool        cross_adaptive = false, plane_cross_adaptive = false, planes_cross_adaptive = false;   // --cross-noise, --plane-cross-noise, --planes-cross-noise: rounds on halves
    float       cross_tol = 0.0f, plane_cross_tol[2] = {0.0f, 0.0f}, planes_cross_tol[3] = {0.0f, 0.0f, 0.0f};
    std::string cross_noise_out, plane_cross_noise_out;
    std::string features_out;
    vp_feature_params feat = {0.001f, VP_FEATURE_TAU_Z_DEFAULT};

    void parse(int argc, char** argv);
};
static_assert((int)VOLUME_U8 == (int)VP_VOL_U8 && (int)VOLUME_F32 == (int)VP_VOL_F32 && (int)VOLUME_F16 == (int)VP_VOL_F16, "the loaders' formats are vp_init_volume's");

void Options::parse(int argc, char** argv)
{
    const auto at_least_0 = [](float v) { return v >= 0.0f; };
    const auto above_0    = [](float v) { return std::isfinite(v) && v > 0.0f; };
    const auto finite     = [](float v) { return (bool)std::isfinite(v); };
    for (int i = 1; i < argc; i++)
    {
        std::string a = argv[i];
        auto need = [&](int n) { ::need(argc, i, n); };
        if (a == "--julia") { need(1); julia = atoi(argv[++i]); }
        else if (a == "--bin") { need(1); bin = argv[++i]; }
        else if (a == "--vdb") { need(1); vdb = argv[++i]; }
        else if (a == "--volume-format")
        {
            need(1);
            const char* f = argv[++i];
            if (!strcmp(f, "u8")) vol_format = VP_VOL_U8;
            else if (!strcmp(f, "f32")) vol_format = VP_VOL_F32;
            else if (!strcmp(f, "f16")) vol_format = VP_VOL_F16;
            else refuse(USAGE, "unknown --volume-format %s (u8, f32 or f16)", f);
        }
        else if (a == "--size") { need(2); W = atoi(argv[++i]); H = atoi(argv[++i]); }
        else if (a == "--spp") { need(1); spp = atoi(argv[++i]); }
        else if (a == "--preset") { need(1); preset = atoi(argv[++i]); }
        else if (a == "--density") { need(1); density = (float)atof(argv[++i]); }
        else if (a == "--g") { need(1); g = (float)atof(argv[++i]); }
        else if (a == "--estimator")
        {
            need(1);
            const char* e = argv[++i];
            est = !strcmp(e, "global") ? VP_EST_GLOBAL : !strcmp(e, "bounded") ? VP_EST_BOUNDED : VP_EST_DECOMP;
        }
        else if (a == "--brick") { need(1); brick = atoi(argv[++i]); }
        else if (a == "--rng") { need(1); ++i; philox = !strcmp(argv[i], "philox") ? 1 : !strcmp(argv[i], "philox7") ? 2 : 0; }
        else if (a == "--tracking")
        {
            need(1);
            const char* t = argv[++i];
            tracking = !strcmp(t, "scalar") ? VP_TRACK_SCALAR : !strcmp(t, "multichannel") ? VP_TRACK_MULTI_CHANNEL : VP_TRACK_SPECTRAL;
        }
        else if (a == "--env") { need(1); env_mode = !strcmp(argv[++i], "mis") ? VP_ENV_MIS : VP_ENV_PASSIVE; }
        else if (a == "--arith")
        {
            need(1);
            const char* m = argv[++i];
            if (!strcmp(m, "exact")) arith = VP_ARITH_EXACT;
            else if (!strcmp(m, "fast")) arith = VP_ARITH_FAST;
            else refuse(USAGE, "unknown --arith %s", m);
        }
        else if (a == "--aa")
        {
            need(1);
            const char* m = argv[++i];
            aa = !strcmp(m, "1") ? 1 : !strcmp(m, "2") ? 2 : !strcmp(m, "4") ? 4 : !strcmp(m, "8") ? 8 : 0;
            if (!aa) refuse(USAGE, "unknown --aa %s (1, 2, 4 or 8)", m);
        }
        else if (a == "--noise") { parse_floats(argc, argv, i, 1, &noise_tol, at_least_0, "a tolerance >= 0"); adaptive = true; }
        else if (a == "--plane-noise") { parse_floats(argc, argv, i, 2, plane_tol, at_least_0, "two tolerances >= 0"); plane_adaptive = true; }
        else if (a == "--plane-noise-out") { need(1); plane_noise_out = argv[++i]; }
        else if (a == "--planes-noise") { parse_floats(argc, argv, i, 3, planes_tol, at_least_0, "three tolerances >= 0"); planes_adaptive = true; }
        else if (a == "--planes-noise-out") { need(1); planes_noise_out = argv[++i]; }
        else if (a == "--cross-noise") { parse_floats(argc, argv, i, 1, &cross_tol, at_least_0, "a tolerance >= 0"); cross_adaptive = denoise_cross = denoise = true; }
        else if (a == "--cross-noise-out") { need(1); cross_noise_out = argv[++i]; }
        else if (a == "--plane-cross-noise") { parse_floats(argc, argv, i, 2, plane_cross_tol, at_least_0, "two tolerances >= 0"); plane_cross_adaptive = true; }
        else if (a == "--planes-cross-noise") { parse_floats(argc, argv, i, 3, planes_cross_tol, at_least_0, "three tolerances >= 0"); planes_cross_adaptive = true; }
        else if (a == "--plane-cross-noise-out") { need(1); plane_cross_noise_out = argv[++i]; }
        else if (a == "--min-spp") { need(1); min_spp = atoi(argv[++i]); }
        else if (a == "--round") { need(1); round_frames = atoi(argv[++i]); }
        else if (a == "--noise-out") { need(1); noise_out = argv[++i]; }
        else if (a == "--denoise") denoise = true;
        else if (a == "--denoise-cross") denoise_cross = denoise = true;
        else if (a == "--resid-out") { need(1); resid_out = argv[++i]; }
        else if (a == "--denoise-var") denoise_var = denoise_cross = denoise = true;
        else if (a == "--var-out") { need(1); var_out = argv[++i]; }
        else if (a == "--denoise-select") denoise_select = denoise_var = denoise_cross = denoise = true;
        else if (a == "--select-out") { need(1); select_out = argv[++i]; }
        else if (a == "--denoise-select-smooth" || a == "--denoise-select-blend")
        {
            need(1);
            char* end = nullptr;
            const char* v = argv[++i];
            const long n = strtol(v, &end, 10);
            if (end == v || *end || n < 0 || n > VP_SELECT_MAX_RADIUS) refuse(USAGE, "%s %s: a radius 0..%d", a.c_str(), v, VP_SELECT_MAX_RADIUS);
            (a == "--denoise-select-smooth" ? sel.smooth_radius : sel.blend_radius) = (int)n;
        }
        else if (a == "--denoise-radius" || a == "--denoise-patch" || a == "--denoise-k" || a == "--denoise-var-radius" || a == "--denoise-var-patch" ||
                 a == "--denoise-var-k" || a == "--denoise-select-radius" || a == "--denoise-select-patch")
        {
            need(1);
            char* end = nullptr;
            const char* v = argv[++i];
            // the variance pass's window, the second candidate's or the colour pass's
            vp_denoise_params& d = a.compare(0, 13, "--denoise-var") == 0 ? dnv : a.compare(0, 16, "--denoise-select") == 0 ? dns : dn;
            const char what = a[a.rfind('-') + 1];                                     // r, p or k
            bool ok;
            if (what == 'k') { d.k = strtof(v, &end); ok = end != v && !*end && std::isfinite(d.k) && d.k > 0.0f; }
            else
            {
                const long n = strtol(v, &end, 10);
                ok = end != v && !*end && n >= 0 && n <= (what == 'r' ? VP_DENOISE_MAX_RADIUS : VP_DENOISE_MAX_PATCH);
                (what == 'r' ? d.radius : d.patch) = (int)n;
            }
            if (!ok) refuse(USAGE, "%s %s: radius 0..%d, patch 0..%d, k a finite number > 0", a.c_str(), v, VP_DENOISE_MAX_RADIUS, VP_DENOISE_MAX_PATCH);
        }
        else if (a == "--denoise-features") denoise_features = true;
        else if (a == "--denoise-sigma-alpha") parse_floats(argc, argv, i, 1, &dn_sigma_alpha, above_0, "a finite number > 0");
        else if (a == "--denoise-sigma-depth") parse_floats(argc, argv, i, 1, &dn_sigma_depth, above_0, "a finite number > 0");
        else if (a == "--layers-out") { need(1); layers_out = argv[++i]; }
        else if (a == "--over") { parse_floats(argc, argv, i, 3, over_rgb, finite, "three finite numbers"); over = true; }
        else if (a == "--groups-out") { need(1); groups_out = argv[++i]; }
        else if (a == "--sun-gain" || a == "--sky-gain") { parse_floats(argc, argv, i, 3, a == "--sun-gain" ? sun_gain : sky_gain, finite, "three finite numbers"); relit = true; }
        else if (a == "--features-out") { need(1); features_out = argv[++i]; }
        else if (a == "--feature-step") parse_floats(argc, argv, i, 1, &feat.step, above_0, "a finite number > 0");
        else if (a == "--depth-tau") parse_floats(argc, argv, i, 1, &feat.tau_z, above_0, "a finite number > 0");
        else if (a == "--planes-out") { need(1); planes_out = argv[++i]; }
        else if (a == "--planes-denoise") planes_denoise = true;
        else if (a == "--groups-denoise") groups_denoise = true;
        else if (a == "--layers-denoise") layers_denoise = true;
        else if (a == "--planes-denoise-cross") planes_cross = planes_denoise = true;
        else if (a == "--groups-denoise-cross") groups_cross = groups_denoise = true;
        else if (a == "--layers-denoise-cross") layers_cross = layers_denoise = true;
        else if (a == "--plane-denoise-var") plane_denoise_var = true;
        else if (a == "--plane-resid-out") { need(1); plane_resid_out = argv[++i]; }
        else if (a == "--sun") { need(2); sunx = (float)atof(argv[++i]); suny = (float)atof(argv[++i]); }
        else if (a == "--batch") { need(1); batch = atoi(argv[++i]); }
        else if (a == "--out") { need(1); out = argv[++i]; }
        else if (a == "--gpus") { need(1); gpus = atoi(argv[++i]); }
        else if (a == "--devices") { need(1); devlist = argv[++i]; }
        else if (a == "--rccl-selftest")
        {
            // the RCCL calls of the multi-GPU path on one device (multigpu.h)
            const int   dev = i + 1 < argc ? atoi(argv[i + 1]) : 0;
            std::string report;
            const bool  ok = volpath::rccl_selftest(dev, (size_t)1280 * 720 * 4, report);
            printf("%s\n", report.c_str());
            exit(ok ? 0 : 1);
        }
        else { usage(); exit(a == "--help" ? 0 : 2); }
    }
}

// ---- what the run is
// One image plane of the render: the suffix of its files, the floor of its adaptive criterion and noise map, and its device buffers
// (the sum of its samples; a record per pixel where the job keeps records; its mean image where the job forms one).
struct Plane
{
    const char*     suffix;
    float           floor;
    vp_float4*      acc;
    vp_pixel_stats* rec;
    vp_float4*      mean;
};
static const float kFloor = 1e-3f, kFloorTrans = 1e-2f;   // (the transmittance lives in [0, 1])
static const Plane kBeauty = {"", kFloor}, kSun = {"_sun.hdr", kFloor}, kSky = {"_sky.hdr", kFloor}, kFg = {"_fg.hdr", kFloor}, kTrans = {"_trans.hdr", kFloorTrans};

enum Mode { BEAUTY, LAYERS, GROUPS, PLANES };
struct Job
{
    Options          o;
    Param            P;
    std::vector<int> devices;
    int              batch = 0;
    bool             hdr = false;        // --out is the scaled accumulator, not its gamma-corrected bytes
    Mode             mode = BEAUTY;
    bool             cross = false;      // planes in two halves (--*-denoise-cross): plane[k] is half 0's, other[k] half 1's, the mean the cross-filter's
    Plane            other[3] = {};
    int              n = 1;              // planes: beauty 1 (--denoise-cross 2: its half-buffers), layers fg trans, groups sun sky, planes sun sky trans
    Plane            plane[3] = {};
    bool             filter = false;     // the mean of a plane is vp_denoise's (beauty: --denoise and its variants)
    bool             adaptive = false;   // rounds to the tolerances tol[k], then no batch loop
    bool             halves_adaptive = false;   // ... into two halves (--cross-noise, --plane-cross-noise, --planes-cross-noise): each plane's two records pooled
    int              ntol = 1;           // the planes the criterion is asked of (n, but 1 for the beauty image's two half-buffers)
    bool             records = false;    // the frames go through the mode's _stats call / its adaptive call
    bool             means = false;      // a mean buffer per plane
    float            tol[3] = {};
    const char*      noise_flag = "";    // the adaptive flag, for the report
    std::string      prefix, noise_prefix;   // plane files and noise maps: PREFIX + suffix (beauty: --noise-out's one name)
};

struct Conflict { bool given; const char* flag; };
// the first flag of the list that was given, or nullptr
static const char* first_of(std::initializer_list<Conflict> list)
{
    for (const Conflict& c : list) if (c.given) return c.flag;
    return nullptr;
}

// the refusals of flags that do not go together, in their order; what passes them is one of the four modes
static Mode refuse_conflicts(const Options& o)
{
    if (o.vol_format != VP_VOL_U8 && o.bin.empty() && o.vdb.empty())
        refuse(PLAIN, "--volume-format %s needs --bin or --vdb: --julia voxelises to bytes (u8)", o.vol_format == VP_VOL_F16 ? "f16" : "f32");
    if (o.gpus < 1) { usage(); exit(2); }
    // what every mode with per-pixel records refuses: they are not reduced across ranks, and the beauty image's rounds and filter are its own
    const auto  beauty_flag = [&] { return first_of({{o.gpus > 1, "--gpus"}, {o.adaptive, "--noise"}, {o.denoise, "--denoise"}}); };
    const bool  plain_lights = o.tracking == VP_TRACK_SPECTRAL && o.env_mode == VP_ENV_PASSIVE && o.arith == VP_ARITH_EXACT;
    const bool  bad_rounds = o.min_spp < 2 || o.round_frames < 1;
    const char* other;
    if (o.adaptive && o.gpus > 1)
        refuse(PLAIN, "--noise with --gpus %d: reducing per-pixel statistics across ranks is not part of adaptive sampling; use one GPU", o.gpus);
    if (!o.denoise_cross && !o.resid_out.empty()) refuse(PLAIN, "--resid-out needs --denoise-cross: the map is the disagreement of the two filtered halves");
    if (!o.denoise_var && !o.var_out.empty()) refuse(PLAIN, "--var-out needs --denoise-var: the map is the filtered variance plane of that stage");
    if (!o.denoise_select && !o.select_out.empty()) refuse(PLAIN, "--select-out needs --denoise-select: the map is the index of the candidate picked per pixel");
    if (o.denoise_select && !o.resid_out.empty()) refuse(PLAIN, "--denoise-select with --resid-out: a residual map of a blend of candidates is not defined here");
    // adaptive rounds on halves: one GPU, no other adaptive flag, and each flag with the cross-filter of its own mode
    const char* cross_noise = first_of({{o.cross_adaptive, "--cross-noise"}, {o.plane_cross_adaptive, "--plane-cross-noise"}, {o.planes_cross_adaptive, "--planes-cross-noise"}});
    if (cross_noise && (other = first_of({{o.gpus > 1, "--gpus"}, {o.adaptive, "--noise"}, {o.plane_adaptive, "--plane-noise"}, {o.planes_adaptive, "--planes-noise"}})))
        refuse(PLAIN, "%s with %s: the halves' records are not reduced across ranks, and rounds on halves are the run's only adaptive rounds (they judge the "
               "two records of a plane together); use one GPU without --noise, --plane-noise and --planes-noise", cross_noise, other);
    if (o.cross_adaptive && (other = first_of({{o.plane_cross_adaptive, "--plane-cross-noise"}, {o.planes_cross_adaptive, "--planes-cross-noise"}})))
        refuse(PLAIN, "--cross-noise with %s: --cross-noise samples the beauty image's half-buffers, %s the halves of planes", other, other);
    if (o.plane_cross_adaptive && (o.planes_cross_adaptive || o.planes_cross || !(o.layers_cross || o.groups_cross)))
        refuse(PLAIN, "--plane-cross-noise needs --layers-denoise-cross or --groups-denoise-cross: it samples the halves of that render's two planes "
               "(three planes: --planes-cross-noise TOL_SUN TOL_SKY TOL_TRANS with --planes-denoise-cross)");
    if (o.planes_cross_adaptive && !o.planes_cross)
        refuse(PLAIN, "--planes-cross-noise needs --planes-denoise-cross: it samples the halves of that render's three planes "
               "(two planes: --plane-cross-noise TOL0 TOL1 with --layers-denoise-cross or --groups-denoise-cross)");
    if (cross_noise && bad_rounds) refuse(USAGE, "%s needs --min-spp >= 2 and --round >= 1", cross_noise);
    if (!o.cross_adaptive && !o.cross_noise_out.empty()) refuse(PLAIN, "--cross-noise-out needs --cross-noise");
    if (!o.plane_cross_adaptive && !o.planes_cross_adaptive && !o.plane_cross_noise_out.empty())
        refuse(PLAIN, "--plane-cross-noise-out needs --plane-cross-noise or --planes-cross-noise");
    // the cross-filter on planes: one GPU, no adaptive rounds of any kind, and not beside the beauty image's cross-filter
    const char* plane_cross = first_of({{o.layers_cross, "--layers-denoise-cross"}, {o.groups_cross, "--groups-denoise-cross"}, {o.planes_cross, "--planes-denoise-cross"}});
    if (o.cross_adaptive && plane_cross)
        refuse(PLAIN, "--cross-noise with %s: --cross-noise samples the beauty image's half-buffers; the halves of planes take --plane-cross-noise TOL0 TOL1 "
               "(layers, groups) or --planes-cross-noise TOL_SUN TOL_SKY TOL_TRANS", plane_cross);
    if (!plane_cross && o.plane_denoise_var)
        refuse(PLAIN, "--plane-denoise-var needs --layers-denoise-cross, --groups-denoise-cross or --planes-denoise-cross: it is the variance stage of that filter");
    if (!plane_cross && !o.plane_resid_out.empty())
        refuse(PLAIN, "--plane-resid-out needs --layers-denoise-cross, --groups-denoise-cross or --planes-denoise-cross: the maps are the disagreement of each plane's two filtered halves");
    if (plane_cross && (other = first_of({{o.gpus > 1, "--gpus"}, {o.adaptive, "--noise"}, {o.plane_adaptive, "--plane-noise"}, {o.planes_adaptive, "--planes-noise"},
                                          {o.denoise_select, "--denoise-select"}, {o.denoise_var, "--denoise-var"}, {o.denoise_cross, "--denoise-cross"}})))
        refuse(PLAIN, "%s with %s: the halves' records are not reduced across ranks, adaptive rounds on halves are not built and the beauty image's halves are "
               "its own; use one GPU without --noise, --plane-noise, --planes-noise and --denoise-cross / -var / -select", plane_cross, other);
    if (o.denoise_cross && (other = first_of({{o.gpus > 1, "--gpus"}, {o.adaptive, "--noise"}, {!o.planes_out.empty(), "--planes-out"}, {!o.groups_out.empty(), "--groups-out"},
                                              {o.relit, "--sun-gain / --sky-gain"}, {!o.layers_out.empty(), "--layers-out"}, {o.over, "--over"}, {o.plane_adaptive, "--plane-noise"},
                                              {o.planes_adaptive, "--planes-noise"}, {o.groups_denoise, "--groups-denoise"}, {o.layers_denoise, "--layers-denoise"},
                                              {o.planes_denoise, "--planes-denoise"}})))
        refuse(PLAIN, "--denoise-cross with %s: the half-buffers' records are not reduced across ranks, adaptive rounds on halves are not built and the halves are "
               "the beauty image's, not a plane's; use one GPU without --noise and without plane outputs or plane filters", other);
    if (o.denoise && o.gpus > 1)
        refuse(PLAIN, "--denoise with --gpus %d: the filter reads per-pixel statistics, which are not reduced across ranks; use one GPU", o.gpus);
    if (o.denoise_features && !o.denoise) refuse(PLAIN, "--denoise-features needs --denoise: it cuts the weights of that filter (the per-plane filters do not take it)");
    if (o.denoise_features && o.aa > 1)
        refuse(PLAIN, "--denoise-features with --aa %d: the feature pass marches pixel-centre rays and refuses a sub-pixel factor; use --aa 1", o.aa);
    // --planes-out: sun, sky and trans from one render; the gains and --over are then its parameters, not a groups or a layers render's
    const bool planes = !o.planes_out.empty();
    if (o.planes_denoise && !planes) refuse(PLAIN, "--planes-denoise needs --planes-out: it filters the three planes of that render");
    if (planes && (other = first_of({{o.gpus > 1, "--gpus"}, {o.adaptive, "--noise"}, {o.denoise, "--denoise"}, {!o.groups_out.empty(), "--groups-out"},
                                     {!o.layers_out.empty(), "--layers-out"}, {o.plane_adaptive, "--plane-noise"}, {o.groups_denoise, "--groups-denoise"},
                                     {o.layers_denoise, "--layers-denoise"}})))
        refuse(PLAIN, "--planes-out with %s: the three planes are not reduced across ranks, are filtered by --planes-denoise only, are sampled adaptively by "
               "--planes-noise only and replace the groups and the layers render; use one GPU without --noise, --denoise, --groups-out, --layers-out and "
               "--plane-noise (three tolerances: --planes-noise TOL_SUN TOL_SKY TOL_TRANS)", other);
    if (planes && !plain_lights) refuse(PLAIN, "--planes-out needs spectral tracking, --env passive and --arith exact");
    // adaptive rounds on the three planes: --planes-out, one GPU, and neither the beauty image's rounds nor its filter (refused above)
    if (o.planes_adaptive && !planes) refuse(PLAIN, "--planes-noise needs --planes-out: it samples the three planes of that render");
    if (o.planes_adaptive && bad_rounds) refuse(USAGE, "--planes-noise needs --min-spp >= 2 and --round >= 1");
    if (!o.planes_adaptive && !o.planes_noise_out.empty()) refuse(PLAIN, "--planes-noise-out needs --planes-noise");
    const bool layers = !planes && (o.over || !o.layers_out.empty());
    const bool groups = !planes && (o.relit || !o.groups_out.empty());
    // the per-plane filters: each needs its plane flag, one GPU, and neither the beauty image's filter nor adaptive rounds
    for (int k = 0; k < 2; k++)
    {
        const char* flag = k ? "--layers-denoise" : "--groups-denoise";
        if (!(k ? o.layers_denoise : o.groups_denoise)) continue;
        if (!(k ? layers : groups))
            refuse(PLAIN, "%s needs %s: it filters the planes of a %s render", flag, k ? "--layers-out or --over" : "--groups-out, --sun-gain or --sky-gain", k ? "layers" : "light-groups");
        if ((other = beauty_flag()))
            refuse(PLAIN, "%s with %s: per-plane records are not reduced across ranks, adaptive rounds on planes are --plane-noise's, and --denoise filters the beauty image; "
                   "use one GPU without --noise and --denoise", flag, other);
    }
    // adaptive rounds on planes: a plane flag, one GPU, and neither the beauty image's rounds nor its filter
    if (o.plane_adaptive && !layers && !groups)
        refuse(PLAIN, "--plane-noise needs --groups-out, --sun-gain or --sky-gain, or --layers-out or --over: it samples the planes of a light-groups or layers render");
    if (o.plane_adaptive && (other = beauty_flag()))
        refuse(PLAIN, "--plane-noise with %s: per-plane records are not reduced across ranks, --noise samples the beauty image and --denoise filters it; "
               "use one GPU without --noise and --denoise", other);
    if (o.plane_adaptive && bad_rounds) refuse(USAGE, "--plane-noise needs --min-spp >= 2 and --round >= 1");
    if (!o.plane_adaptive && !o.plane_noise_out.empty()) refuse(PLAIN, "--plane-noise-out needs --plane-noise");
    if (layers && (other = beauty_flag()))
        refuse(PLAIN, "--layers-out / --over with %s: layers are not reduced across ranks and carry no per-pixel statistics; use one GPU without --noise and --denoise", other);
    if (layers && !plain_lights) refuse(PLAIN, "--layers-out / --over need spectral tracking, --env passive and --arith exact");
    if (groups && ((other = beauty_flag()) || (other = first_of({{o.over, "--over"}, {layers, "--layers-out"}}))))
        refuse(PLAIN, "--groups-out / --sun-gain / --sky-gain with %s: light groups are not reduced across ranks, carry no per-pixel statistics and are not combined with layers; "
               "use one GPU without --noise, --denoise, --layers-out and --over", other);
    if (groups && !plain_lights) refuse(PLAIN, "--groups-out / --sun-gain / --sky-gain need spectral tracking, --env passive and --arith exact");
    if (o.adaptive && bad_rounds) refuse(USAGE, "--noise needs --min-spp >= 2 and --round >= 1");
    if (!o.adaptive && !o.noise_out.empty()) refuse(PLAIN, "--noise-out needs --noise");
    if (o.arith == VP_ARITH_FAST && (o.philox == 0 || o.est == VP_EST_BOUNDED || o.tracking != VP_TRACK_SPECTRAL || o.env_mode != VP_ENV_PASSIVE))
        refuse(PLAIN, "--arith fast needs --rng philox|philox7, --estimator decomp|global, spectral tracking and --env passive");
    return planes ? PLANES : layers ? LAYERS : groups ? GROUPS : BEAUTY;
}

// the one place that decides what the run is
static Job validate(const Options& o)
{
    Job j;
    j.o = o;
    j.P = default_param(o.W, o.H);  // host.cpp:1286-1292
    j.P.density = o.density;
    j.P.g       = o.g;
    if (!material_preset(j.P, o.preset)) refuse(PLAIN, "preset must be 0..12");
    j.mode = refuse_conflicts(o);
    for (size_t pos = 0; pos < o.devlist.size();)
    {
        size_t e = o.devlist.find(',', pos);
        if (e == std::string::npos) e = o.devlist.size();
        j.devices.push_back(atoi(o.devlist.substr(pos, e - pos).c_str()));
        pos = e + 1;
    }
    if (j.devices.empty()) for (int r = 0; r < o.gpus; r++) j.devices.push_back(r);
    if ((int)j.devices.size() != o.gpus) refuse(PLAIN, "--devices must list %d devices", o.gpus);
    j.batch = o.gpus > 1 && o.batch <= 0 ? std::min(o.spp, 256) : o.batch;  // shards render in batches: one launch per rank keeps every GPU busy
    j.hdr   = o.out.size() > 4 && o.out.substr(o.out.size() - 4) == ".hdr";

    // ---- the plane table of the mode, with its one filter flag and its one adaptive flag
    const bool   layers = j.mode == LAYERS;
    const float* tol = &o.noise_tol;
    switch (j.mode)
    {
    case BEAUTY:
        j.plane[0] = kBeauty, j.plane[1] = kBeauty, j.n = o.denoise_cross ? 2 : 1;
        j.filter = o.denoise, j.adaptive = o.adaptive, j.noise_flag = "--noise", j.noise_prefix = o.noise_out;
        if (o.cross_adaptive) j.halves_adaptive = true, j.noise_flag = "--cross-noise", j.noise_prefix = o.cross_noise_out, tol = &o.cross_tol;
        break;
    case LAYERS:
    case GROUPS:
        j.plane[0] = layers ? kFg : kSun, j.plane[1] = layers ? kTrans : kSky, j.n = 2;
        j.filter = layers ? o.layers_denoise : o.groups_denoise, j.prefix = layers ? o.layers_out : o.groups_out;
        j.adaptive = o.plane_adaptive, j.noise_flag = "--plane-noise", j.noise_prefix = o.plane_noise_out, tol = o.plane_tol;
        j.cross = layers ? o.layers_cross : o.groups_cross;
        if (o.plane_cross_adaptive) j.halves_adaptive = true, j.noise_flag = "--plane-cross-noise", j.noise_prefix = o.plane_cross_noise_out, tol = o.plane_cross_tol;
        j.ntol = 2;
        break;
    case PLANES:
        j.plane[0] = kSun, j.plane[1] = kSky, j.plane[2] = kTrans, j.n = 3;
        j.filter = o.planes_denoise, j.prefix = o.planes_out;
        j.adaptive = o.planes_adaptive, j.noise_flag = "--planes-noise", j.noise_prefix = o.planes_noise_out, tol = o.planes_tol;
        j.cross = o.planes_cross;
        if (o.planes_cross_adaptive) j.halves_adaptive = true, j.noise_flag = "--planes-cross-noise", j.noise_prefix = o.plane_cross_noise_out, tol = o.planes_cross_tol;
        j.ntol = 3;
        break;
    }
    // (a cross flag of another mode than the run's: that mode's refusals took it above, as they take its -denoise flag)
    for (int k = 0; k < j.n && j.cross; k++) j.other[k] = j.plane[k];
    // (a --plane-cross-noise / --planes-cross-noise of a run without its cross flag was refused above)
    j.halves_adaptive = j.halves_adaptive && (j.mode == BEAUTY || j.cross);
    j.adaptive = j.adaptive || j.halves_adaptive;
    for (int k = 0; k < j.ntol && j.adaptive; k++) j.tol[k] = tol[k];
    j.records = j.filter || j.adaptive;
    j.means   = j.mode == BEAUTY ? o.denoise_cross : j.records;   // (the beauty image's mean is formed in the display buffer)
    return j;
}

// ---- the devices of the run: one context per rank (a single rank runs in the default context, as the reference's host would)
struct Run
{
    int                     gpus = 1, npix = 0;
    std::vector<vp_ctx*>    ctx;
    std::vector<vp_float4*> accum;     // full frame on every rank: zero outside its tiles
    std::vector<void*>      streams;
    volpath::SunSky         sky;
    volpath::NodeReducer    reducer;
    vp_float4*              disp = nullptr;
    vp_adaptive_result      ares = {};
    int                     round_frames = 0;   // the round of an adaptive run (--round; rounded up for rounds on halves under a sub-pixel factor)

    void use(int r) const { if (gpus > 1) vp_ctx_set_current(ctx[r]); }
};

template <class T> static T* device_alloc(int n, bool zeroed)
{
    T* p = (T*)vp_malloc((size_t)n * sizeof(T));
    must(!p || (zeroed && vp_memset(p, 0, (size_t)n * sizeof(T))));
    return p;
}

// contexts, the volume and the scene on every rank, the accumulators, the reducer, the display buffer
static void set_up(const Job& j, Run& run)
{
    const Options& o = j.o;
    run.gpus = o.gpus;
    run.npix = o.W * o.H;
    run.ctx.assign(o.gpus, nullptr);
    run.accum.assign(o.gpus, nullptr);
    run.streams.assign(o.gpus, nullptr);
    if (o.gpus > 1)
        for (int r = 0; r < o.gpus; r++) must(!(run.ctx[r] = vp_ctx_create(j.devices[r])));
    else must(vp_set_device(j.devices[0]));

    // ---- volume (host.cpp:1330-1344): loaded once, uploaded to every rank (all read-only scene data is replicated)
    int   width = 0, height = 0, depth = 0;
    void* h_volume = nullptr;
    if (!o.bin.empty()) h_volume = loadBinaryFileAs(o.bin.c_str(), width, height, depth, o.vol_format);
    else if (!o.vdb.empty()) h_volume = loadVdbFileAs(o.vdb.c_str(), width, height, depth, o.vol_format);
    else
    {
        width = height = depth = o.julia;
        h_volume = malloc((size_t)o.julia * o.julia * o.julia);
        run.use(0);
        must(!h_volume || vp_julia_voxelize(o.julia, (unsigned char*)h_volume));
    }
    if (!h_volume) exit(1);
    vp_float3 box_min = {-1.0f, -(float)height / (float)width, -(float)depth / (float)width};
    vp_float3 box_max = {1.0f, (float)height / (float)width, (float)depth / (float)width};
    float identity[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    Camera cam;
    float  m[12];
    cam.inv_view_matrix(m);
    // sun / sky (host.cpp:1388-1390 -> update_sunsky)
    run.sky = volpath::bake_sunsky(o.sunx, o.suny);
    volpath::SunSky& sky = run.sky;
    printf("sun power = %f, %f, %f\n", sky.sun_power.x, sky.sun_power.y, sky.sun_power.z);

    for (int r = 0; r < o.gpus; r++)
    {
        run.use(r);
        vp_set_bound_brick(o.brick);
        if (o.vol_format == VP_VOL_U8) init_cuda(h_volume, vp_extent{(size_t)width, (size_t)height, (size_t)depth}, true, &box_min, &box_max);
        else must(vp_init_volume(h_volume, vp_extent{(size_t)width, (size_t)height, (size_t)depth}, o.vol_format, &box_min, &box_max));
        set_texture_filter_mode(true);
        copy_inv_model_matrix(identity, sizeof(identity));  // host.cpp:1350-1353
        copy_inv_view_matrix(m, sizeof(m));                 // host.cpp:617-623
        init_envmap(reinterpret_cast<const vp_float4*>(sky.envmap.data()), sky.width, sky.height);
        set_sun(&sky.sun_dir.x, &sky.sun_power.x);
        vp_set_estimator(o.est);
        must(vp_set_tracking(o.tracking) || vp_set_envmap_sampling(o.env_mode) || vp_set_shard(r, o.gpus));
        vp_set_rng(o.philox == 2 ? VP_RNG_PHILOX7 : o.philox ? VP_RNG_PHILOX : VP_RNG_SAMPLERH, 0x9E3779B9u, 0x85EBCA6Bu);
        must(vp_set_arithmetic(o.arith));
        must(o.aa && vp_set_subpixel(o.aa));
        // frame buffer (CudaFrameBuffer host.cpp:358-389)
        must(!(run.accum[r] = (vp_float4*)vp_malloc((size_t)run.npix * sizeof(vp_float4))));
        vp_memset(run.accum[r], 0, (size_t)run.npix * sizeof(vp_float4));
        run.streams[r] = vp_get_stream();
    }
    free(h_volume);
    std::string rerr;
    if (!run.reducer.init(j.devices, rerr)) { fprintf(stderr, "%s\n", rerr.c_str()); exit(1); }
    if (o.gpus > 1) printf("multi-GPU reducer: %s\n", run.reducer.describe().c_str());
    run.use(0);
    run.disp = device_alloc<vp_float4>(run.npix, false);
    for (int r = 0; r < o.gpus; r++) { run.use(r); vp_synchronize(); vp_render_time_ms(nullptr, nullptr, 1); }
}

// the plane table's buffers (more than one plane: one rank): accumulators zeroed (plane 0's is the rank's own), records zeroed where kept, means where formed
static void alloc_planes(Job& j, const Run& run)
{
    for (int k = 0; k < j.n; k++)
    {
        Plane& p = j.plane[k];
        p.acc = k ? device_alloc<vp_float4>(run.npix, true) : run.accum[0];
        if (j.records) p.rec = device_alloc<vp_pixel_stats>(run.npix, true);
        if (j.means) p.mean = device_alloc<vp_float4>(run.npix, false);
        if (!j.cross) continue;
        Plane& q = j.other[k];   // the second half of the plane: all three buffers its own
        q.acc = device_alloc<vp_float4>(run.npix, true);
        q.rec = device_alloc<vp_pixel_stats>(run.npix, true);
        q.mean = device_alloc<vp_float4>(run.npix, false);
    }
}
static void free_planes(Job& j)
{
    for (int k = 0; k < j.n; k++)
    {
        Plane& p = j.plane[k];
        if (p.rec) vp_free(p.rec);
        if (p.mean) vp_free(p.mean);
        if (k) vp_free(p.acc);
        const Plane& q = j.other[k];
        if (q.acc) { vp_free(q.acc); vp_free(q.rec); vp_free(q.mean); }
    }
}

// the two halves of a job with planes in halves as the planes-halves calls take them, and the mode
static int plane_halves(const Job& j, vp_plane_bufs h[2])
{
    for (int k = 0; k < j.n; k++) h[0].acc[k] = j.plane[k].acc, h[0].rec[k] = j.plane[k].rec, h[1].acc[k] = j.other[k].acc, h[1].rec[k] = j.other[k].rec;
    return j.mode == PLANES ? VP_PLANES_GROUP_LAYERS : j.mode == LAYERS ? VP_PLANES_LAYERS : VP_PLANES_GROUPS;
}
// frames s .. s + n - 1 by the mode's call on rank 0, with the records where the job keeps them (the same accumulator bits)
static int render_frames(const Job& j, int s, int n)
{
    const Plane* p = j.plane;
    const Param* P = &j.P;
    if (j.cross)   // the mode's _stats call, its frames split between the two halves of every plane
    {
        vp_plane_bufs h[2] = {};
        const int     mode = plane_halves(j, h);
        return vp_render_frames_planes_halves_stats(mode, &h[0], &h[1], s, n, P);
    }
    switch (j.mode)
    {
    case PLANES:
        return j.records ? vp_render_frames_group_layers_stats(p[0].acc, p[1].acc, p[2].acc, p[0].rec, p[1].rec, p[2].rec, s, n, P)
                         : vp_render_frames_group_layers(p[0].acc, p[1].acc, p[2].acc, s, n, P);
    case LAYERS: return j.records ? vp_render_frames_layers_stats(p[0].acc, p[1].acc, p[0].rec, p[1].rec, s, n, P) : vp_render_frames_layers(p[0].acc, p[1].acc, s, n, P);
    case GROUPS: return j.records ? vp_render_frames_groups_stats(p[0].acc, p[1].acc, p[0].rec, p[1].rec, s, n, P) : vp_render_frames_groups(p[0].acc, p[1].acc, s, n, P);
    default:     // --denoise: the filter needs the records; --denoise-cross: even and odd frames (blocks of frames) into the two halves
        return j.n == 2 ? vp_render_frames_halves_stats(p[0].acc, p[1].acc, p[0].rec, p[1].rec, s, n, P) : vp_render_frames_stats(p[0].acc, p[0].rec, s, n, P);
    }
}
// rounds on the pixels none of whose planes has met its tolerance, --spp frames at most
static int render_adaptive(const Job& j, int round_frames, vp_adaptive_result* res)
{
    const Options& o = j.o;
    const Plane*   p = j.plane;
    if (j.halves_adaptive && j.mode == BEAUTY)   // the two half-buffers: one criterion on their pooled records
    {
        const vp_adaptive ad = {j.tol[0], p[0].floor, o.min_spp, round_frames};
        return vp_render_adaptive_halves(p[0].acc, p[1].acc, p[0].rec, p[1].rec, 0, o.spp, &j.P, &ad, res);
    }
    if (j.halves_adaptive)   // two halves of every plane: each plane's criterion on its two records pooled
    {
        vp_plane_bufs h[2] = {};
        const int     mode = plane_halves(j, h);
        const vp_adaptive_planes3 ap = {{j.tol[0], j.tol[1], j.tol[2]}, {p[0].floor, p[1].floor, p[2].floor}, o.min_spp, round_frames};
        return vp_render_adaptive_planes_halves(mode, &h[0], &h[1], 0, o.spp, &j.P, &ap, res);
    }
    switch (j.mode)
    {
    case PLANES:
    {
        const vp_adaptive_planes3 ap = {{j.tol[0], j.tol[1], j.tol[2]}, {p[0].floor, p[1].floor, p[2].floor}, o.min_spp, o.round_frames};
        return vp_render_adaptive_group_layers(p[0].acc, p[1].acc, p[2].acc, p[0].rec, p[1].rec, p[2].rec, 0, o.spp, &j.P, &ap, res);
    }
    case LAYERS:
    case GROUPS:
    {
        const vp_adaptive_planes ap = {{j.tol[0], j.tol[1]}, {p[0].floor, p[1].floor}, o.min_spp, o.round_frames};
        return (j.mode == LAYERS ? vp_render_adaptive_layers : vp_render_adaptive_groups)(p[0].acc, p[1].acc, p[0].rec, p[1].rec, 0, o.spp, &j.P, &ap, res);
    }
    default:
    {
        const vp_adaptive ad = {j.tol[0], p[0].floor, o.min_spp, o.round_frames};
        return vp_render_adaptive(p[0].acc, p[0].rec, 0, o.spp, &j.P, &ad, res);
    }
    }
}

static void render(const Job& j, Run& run)
{
    const Options& o = j.o;
    const float*   sun_dir = &run.sky.sun_dir.x;
    if (j.adaptive)
    {
        if (o.est == VP_EST_DECOMP && o.spp > 11) precompute_opacity(sun_dir);   // host.cpp:336-343
        run.round_frames = o.round_frames;
        const int s2 = j.halves_adaptive ? 2 * vp_get_subpixel() * vp_get_subpixel() : 0;
        if (s2 > 2 && run.round_frames % s2)   // (a sub-pixel factor S: whole blocks of S^2 frames, as many for one half as for the other)
        {
            run.round_frames = (run.round_frames + s2 - 1) / s2 * s2;
            fprintf(stderr, "%s: --round %d rounded up to %d, a multiple of 2 S^2 = %d, so that every round feeds both halves equally\n", j.noise_flag,
                    o.round_frames, run.round_frames, s2);
        }
        must(render_adaptive(j, run.round_frames, &run.ares));
        return;
    }
    const bool    own_call = j.mode != BEAUTY || j.records;   // planes or records: the mode's frames call, one rank
    const vp_dim3 block = {8, 8, 1}, grid = {(unsigned)(o.W + 7) / 8, (unsigned)(o.H + 7) / 8, 1};
    bool          have_opacity = false;
    for (int s = 0; s < o.spp;)
    {
        if (!have_opacity && o.est == VP_EST_DECOMP && (s > 10 || (j.batch > 0 && s + j.batch > 11)))
        {
            for (int r = 0; r < o.gpus; r++) { run.use(r); precompute_opacity(sun_dir); }  // host.cpp:336-343
            have_opacity = true;
        }
        const int n = j.batch > 0 ? std::min(j.batch, o.spp - s) : 1;
        if (own_call) must(render_frames(j, s, n));
        else if (j.batch > 0)
            for (int r = 0; r < o.gpus; r++)  // asynchronous: every rank's launch is queued before any is waited for
            {
                run.use(r);
                must(vp_render_frames(run.accum[r], s, n, &j.P));
            }
        else
        {
            run.use(0);
            render_kernel(grid, block, run.accum[0], s, j.P);  // host.cpp:631
        }
        s += n;
    }
}

static void report(const Job& j, const Run& run, double sec)
{
    const Options& o = j.o;
    if (j.adaptive)
    {
        const vp_adaptive_result& ares = run.ares;
        const double all = (double)o.W * o.H * o.spp;
        char what[96];
        int  len = snprintf(what, sizeof what, "%s", j.noise_flag);
        for (int k = 0; k < j.ntol; k++) len += snprintf(what + len, sizeof what - len, " %g", j.tol[k]);
        printf("adaptive: %llu of %.0f samples (%.1f %%), %u rounds of %d frames, %u pixels still above %s after %u frames\n",
               (unsigned long long)ares.samples, all, 100.0 * (double)ares.samples / all, ares.rounds, run.round_frames, ares.active_left, what, ares.frames_used);
        printf("%f M samples / s, %d x %d, at most %d spp, %f s\n", (double)ares.samples / sec / 1e6, o.W, o.H, o.spp, sec);
    }
    else printf("%f M samples / s, %d x %d, %d spp, %f s\n", (double)o.W * o.H * o.spp / sec / 1e6, o.W, o.H, o.spp, sec);
    if (o.gpus > 1)
    {
        double tmax = 0, tsum = 0;
        printf("%d ranks (%s): kernel ms per rank", o.gpus, run.reducer.uses_rccl() ? "RCCL reduce" : "shared device, on-device sum");
        for (int r = 0; r < o.gpus; r++)
        {
            run.use(r);
            double ms = 0; int nl = 0;
            vp_render_time_ms(&ms, &nl, 1);
            printf(" %.2f", ms);
            tmax = std::max(tmax, ms); tsum += ms;
        }
        printf("; balance max/mean %.3f\n", tsum > 0 ? tmax / (tsum / o.gpus) : 1.0);
    }
}

// ---- capture (host.cpp:585-610, :508-517) from rank 0
static void write_image(const Job& j, const vp_float4* d_image, const std::string& name, bool hdr)
{
    Image image(j.o.W, j.o.H);
    vp_download(image.buffer(), d_image, (size_t)j.o.W * j.o.H * sizeof(vp_float4));
    if (hdr) image.dump_hdr(name.c_str());
    else image.dump_ppm(name.c_str());
    printf("wrote %s\n", name.c_str());
}
// a device map of one float per pixel, grey, as HDR
static void write_grey_map(const Job& j, const float* d_map, const std::string& name)
{
    const int          npix = j.o.W * j.o.H;
    std::vector<float> map((size_t)npix);
    must(vp_download(map.data(), d_map, (size_t)npix * sizeof(float)));
    Image im(j.o.W, j.o.H);
    for (int k = 0; k < npix; k++) { float* px = im.buffer() + 4 * (size_t)k; px[0] = px[1] = px[2] = map[(size_t)k]; px[3] = 1.0f; }
    im.dump_hdr(name.c_str());
    printf("wrote %s\n", name.c_str());
}

// --denoise-select: the two candidates of the cross-filter with the variance plane d_uf -- per candidate both halves filtered with the
// roles swapped, the error estimate of the pair, the merge into the candidate's image -- and the selection into disp; --select-out: the
// index map, the index as a grey value
static void select_beauty(const Job& j, const Run& run, const float* d_uf, const vp_denoise_feature* f, int nf)
{
    const Options& o = j.o;
    const Plane*   p = j.plane;
    const int      W = o.W, H = o.H, npix = run.npix;
    vp_denoise_params cand[2] = {o.dn, o.dns};
    cand[1].k = o.dn.k;
    vp_float4* d_img[2];
    float*     d_err[2];
    uint8_t*   d_index = o.select_out.empty() ? nullptr : (uint8_t*)vp_malloc((size_t)npix);
    must(!o.select_out.empty() && !d_index);
    for (int c = 0; c < 2; c++)
    {
        d_img[c] = device_alloc<vp_float4>(npix, false);
        d_err[c] = device_alloc<float>(npix, false);
        must(vp_denoise_var(p[0].mean, p[0].acc, p[0].rec, p[1].acc, p[1].rec, d_uf, f, nf, W, H, &cand[c]) ||
             vp_denoise_var(p[1].mean, p[1].acc, p[1].rec, p[0].acc, p[0].rec, d_uf, f, nf, W, H, &cand[c]) ||
             vp_cross_error(d_err[c], p[0].mean, p[1].mean, p[0].acc, p[0].rec, p[1].acc, p[1].rec, npix) ||
             vp_merge_halves(d_img[c], nullptr, p[0].mean, p[0].rec, p[1].mean, p[1].rec, npix, p[0].floor));
    }
    must(vp_select(run.disp, d_index, d_img, d_err, 2, W, H, &o.sel));
    if (d_index)
    {
        std::vector<uint8_t> idx((size_t)npix);
        must(vp_download(idx.data(), d_index, (size_t)npix));
        Image im(W, H);
        for (int k = 0; k < npix; k++) { float* px = im.buffer() + 4 * (size_t)k; px[0] = px[1] = px[2] = px[3] = (float)idx[(size_t)k]; }
        im.dump_hdr(o.select_out.c_str());
        printf("wrote %s\n", o.select_out.c_str());
    }
    must(vp_synchronize());
    for (int c = 0; c < 2; c++) { vp_free(d_img[c]); vp_free(d_err[c]); }
    if (d_index) vp_free(d_index);
}

// the beauty image's filter into disp: the division by each pixel's count is part of the call.  --denoise-features: the feature pass
// first, then the filter with three of its channels (alpha.y, zt and the cover flag).  --denoise-cross: each half with the other as
// guide, then the merge -- and, for --resid-out, the residual map, which is returned (the caller writes and frees it).  --denoise-var:
// the pooled variance of the halves and its filter in front, and both halves' filters with that plane as their guide's variance.
// --denoise-select: that at two windows, each candidate's error estimate and merge, and the per-pixel selection into disp
static float* denoise_beauty(const Job& j, const Run& run)
{
    const Options& o = j.o;
    const Plane*   p = j.plane;
    const int      W = o.W, H = o.H, npix = run.npix;
    vp_float4 *    d_alpha = nullptr, *d_depth = nullptr;
    float*         d_resid = nullptr;
    int            nf = 0;
    if (o.denoise_features)
    {
        d_alpha = (vp_float4*)vp_malloc((size_t)npix * sizeof(vp_float4));
        d_depth = (vp_float4*)vp_malloc((size_t)npix * sizeof(vp_float4));
        must(!d_alpha || !d_depth || vp_render_features(d_alpha, d_depth, &j.P, &o.feat));
        nf = 3;
    }
    const vp_denoise_feature f3[3] = {{d_alpha, 1, o.dn_sigma_alpha}, {d_depth, 1, o.dn_sigma_depth}, {d_depth, 3, o.dn_sigma_alpha}};
    const vp_denoise_feature* f = nf ? f3 : nullptr;
    if (j.n == 2)
    {
        must(!o.resid_out.empty() && !(d_resid = (float*)vp_malloc((size_t)npix * sizeof(float))));
        float* d_var[3] = {};   // --denoise-var: u, q and the filtered plane
        for (int k = 0; k < 3 && o.denoise_var; k++) d_var[k] = device_alloc<float>(npix, false);
        if (o.denoise_var) must(vp_halves_variance(d_var[0], d_var[1], p[0].rec, p[1].rec, npix) || vp_filter_variance(d_var[2], d_var[0], d_var[1], W, H, &o.dnv));
        const auto half = [&](int a, int b)   // half a with the weights of half b
        {
            return o.denoise_var ? vp_denoise_var(p[a].mean, p[a].acc, p[a].rec, p[b].acc, p[b].rec, d_var[2], f, nf, W, H, &o.dn)
                                 : vp_denoise_guided(p[a].mean, p[a].acc, p[a].rec, p[b].acc, p[b].rec, f, nf, W, H, &o.dn);
        };
        if (!o.denoise_select) must(half(0, 1) || half(1, 0) || vp_merge_halves(run.disp, d_resid, p[0].mean, p[0].rec, p[1].mean, p[1].rec, npix, p[0].floor));
        else select_beauty(j, run, d_var[2], f, nf);
        if (!o.var_out.empty()) write_grey_map(j, d_var[2], o.var_out);
        if (o.denoise_var) must(vp_synchronize());
        for (float* d : d_var) if (d) vp_free(d);
    }
    else must(nf ? vp_denoise_guided(run.disp, p[0].acc, p[0].rec, nullptr, nullptr, f, nf, W, H, &o.dn) : vp_denoise(run.disp, p[0].acc, p[0].rec, nullptr, nullptr, W, H, &o.dn));
    if (o.denoise_features)
    {
        must(vp_synchronize());
        vp_free(d_alpha);
        vp_free(d_depth);
    }
    printf("denoised: radius %d, patch %d, k %g\n", o.dn.radius, o.dn.patch, o.dn.k);
    if (o.denoise_cross) printf("  cross-filtered: two half-buffers, each with the other's weights, merged by their counts\n");
    if (o.denoise_var) printf("  variance: pooled from both halves, filtered at radius %d, patch %d, k %g\n", o.dnv.radius, o.dnv.patch, o.dnv.k);
    if (o.denoise_select)
        printf("  selected per pixel against radius %d, patch %d: errors smoothed at radius %d, picks blended at radius %d\n", o.dns.radius, o.dns.patch,
               o.sel.smooth_radius, o.sel.blend_radius);
    if (o.denoise_features) printf("  weights cut by features: sigma alpha %g, sigma depth %g\n", o.dn_sigma_alpha, o.dn_sigma_depth);
    return d_resid;
}

// the feature pass: a pass of its own behind the render, on rank 0 over the whole image, one camera ray per pixel
static void write_features(const Job& j, const Run& run)
{
    const Options& o = j.o;
    const int      npix = run.npix;
    vp_float4*     d_alpha = (vp_float4*)vp_malloc((size_t)npix * sizeof(vp_float4));
    vp_float4*     d_depth = (vp_float4*)vp_malloc((size_t)npix * sizeof(vp_float4));
    must(!d_alpha || !d_depth || vp_set_shard(0, 1) || vp_set_subpixel(1) || vp_render_features(d_alpha, d_depth, &j.P, &o.feat) || vp_synchronize());
    for (int k = 0; k < 2; k++)
    {
        const std::string name = o.features_out + (k ? "_depth.hdr" : "_alpha.hdr");
        Image fi(o.W, o.H);
        vp_download(fi.buffer(), k ? d_depth : d_alpha, (size_t)npix * sizeof(vp_float4));
        if (k)   // RGBE has no inf: a depth that does not exist is written as 0
            for (size_t q = 0; q < (size_t)npix * 4; q++) if (std::isinf(fi.buffer()[q])) fi.buffer()[q] = 0.0f;
        fi.dump_hdr(name.c_str());
        printf("wrote %s\n", name.c_str());
    }
    vp_free(d_alpha);
    vp_free(d_depth);
}

// --*-denoise-cross: the mean of every plane from its two halves -- each half filtered with the other as guide, the two merged by their
// counts into the plane's mean; --plane-denoise-var: the pooled variance of the plane's halves and its filter in front, both filters
// with that plane as their guide's variance; --plane-resid-out: the residual map of each plane, with the plane's floor
static void cross_planes(const Job& j, const Run& run)
{
    const Options& o = j.o;
    const int      W = o.W, H = o.H, npix = run.npix;
    float*         d_var[3] = {};   // u, q and the filtered plane, one plane after the other
    for (int k = 0; k < 3 && o.plane_denoise_var; k++) d_var[k] = device_alloc<float>(npix, false);
    float* d_resid = o.plane_resid_out.empty() ? nullptr : device_alloc<float>(npix, false);
    for (int k = 0; k < j.n; k++)
    {
        const Plane& a = j.plane[k];
        const Plane& b = j.other[k];
        if (o.plane_denoise_var)
            must(vp_halves_variance(d_var[0], d_var[1], a.rec, b.rec, npix) || vp_filter_variance(d_var[2], d_var[0], d_var[1], W, H, &o.dnv) ||
                 vp_denoise_var(a.mean, a.acc, a.rec, b.acc, b.rec, d_var[2], nullptr, 0, W, H, &o.dn) ||
                 vp_denoise_var(b.mean, b.acc, b.rec, a.acc, a.rec, d_var[2], nullptr, 0, W, H, &o.dn));
        else must(vp_denoise(a.mean, a.acc, a.rec, b.acc, b.rec, W, H, &o.dn) || vp_denoise(b.mean, b.acc, b.rec, a.acc, a.rec, W, H, &o.dn));
        must(vp_merge_halves(a.mean, d_resid, a.mean, a.rec, b.mean, b.rec, npix, a.floor));
        if (d_resid) write_grey_map(j, d_resid, o.plane_resid_out + a.suffix);
    }
    must(vp_synchronize());
    for (float* d : d_var) if (d) vp_free(d);
    if (d_resid) vp_free(d_resid);
}

static void write_outputs(const Job& j, const Run& run)
{
    const Options& o = j.o;
    const Plane*   p = j.plane;
    const int      W = o.W, H = o.H, npix = run.npix;
    vp_float4*     disp = run.disp;
    const float    per_frame = 1.0f / o.spp;
    float*         d_resid = nullptr;
    bool           linear = true;   // disp holds the linear image: gamma follows unless --out is HDR
    run.use(0);
    if (j.mode != BEAUTY)
    {
        // the mean of each plane -- by the filter with the plane's own records as guide (a MEAN image: the division by the count is part of
        // vp_denoise; w is never filtered), by the pixels' own counts after adaptive rounds, or by the one count of all --, written where a
        // prefix is given; then the planes' combination in place of the beauty image, the means with scale 1
        const vp_float4* m[3] = {};
        if (j.cross) cross_planes(j, run);
        for (int k = 0; k < j.n; k++)
        {
            if (j.cross) {}   // (the means are the cross-filter's)
            else if (j.filter) must(vp_denoise(p[k].mean, p[k].acc, p[k].rec, nullptr, nullptr, W, H, &o.dn));
            else if (j.adaptive) must(vp_scale_by_count(p[k].mean, p[k].acc, p[k].rec, npix, 1.0f));
            else if (!j.prefix.empty()) scale(disp, p[k].acc, npix, per_frame);
            m[k] = j.means ? p[k].mean : p[k].acc;
            if (!j.prefix.empty()) write_image(j, j.means ? p[k].mean : disp, j.prefix + p[k].suffix, true);
        }
        const float s = j.means ? 1.0f : per_frame;
        if (j.mode == PLANES) must(vp_relight_composite(disp, m[0], m[1], m[2], o.sun_gain, o.sky_gain, nullptr, o.over_rgb, npix, s));
        else if (j.mode == GROUPS) must(vp_relight(disp, m[0], m[1], o.sun_gain, o.sky_gain, npix, s));
        else if (o.over) must(vp_composite(disp, m[0], m[1], nullptr, o.over_rgb, npix, s));
        if (j.filter) printf("denoised per plane: radius %d, patch %d, k %g\n", o.dn.radius, o.dn.patch, o.dn.k);
        if (j.cross) printf("  cross-filtered: two halves of every plane, each with the other's weights, merged by their counts\n");
        if (j.cross && o.plane_denoise_var) printf("  variance: pooled from both halves of a plane, filtered at radius %d, patch %d, k %g\n", o.dnv.radius, o.dnv.patch, o.dnv.k);
    }
    else if (j.filter) d_resid = denoise_beauty(j, run);
    else if (j.adaptive) must(vp_scale_by_count(disp, p[0].acc, p[0].rec, npix, 1.0f));   // every pixel by its own count (the reference's scale assumes one count for all)
    else if (j.hdr) scale(disp, p[0].acc, npix, per_frame);
    else { gamma_correct(disp, p[0].acc, npix, per_frame, 2.2f); linear = false; }   // (the reference's one call for both)
    if (j.mode != LAYERS || o.over)   // layers without --over: the context's own sky is in neither layer, no image
    {
        if (linear && !j.hdr) gamma_correct(disp, disp, npix, 1.0f, 2.2f);
        write_image(j, disp, o.out, j.hdr);
    }
    if (d_resid)
    {
        write_grey_map(j, d_resid, o.resid_out);
        vp_free(d_resid);
    }
    // the noise maps: estimated standard error of the mean luminance over max(mean, floor), one per plane, each with its plane's floor
    // (rounds on halves: of the pooled records of a plane's two halves -- a zeroed scratch copy, both halves' records added)
    for (int k = 0; k < j.ntol && j.adaptive && !j.noise_prefix.empty(); k++)
    {
        float*                d_noise = (float*)vp_malloc((size_t)npix * sizeof(float));
        const vp_pixel_stats* rec = p[k].rec;
        vp_pixel_stats*       d_pooled = nullptr;
        if (j.halves_adaptive)
        {
            const vp_pixel_stats* second = j.mode == BEAUTY ? p[1].rec : j.other[k].rec;
            rec = d_pooled = device_alloc<vp_pixel_stats>(npix, true);
            must(vp_accumulate_stats(d_pooled, p[k].rec, (size_t)npix) || vp_accumulate_stats(d_pooled, second, (size_t)npix));
        }
        must(!d_noise || vp_stats_rel_error(d_noise, rec, npix, p[k].floor));
        write_grey_map(j, d_noise, j.noise_prefix + p[k].suffix);
        vp_free(d_noise);
        if (d_pooled) vp_free(d_pooled);
    }
    if (!o.features_out.empty()) write_features(j, run);
}

// the buffers first, then each rank's scene, the reducer's communicators (their collectives ran on the contexts' streams), the contexts
static void tear_down(Job& j, Run& run)
{
    free_planes(j);
    vp_free(run.disp);
    for (int r = 0; r < run.gpus; r++)
    {
        run.use(r);
        vp_free(run.accum[r]);
        free_cuda_buffers();
        free_envmap();
    }
    run.reducer.shutdown();
    if (run.gpus > 1) { vp_ctx_set_current(nullptr); for (auto c : run.ctx) vp_ctx_destroy(c); }
}

int main(int argc, char** argv)
{
    Options o;
    o.parse(argc, argv);
    Job job = validate(o);
    Run run;
    set_up(job, run);

    auto t0 = std::chrono::high_resolution_clock::now();
    alloc_planes(job, run);
    render(job, run);
    // ---- the one collective of the job: HDR accumulators -> rank 0
    std::string rerr;
    if (o.gpus > 1 && !run.reducer.reduce_to_root(run.ctx, run.accum, run.streams, (size_t)run.npix, rerr)) { fprintf(stderr, "%s\n", rerr.c_str()); return 1; }
    for (int r = o.gpus - 1; r >= 0; r--) { run.use(r); vp_synchronize(); }
    double sec = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - t0).count();

    report(job, run, sec);
    write_outputs(job, run);
    tear_down(job, run);
    return 0;
}
