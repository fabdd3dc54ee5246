// main.cpp -- volpath_render: headless driver in place of the reference's GLUT shell (host.cpp:1284-1403).
// It performs main()'s set-up sequence against the SAME entry points (init_cuda, set_texture_filter_mode,
// copy_inv_model_matrix, copy_inv_view_matrix, init_envmap, set_sun, precompute_opacity, render_kernel,
// scale / gamma_correct) and writes what the 'c' key captures (host.cpp:585-610): a .ppm of the
// gamma-corrected image or a .hdr of the scaled accumulator.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

int main(int argc, char** argv)
{
    int         julia = 128, W = 400, H = 300, spp = 16, preset = 12, brick = 1, batch = 0;
    float       density = 800.0f, g = 0.877f, sunx = 0.5f, suny = 0.2f;
    int         philox = 0;   // 0 sampler.h, 1 Philox2x32-10, 2 Philox2x32-7
    int         est = VP_EST_DECOMP, tracking = VP_TRACK_SPECTRAL, env_mode = VP_ENV_PASSIVE, arith = VP_ARITH_EXACT;
    std::string bin, vdb, out = "output0.ppm", devlist;
    int         vol_format = VP_VOL_U8;
    static_assert((int)VOLUME_U8 == (int)VP_VOL_U8 && (int)VOLUME_F32 == (int)VP_VOL_F32 && (int)VOLUME_F16 == (int)VP_VOL_F16, "the loaders' formats are vp_init_volume's");
    int         gpus = 1, aa = 0;   // (0: not given -- the contexts keep their default, VP_SUBPIXEL)
    bool        adaptive = false;
    float       noise_tol = 0.0f;
    const float noise_floor = 1e-3f;
    int         min_spp = 16, round_frames = 32;   // (the round: not measured yet)
    std::string noise_out;
    bool        denoise = false;
    vp_denoise_params dn = {5, 1, 0.45f};   // (from a 64 x 48 table, not tuned: DESIGN.md section 2.4)
    bool        denoise_features = false;
    bool        denoise_cross = false;   // --denoise-cross: two half-buffers, each filtered with the other's weights, merged
    std::string resid_out;
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
    const float planes_floor[3] = {1e-3f, 1e-3f, 1e-2f};   // (trans lives in [0, 1])
    std::string planes_noise_out;
    std::string features_out;
    vp_feature_params feat = {0.001f, VP_FEATURE_TAU_Z_DEFAULT};
    for (int i = 1; i < argc; i++)
    {
        std::string a = argv[i];
        auto need = [&](int n) { if (i + n >= argc) { usage(); exit(2); } };
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
            else { fprintf(stderr, "unknown --volume-format %s (u8, f32 or f16)\n", f); usage(); return 2; }
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
            else { fprintf(stderr, "unknown --arith %s\n", m); usage(); return 2; }
        }
        else if (a == "--aa")
        {
            need(1);
            const char* m = argv[++i];
            aa = !strcmp(m, "1") ? 1 : !strcmp(m, "2") ? 2 : !strcmp(m, "4") ? 4 : !strcmp(m, "8") ? 8 : 0;
            if (!aa) { fprintf(stderr, "unknown --aa %s (1, 2, 4 or 8)\n", m); usage(); return 2; }
        }
        else if (a == "--noise")
        {
            need(1);
            char* end = nullptr;
            noise_tol = strtof(argv[++i], &end);
            if (end == argv[i] || *end || !(noise_tol >= 0.0f)) { fprintf(stderr, "--noise %s: a tolerance >= 0\n", argv[i]); usage(); return 2; }
            adaptive = true;
        }
        else if (a == "--plane-noise")
        {
            need(2);
            for (int c = 0; c < 2; c++)
            {
                char* end = nullptr;
                plane_tol[c] = strtof(argv[++i], &end);
                if (end == argv[i] || *end || !(plane_tol[c] >= 0.0f)) { fprintf(stderr, "--plane-noise %s: two tolerances >= 0\n", argv[i]); usage(); return 2; }
            }
            plane_adaptive = true;
        }
        else if (a == "--plane-noise-out") { need(1); plane_noise_out = argv[++i]; }
        else if (a == "--planes-noise")
        {
            need(3);
            for (int c = 0; c < 3; c++)
            {
                char* end = nullptr;
                planes_tol[c] = strtof(argv[++i], &end);
                if (end == argv[i] || *end || !(planes_tol[c] >= 0.0f)) { fprintf(stderr, "--planes-noise %s: three tolerances >= 0\n", argv[i]); usage(); return 2; }
            }
            planes_adaptive = true;
        }
        else if (a == "--planes-noise-out") { need(1); planes_noise_out = argv[++i]; }
        else if (a == "--min-spp") { need(1); min_spp = atoi(argv[++i]); }
        else if (a == "--round") { need(1); round_frames = atoi(argv[++i]); }
        else if (a == "--noise-out") { need(1); noise_out = argv[++i]; }
        else if (a == "--denoise") denoise = true;
        else if (a == "--denoise-cross") denoise_cross = denoise = true;
        else if (a == "--resid-out") { need(1); resid_out = argv[++i]; }
        else if (a == "--denoise-radius" || a == "--denoise-patch" || a == "--denoise-k")
        {
            need(1);
            char* end = nullptr;
            const char* v = argv[++i];
            bool ok;
            if (a == "--denoise-k") { dn.k = strtof(v, &end); ok = end != v && !*end && std::isfinite(dn.k) && dn.k > 0.0f; }
            else
            {
                const long n = strtol(v, &end, 10);
                ok = end != v && !*end && n >= 0 && n <= (a == "--denoise-radius" ? VP_DENOISE_MAX_RADIUS : VP_DENOISE_MAX_PATCH);
                (a == "--denoise-radius" ? dn.radius : dn.patch) = (int)n;
            }
            if (!ok)
            {
                fprintf(stderr, "%s %s: radius 0..%d, patch 0..%d, k a finite number > 0\n", a.c_str(), v, VP_DENOISE_MAX_RADIUS, VP_DENOISE_MAX_PATCH);
                usage();
                return 2;
            }
        }
        else if (a == "--denoise-features") denoise_features = true;
        else if (a == "--denoise-sigma-alpha" || a == "--denoise-sigma-depth")
        {
            need(1);
            char* end = nullptr;
            const float v = strtof(argv[++i], &end);
            if (end == argv[i] || *end || !std::isfinite(v) || !(v > 0.0f)) { fprintf(stderr, "%s %s: a finite number > 0\n", a.c_str(), argv[i]); usage(); return 2; }
            (a == "--denoise-sigma-alpha" ? dn_sigma_alpha : dn_sigma_depth) = v;
        }
        else if (a == "--layers-out") { need(1); layers_out = argv[++i]; }
        else if (a == "--over")
        {
            need(3);
            for (int c = 0; c < 3; c++)
            {
                char* end = nullptr;
                over_rgb[c] = strtof(argv[++i], &end);
                if (end == argv[i] || *end || !std::isfinite(over_rgb[c])) { fprintf(stderr, "--over %s: three finite numbers\n", argv[i]); usage(); return 2; }
            }
            over = true;
        }
        else if (a == "--groups-out") { need(1); groups_out = argv[++i]; }
        else if (a == "--sun-gain" || a == "--sky-gain")
        {
            need(3);
            float* gain = a == "--sun-gain" ? sun_gain : sky_gain;
            for (int c = 0; c < 3; c++)
            {
                char* end = nullptr;
                gain[c] = strtof(argv[++i], &end);
                if (end == argv[i] || *end || !std::isfinite(gain[c])) { fprintf(stderr, "%s %s: three finite numbers\n", a.c_str(), argv[i]); usage(); return 2; }
            }
            relit = true;
        }
        else if (a == "--features-out") { need(1); features_out = argv[++i]; }
        else if (a == "--feature-step" || a == "--depth-tau")
        {
            need(1);
            char* end = nullptr;
            const float v = strtof(argv[++i], &end);
            if (end == argv[i] || *end || !std::isfinite(v) || !(v > 0.0f)) { fprintf(stderr, "%s %s: a finite number > 0\n", a.c_str(), argv[i]); usage(); return 2; }
            (a == "--feature-step" ? feat.step : feat.tau_z) = v;
        }
        else if (a == "--planes-out") { need(1); planes_out = argv[++i]; }
        else if (a == "--planes-denoise") planes_denoise = true;
        else if (a == "--groups-denoise") groups_denoise = true;
        else if (a == "--layers-denoise") layers_denoise = true;
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
            return ok ? 0 : 1;
        }
        else { usage(); return a == "--help" ? 0 : 2; }
    }

    Param P = default_param(W, H);  // host.cpp:1286-1292
    P.density = density;
    P.g       = g;
    if (!material_preset(P, preset)) { fprintf(stderr, "preset must be 0..12\n"); return 2; }

    if (vol_format != VP_VOL_U8 && bin.empty() && vdb.empty())
    {
        fprintf(stderr, "--volume-format %s needs --bin or --vdb: --julia voxelises to bytes (u8)\n", vol_format == VP_VOL_F16 ? "f16" : "f32");
        return 2;
    }
    // ---- the GPUs: one context per rank (a single rank runs in the default context, as the reference's host would)
    if (gpus < 1) { usage(); return 2; }
    if (adaptive && gpus > 1)
    {
        fprintf(stderr, "--noise with --gpus %d: reducing per-pixel statistics across ranks is not part of adaptive sampling; use one GPU\n", gpus);
        return 2;
    }
    if (!denoise_cross && !resid_out.empty()) { fprintf(stderr, "--resid-out needs --denoise-cross: the map is the disagreement of the two filtered halves\n"); return 2; }
    if (denoise_cross)
    {
        const char* other = gpus > 1 ? "--gpus" : adaptive ? "--noise" : !planes_out.empty() ? "--planes-out" : !groups_out.empty() ? "--groups-out" : relit ? "--sun-gain / --sky-gain"
                          : !layers_out.empty() ? "--layers-out" : over ? "--over" : plane_adaptive ? "--plane-noise" : planes_adaptive ? "--planes-noise"
                          : groups_denoise ? "--groups-denoise" : layers_denoise ? "--layers-denoise" : planes_denoise ? "--planes-denoise" : nullptr;
        if (other)
        {
            fprintf(stderr, "--denoise-cross with %s: the half-buffers' records are not reduced across ranks, adaptive rounds on halves are not built and the halves are "
                    "the beauty image's, not a plane's; use one GPU without --noise and without plane outputs or plane filters\n", other);
            return 2;
        }
    }
    if (denoise && gpus > 1)
    {
        fprintf(stderr, "--denoise with --gpus %d: the filter reads per-pixel statistics, which are not reduced across ranks; use one GPU\n", gpus);
        return 2;
    }
    if (denoise_features && (!denoise || aa > 1))
    {
        if (!denoise) fprintf(stderr, "--denoise-features needs --denoise: it cuts the weights of that filter (the per-plane filters do not take it)\n");
        else fprintf(stderr, "--denoise-features with --aa %d: the feature pass marches pixel-centre rays and refuses a sub-pixel factor; use --aa 1\n", aa);
        return 2;
    }
    // --planes-out: sun, sky and trans from one render; the gains and --over are then its parameters, not a groups or a layers render's
    const bool planes = !planes_out.empty();
    if (planes_denoise && !planes) { fprintf(stderr, "--planes-denoise needs --planes-out: it filters the three planes of that render\n"); return 2; }
    if (planes)
    {
        const char* other = gpus > 1 ? "--gpus" : adaptive ? "--noise" : denoise ? "--denoise" : !groups_out.empty() ? "--groups-out" : !layers_out.empty() ? "--layers-out"
                          : plane_adaptive ? "--plane-noise" : groups_denoise ? "--groups-denoise" : layers_denoise ? "--layers-denoise" : nullptr;
        if (other)
        {
            fprintf(stderr, "--planes-out with %s: the three planes are not reduced across ranks, are filtered by --planes-denoise only, are sampled adaptively by "
                    "--planes-noise only and replace the groups and the layers render; use one GPU without --noise, --denoise, --groups-out, --layers-out and "
                    "--plane-noise (three tolerances: --planes-noise TOL_SUN TOL_SKY TOL_TRANS)\n", other);
            return 2;
        }
        if (tracking != VP_TRACK_SPECTRAL || env_mode != VP_ENV_PASSIVE || arith != VP_ARITH_EXACT)
        {
            fprintf(stderr, "--planes-out needs spectral tracking, --env passive and --arith exact\n");
            return 2;
        }
    }
    // adaptive rounds on the three planes: --planes-out, one GPU, and neither the beauty image's rounds nor its filter (refused above)
    if (planes_adaptive && !planes) { fprintf(stderr, "--planes-noise needs --planes-out: it samples the three planes of that render\n"); return 2; }
    if (planes_adaptive && (min_spp < 2 || round_frames < 1)) { fprintf(stderr, "--planes-noise needs --min-spp >= 2 and --round >= 1\n"); usage(); return 2; }
    if (!planes_adaptive && !planes_noise_out.empty()) { fprintf(stderr, "--planes-noise-out needs --planes-noise\n"); return 2; }
    const bool layers = !planes && (over || !layers_out.empty());
    const bool groups = !planes && (relit || !groups_out.empty());
    // the per-plane filters: each needs its plane flag, one GPU, and neither the beauty image's filter nor adaptive rounds
    for (int k = 0; k < 2; k++)
    {
        const char* flag = k ? "--layers-denoise" : "--groups-denoise";
        if (!(k ? layers_denoise : groups_denoise)) continue;
        if (!(k ? layers : groups))
        {
            fprintf(stderr, "%s needs %s: it filters the planes of a %s render\n", flag, k ? "--layers-out or --over" : "--groups-out, --sun-gain or --sky-gain", k ? "layers" : "light-groups");
            return 2;
        }
        if (gpus > 1 || adaptive || denoise)
        {
            fprintf(stderr, "%s with %s: per-plane records are not reduced across ranks, adaptive rounds on planes are --plane-noise's, and --denoise filters the beauty image; "
                    "use one GPU without --noise and --denoise\n", flag, gpus > 1 ? "--gpus" : adaptive ? "--noise" : "--denoise");
            return 2;
        }
    }
    const bool plane_denoise = groups_denoise || layers_denoise;
    // adaptive rounds on planes: a plane flag, one GPU, and neither the beauty image's rounds nor its filter
    if (plane_adaptive && !layers && !groups)
    {
        fprintf(stderr, "--plane-noise needs --groups-out, --sun-gain or --sky-gain, or --layers-out or --over: it samples the planes of a light-groups or layers render\n");
        return 2;
    }
    if (plane_adaptive && (gpus > 1 || adaptive || denoise))
    {
        fprintf(stderr, "--plane-noise with %s: per-plane records are not reduced across ranks, --noise samples the beauty image and --denoise filters it; "
                "use one GPU without --noise and --denoise\n", gpus > 1 ? "--gpus" : adaptive ? "--noise" : "--denoise");
        return 2;
    }
    if (plane_adaptive && (min_spp < 2 || round_frames < 1)) { fprintf(stderr, "--plane-noise needs --min-spp >= 2 and --round >= 1\n"); usage(); return 2; }
    if (!plane_adaptive && !plane_noise_out.empty()) { fprintf(stderr, "--plane-noise-out needs --plane-noise\n"); return 2; }
    if (layers && (gpus > 1 || adaptive || denoise))
    {
        fprintf(stderr, "--layers-out / --over with %s: layers are not reduced across ranks and carry no per-pixel statistics; use one GPU without --noise and --denoise\n",
                gpus > 1 ? "--gpus" : adaptive ? "--noise" : "--denoise");
        return 2;
    }
    if (layers && (tracking != VP_TRACK_SPECTRAL || env_mode != VP_ENV_PASSIVE || arith != VP_ARITH_EXACT))
    {
        fprintf(stderr, "--layers-out / --over need spectral tracking, --env passive and --arith exact\n");
        return 2;
    }
    if (groups && (gpus > 1 || adaptive || denoise || layers))
    {
        fprintf(stderr, "--groups-out / --sun-gain / --sky-gain with %s: light groups are not reduced across ranks, carry no per-pixel statistics and are not combined with layers; "
                "use one GPU without --noise, --denoise, --layers-out and --over\n",
                gpus > 1 ? "--gpus" : adaptive ? "--noise" : denoise ? "--denoise" : over ? "--over" : "--layers-out");
        return 2;
    }
    if (groups && (tracking != VP_TRACK_SPECTRAL || env_mode != VP_ENV_PASSIVE || arith != VP_ARITH_EXACT))
    {
        fprintf(stderr, "--groups-out / --sun-gain / --sky-gain need spectral tracking, --env passive and --arith exact\n");
        return 2;
    }
    if (adaptive && (min_spp < 2 || round_frames < 1)) { fprintf(stderr, "--noise needs --min-spp >= 2 and --round >= 1\n"); usage(); return 2; }
    if (!adaptive && !noise_out.empty()) { fprintf(stderr, "--noise-out needs --noise\n"); return 2; }
    if (arith == VP_ARITH_FAST && (philox == 0 || est == VP_EST_BOUNDED || tracking != VP_TRACK_SPECTRAL || env_mode != VP_ENV_PASSIVE))
    {
        fprintf(stderr, "--arith fast needs --rng philox|philox7, --estimator decomp|global, spectral tracking and --env passive\n");
        return 2;
    }
    std::vector<int> devices;
    for (size_t pos = 0; pos < devlist.size();)
    {
        size_t e = devlist.find(',', pos);
        if (e == std::string::npos) e = devlist.size();
        devices.push_back(atoi(devlist.substr(pos, e - pos).c_str()));
        pos = e + 1;
    }
    if (devices.empty()) for (int r = 0; r < gpus; r++) devices.push_back(r);
    if ((int)devices.size() != gpus) { fprintf(stderr, "--devices must list %d devices\n", gpus); return 2; }
    if (gpus > 1 && batch <= 0) batch = std::min(spp, 256);  // shards render in batches: one launch per rank keeps every GPU busy
    std::vector<vp_ctx*> ctx(gpus, nullptr);
    if (gpus > 1)
        for (int r = 0; r < gpus; r++)
        {
            ctx[r] = vp_ctx_create(devices[r]);
            if (!ctx[r]) { fprintf(stderr, "%s\n", vp_last_error()); return 1; }
        }
    else if (vp_set_device(devices[0])) { fprintf(stderr, "%s\n", vp_last_error()); return 1; }
    auto use = [&](int r) { if (gpus > 1) vp_ctx_set_current(ctx[r]); };

    // ---- volume (host.cpp:1330-1344): loaded once, uploaded to every rank (all read-only scene data is replicated)
    int   width = 0, height = 0, depth = 0;
    void* h_volume = nullptr;
    if (!bin.empty()) h_volume = loadBinaryFileAs(bin.c_str(), width, height, depth, vol_format);
    else if (!vdb.empty()) h_volume = loadVdbFileAs(vdb.c_str(), width, height, depth, vol_format);
    else
    {
        width = height = depth = julia;
        h_volume = malloc((size_t)julia * julia * julia);
        use(0);
        if (!h_volume || vp_julia_voxelize(julia, (unsigned char*)h_volume)) { fprintf(stderr, "%s\n", vp_last_error()); return 1; }
    }
    if (!h_volume) return 1;
    vp_float3 box_min = {-1.0f, -(float)height / (float)width, -(float)depth / (float)width};
    vp_float3 box_max = {1.0f, (float)height / (float)width, (float)depth / (float)width};
    float identity[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    Camera cam;
    float  m[12];
    cam.inv_view_matrix(m);
    // sun / sky (host.cpp:1388-1390 -> update_sunsky)
    volpath::SunSky sky = volpath::bake_sunsky(sunx, suny);
    printf("sun power = %f, %f, %f\n", sky.sun_power.x, sky.sun_power.y, sky.sun_power.z);

    const int               npix = W * H;
    std::vector<vp_float4*> accum(gpus, nullptr);
    std::vector<void*>      streams(gpus, nullptr);
    for (int r = 0; r < gpus; r++)
    {
        use(r);
        vp_set_bound_brick(brick);
        if (vol_format == VP_VOL_U8) init_cuda(h_volume, vp_extent{(size_t)width, (size_t)height, (size_t)depth}, true, &box_min, &box_max);
        else if (vp_init_volume(h_volume, vp_extent{(size_t)width, (size_t)height, (size_t)depth}, vol_format, &box_min, &box_max))
        {
            fprintf(stderr, "%s\n", vp_last_error());
            return 1;
        }
        set_texture_filter_mode(true);
        copy_inv_model_matrix(identity, sizeof(identity));  // host.cpp:1350-1353
        copy_inv_view_matrix(m, sizeof(m));                 // host.cpp:617-623
        init_envmap(reinterpret_cast<const vp_float4*>(sky.envmap.data()), sky.width, sky.height);
        set_sun(&sky.sun_dir.x, &sky.sun_power.x);
        vp_set_estimator(est);
        if (vp_set_tracking(tracking) || vp_set_envmap_sampling(env_mode) || vp_set_shard(r, gpus)) { fprintf(stderr, "%s\n", vp_last_error()); return 1; }
        vp_set_rng(philox == 2 ? VP_RNG_PHILOX7 : philox ? VP_RNG_PHILOX : VP_RNG_SAMPLERH, 0x9E3779B9u, 0x85EBCA6Bu);
        if (vp_set_arithmetic(arith)) { fprintf(stderr, "%s\n", vp_last_error()); return 1; }
        if (aa && vp_set_subpixel(aa)) { fprintf(stderr, "%s\n", vp_last_error()); return 1; }
        // frame buffer (CudaFrameBuffer host.cpp:358-389), full frame on every rank: zero outside its tiles
        accum[r] = (vp_float4*)vp_malloc((size_t)npix * sizeof(vp_float4));
        if (!accum[r]) { fprintf(stderr, "%s\n", vp_last_error()); return 1; }
        vp_memset(accum[r], 0, (size_t)npix * sizeof(vp_float4));
        streams[r] = vp_get_stream();
    }
    free(h_volume);
    volpath::NodeReducer reducer;
    std::string          rerr;
    if (!reducer.init(devices, rerr)) { fprintf(stderr, "%s\n", rerr.c_str()); return 1; }
    if (gpus > 1) printf("multi-GPU reducer: %s\n", reducer.describe().c_str());
    use(0);
    vp_float4* disp = (vp_float4*)vp_malloc((size_t)npix * sizeof(vp_float4));
    if (!disp) { fprintf(stderr, "%s\n", vp_last_error()); return 1; }
    for (int r = 0; r < gpus; r++) { use(r); vp_synchronize(); vp_render_time_ms(nullptr, nullptr, 1); }

    auto t0 = std::chrono::high_resolution_clock::now();
    vp_dim3 block = {8, 8, 1}, grid = {(unsigned)(W + 7) / 8, (unsigned)(H + 7) / 8, 1};
    bool    have_opacity = false;
    vp_pixel_stats*    stats = nullptr;
    vp_adaptive_result ares = {};
    if (adaptive)
    {
        // rounds on the pixels that still need samples, --spp frames at most (vp_render_adaptive)
        use(0);
        stats = (vp_pixel_stats*)vp_malloc((size_t)npix * sizeof(vp_pixel_stats));
        if (!stats || vp_memset(stats, 0, (size_t)npix * sizeof(vp_pixel_stats))) { fprintf(stderr, "%s\n", vp_last_error()); return 1; }
        if (est == VP_EST_DECOMP && spp > 11) precompute_opacity(&sky.sun_dir.x);   // host.cpp:336-343
        const vp_adaptive ad = {noise_tol, noise_floor, min_spp, round_frames};
        if (vp_render_adaptive(accum[0], stats, 0, spp, &P, &ad, &ares)) { fprintf(stderr, "%s\n", vp_last_error()); return 1; }
    }
    if (denoise && !adaptive)
    {
        // the filter needs the records: the frames go through vp_render_frames_stats (the same accumulator bits)
        stats = (vp_pixel_stats*)vp_malloc((size_t)npix * sizeof(vp_pixel_stats));
        if (!stats || vp_memset(stats, 0, (size_t)npix * sizeof(vp_pixel_stats))) { fprintf(stderr, "%s\n", vp_last_error()); return 1; }
    }
    // --denoise-cross: accum[0] and `stats` are half 0's, these half 1's; the two filtered means
    vp_float4*      half1 = nullptr;
    vp_pixel_stats* half1_stats = nullptr;
    vp_float4*      half_mean[2] = {nullptr, nullptr};
    float*          d_resid = nullptr;   // --resid-out: the residual map, written with the merge
    if (denoise_cross)
    {
        half1       = (vp_float4*)vp_malloc((size_t)npix * sizeof(vp_float4));
        half1_stats = (vp_pixel_stats*)vp_malloc((size_t)npix * sizeof(vp_pixel_stats));
        for (vp_float4*& m2 : half_mean) m2 = (vp_float4*)vp_malloc((size_t)npix * sizeof(vp_float4));
        if (!half1 || !half1_stats || !half_mean[0] || !half_mean[1] || vp_memset(half1, 0, (size_t)npix * sizeof(vp_float4)) ||
            vp_memset(half1_stats, 0, (size_t)npix * sizeof(vp_pixel_stats)))
        {
            fprintf(stderr, "%s\n", vp_last_error());
            return 1;
        }
    }
    vp_float4* trans = nullptr;   // --layers-out / --over: accum[0] is the foreground accumulator, this the transmittance accumulator
    // (--groups-out / --sun-gain / --sky-gain: accum[0] is the sun accumulator, this the sky accumulator)
    // (--planes-out: accum[0] sun, this sky, trans3 the transmittance; stats3 and mean3 its records and its filtered mean)
    vp_float4*      trans3 = nullptr;
    vp_float4*      mean3  = nullptr;
    vp_pixel_stats* stats3 = nullptr;
    if (planes)
    {
        trans3 = (vp_float4*)vp_malloc((size_t)npix * sizeof(vp_float4));
        if (!trans3 || vp_memset(trans3, 0, (size_t)npix * sizeof(vp_float4))) { fprintf(stderr, "%s\n", vp_last_error()); return 1; }
        if (planes_denoise || planes_adaptive)
        {
            stats3 = (vp_pixel_stats*)vp_malloc((size_t)npix * sizeof(vp_pixel_stats));
            mean3  = (vp_float4*)vp_malloc((size_t)npix * sizeof(vp_float4));
            if (!stats3 || !mean3 || vp_memset(stats3, 0, (size_t)npix * sizeof(vp_pixel_stats))) { fprintf(stderr, "%s\n", vp_last_error()); return 1; }
        }
    }
    if (layers || groups || planes)
    {
        trans = (vp_float4*)vp_malloc((size_t)npix * sizeof(vp_float4));
        if (!trans || vp_memset(trans, 0, (size_t)npix * sizeof(vp_float4))) { fprintf(stderr, "%s\n", vp_last_error()); return 1; }
    }
    // --groups-denoise / --layers-denoise / --plane-noise: one record buffer per plane (`stats` the first plane's), and the two means
    vp_pixel_stats* stats2 = nullptr;
    vp_float4*      mean[2] = {nullptr, nullptr};
    const float     plane_floor[2] = {1e-3f, layers ? 1e-2f : 1e-3f};   // (trans lives in [0, 1])
    if (plane_denoise || plane_adaptive || planes_denoise || planes_adaptive)
    {
        stats  = (vp_pixel_stats*)vp_malloc((size_t)npix * sizeof(vp_pixel_stats));
        stats2 = (vp_pixel_stats*)vp_malloc((size_t)npix * sizeof(vp_pixel_stats));
        for (vp_float4*& m2 : mean) m2 = (vp_float4*)vp_malloc((size_t)npix * sizeof(vp_float4));
        if (!stats || !stats2 || !mean[0] || !mean[1] || vp_memset(stats, 0, (size_t)npix * sizeof(vp_pixel_stats)) || vp_memset(stats2, 0, (size_t)npix * sizeof(vp_pixel_stats)))
        {
            fprintf(stderr, "%s\n", vp_last_error());
            return 1;
        }
    }
    if (plane_adaptive)
    {
        // rounds on the pixels neither of whose planes has met its tolerance, --spp frames at most
        if (est == VP_EST_DECOMP && spp > 11) precompute_opacity(&sky.sun_dir.x);   // host.cpp:336-343
        const vp_adaptive_planes ap = {{plane_tol[0], plane_tol[1]}, {plane_floor[0], plane_floor[1]}, min_spp, round_frames};
        if ((layers ? vp_render_adaptive_layers : vp_render_adaptive_groups)(accum[0], trans, stats, stats2, 0, spp, &P, &ap, &ares))
        {
            fprintf(stderr, "%s\n", vp_last_error());
            return 1;
        }
    }
    if (planes_adaptive)
    {
        // rounds on the pixels none of whose three planes has met its tolerance, --spp frames at most
        if (est == VP_EST_DECOMP && spp > 11) precompute_opacity(&sky.sun_dir.x);   // host.cpp:336-343
        const vp_adaptive_planes3 ap = {{planes_tol[0], planes_tol[1], planes_tol[2]}, {planes_floor[0], planes_floor[1], planes_floor[2]}, min_spp, round_frames};
        if (vp_render_adaptive_group_layers(accum[0], trans, trans3, stats, stats2, stats3, 0, spp, &P, &ap, &ares)) { fprintf(stderr, "%s\n", vp_last_error()); return 1; }
    }
    for (int s = adaptive || plane_adaptive || planes_adaptive ? spp : 0; s < spp;)
    {
        if (!have_opacity && est == VP_EST_DECOMP && (s > 10 || (batch > 0 && s + batch > 11)))
        {
            for (int r = 0; r < gpus; r++) { use(r); precompute_opacity(&sky.sun_dir.x); }  // host.cpp:336-343
            have_opacity = true;
        }
        if (planes)
        {
            const int n = batch > 0 ? std::min(batch, spp - s) : 1;
            if (planes_denoise ? vp_render_frames_group_layers_stats(accum[0], trans, trans3, stats, stats2, stats3, s, n, &P)
                               : vp_render_frames_group_layers(accum[0], trans, trans3, s, n, &P)) { fprintf(stderr, "%s\n", vp_last_error()); return 1; }
            s += n;
        }
        else if (layers)
        {
            const int n = batch > 0 ? std::min(batch, spp - s) : 1;
            if (layers_denoise ? vp_render_frames_layers_stats(accum[0], trans, stats, stats2, s, n, &P) : vp_render_frames_layers(accum[0], trans, s, n, &P)) { fprintf(stderr, "%s\n", vp_last_error()); return 1; }
            s += n;
        }
        else if (groups)
        {
            const int n = batch > 0 ? std::min(batch, spp - s) : 1;
            if (groups_denoise ? vp_render_frames_groups_stats(accum[0], trans, stats, stats2, s, n, &P) : vp_render_frames_groups(accum[0], trans, s, n, &P)) { fprintf(stderr, "%s\n", vp_last_error()); return 1; }
            s += n;
        }
        else if (denoise)
        {
            const int n = batch > 0 ? std::min(batch, spp - s) : 1;
            if (denoise_cross ? vp_render_frames_halves_stats(accum[0], half1, stats, half1_stats, s, n, &P) : vp_render_frames_stats(accum[0], stats, s, n, &P))
            {
                fprintf(stderr, "%s\n", vp_last_error());
                return 1;
            }
            s += n;
        }
        else if (batch > 0)
        {
            int n = std::min(batch, spp - s);
            for (int r = 0; r < gpus; r++)  // asynchronous: every rank's launch is queued before any is waited for
            {
                use(r);
                if (vp_render_frames(accum[r], s, n, &P)) { fprintf(stderr, "%s\n", vp_last_error()); return 1; }
            }
            s += n;
        }
        else
        {
            use(0);
            render_kernel(grid, block, accum[0], s, P);  // host.cpp:631
            s += 1;
        }
    }
    // ---- the one collective of the job: HDR accumulators -> rank 0
    if (gpus > 1 && !reducer.reduce_to_root(ctx, accum, streams, (size_t)npix, rerr)) { fprintf(stderr, "%s\n", rerr.c_str()); return 1; }
    for (int r = gpus - 1; r >= 0; r--) { use(r); vp_synchronize(); }
    double sec = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - t0).count();
    if (adaptive || plane_adaptive || planes_adaptive)
    {
        const double all = (double)W * H * spp;
        char what[96];
        if (adaptive) snprintf(what, sizeof what, "--noise %g", noise_tol);
        else if (planes_adaptive) snprintf(what, sizeof what, "--planes-noise %g %g %g", planes_tol[0], planes_tol[1], planes_tol[2]);
        else snprintf(what, sizeof what, "--plane-noise %g %g", plane_tol[0], plane_tol[1]);
        printf("adaptive: %llu of %.0f samples (%.1f %%), %u rounds of %d frames, %u pixels still above %s after %u frames\n",
               (unsigned long long)ares.samples, all, 100.0 * (double)ares.samples / all, ares.rounds, round_frames, ares.active_left, what, ares.frames_used);
        printf("%f M samples / s, %d x %d, at most %d spp, %f s\n", (double)ares.samples / sec / 1e6, W, H, spp, sec);
    }
    else printf("%f M samples / s, %d x %d, %d spp, %f s\n", (double)W * H * spp / sec / 1e6, W, H, spp, sec);
    if (gpus > 1)
    {
        double tmax = 0, tsum = 0;
        printf("%d ranks (%s): kernel ms per rank", gpus, reducer.uses_rccl() ? "RCCL reduce" : "shared device, on-device sum");
        for (int r = 0; r < gpus; r++)
        {
            use(r);
            double ms = 0; int nl = 0;
            vp_render_time_ms(&ms, &nl, 1);
            printf(" %.2f", ms);
            tmax = std::max(tmax, ms); tsum += ms;
        }
        printf("; balance max/mean %.3f\n", tsum > 0 ? tmax / (tsum / gpus) : 1.0);
    }

    // ---- capture (host.cpp:585-610, :508-517) from rank 0
    use(0);
    bool  hdr = out.size() > 4 && out.substr(out.size() - 4) == ".hdr";
    Image image(W, H);
    if (planes)
    {
        // the three mean planes -- as they are, or each filtered with its own records as guide (a MEAN image: the division by the count
        // is part of vp_denoise; w is never filtered) --, then their relit composite over --over's colour in place of the beauty image
        // (--planes-noise without the filter: each plane by its own counts, sum / n per pixel, combined with scale 1)
        const bool means = planes_denoise || planes_adaptive;
        vp_float4* const       acc3[3] = {accum[0], trans, trans3};
        vp_float4* const       mean_of[3] = {mean[0], mean[1], mean3};
        vp_pixel_stats* const  rec3[3] = {stats, stats2, stats3};
        static const char* const suffix[3] = {"_sun.hdr", "_sky.hdr", "_trans.hdr"};
        for (int k = 0; k < 3; k++)
        {
            if (planes_denoise) { if (vp_denoise(mean_of[k], acc3[k], rec3[k], nullptr, nullptr, W, H, &dn)) { fprintf(stderr, "%s\n", vp_last_error()); return 1; } }
            else if (planes_adaptive) { if (vp_scale_by_count(mean_of[k], acc3[k], rec3[k], npix, 1.0f)) { fprintf(stderr, "%s\n", vp_last_error()); return 1; } }
            else scale(disp, acc3[k], npix, 1.0f / spp);
            const std::string name = planes_out + suffix[k];
            vp_download(image.buffer(), means ? mean_of[k] : disp, (size_t)npix * sizeof(vp_float4));
            image.dump_hdr(name.c_str());
            printf("wrote %s\n", name.c_str());
        }
        if (means ? vp_relight_composite(disp, mean_of[0], mean_of[1], mean_of[2], sun_gain, sky_gain, nullptr, over_rgb, npix, 1.0f)
                  : vp_relight_composite(disp, accum[0], trans, trans3, sun_gain, sky_gain, nullptr, over_rgb, npix, 1.0f / spp))
        {
            fprintf(stderr, "%s\n", vp_last_error());
            return 1;
        }
        if (!hdr) gamma_correct(disp, disp, npix, 1.0f, 2.2f);
        if (planes_denoise) printf("denoised per plane: radius %d, patch %d, k %g\n", dn.radius, dn.patch, dn.k);
    }
    else if (plane_denoise || plane_adaptive)
    {
        // each plane filtered with its own records as guide: two MEAN images (the division by the count is part of vp_denoise; w is
        // never filtered), written in place of the raw means and combined with scale 1
        // (--plane-noise without the filter: each plane by its own counts, sum / n per pixel)
        const bool        lay = layers;
        const std::string prefix = lay ? layers_out : groups_out;
        for (int k = 0; k < 2; k++)
        {
            if (plane_denoise ? vp_denoise(mean[k], k ? trans : accum[0], k ? stats2 : stats, nullptr, nullptr, W, H, &dn)
                              : vp_scale_by_count(mean[k], k ? trans : accum[0], k ? stats2 : stats, npix, 1.0f))
            {
                fprintf(stderr, "%s\n", vp_last_error());
                return 1;
            }
            if (prefix.empty()) continue;
            const std::string name = prefix + (lay ? (k ? "_trans.hdr" : "_fg.hdr") : (k ? "_sky.hdr" : "_sun.hdr"));
            vp_download(image.buffer(), mean[k], (size_t)npix * sizeof(vp_float4));
            image.dump_hdr(name.c_str());
            printf("wrote %s\n", name.c_str());
        }
        if (lay ? (over && vp_composite(disp, mean[0], mean[1], nullptr, over_rgb, npix, 1.0f)) : vp_relight(disp, mean[0], mean[1], sun_gain, sky_gain, npix, 1.0f))
        {
            fprintf(stderr, "%s\n", vp_last_error());
            return 1;
        }
        if (!hdr && (!lay || over)) gamma_correct(disp, disp, npix, 1.0f, 2.2f);
        if (plane_denoise) printf("denoised per plane: radius %d, patch %d, k %g\n", dn.radius, dn.patch, dn.k);
    }
    else if (layers)
    {
        // the two mean layers as they are; the composite over --over's colour in place of the beauty image
        if (!layers_out.empty())
            for (int k = 0; k < 2; k++)
            {
                const std::string name = layers_out + (k ? "_trans.hdr" : "_fg.hdr");
                scale(disp, k ? trans : accum[0], npix, 1.0f / spp);
                vp_download(image.buffer(), disp, (size_t)npix * sizeof(vp_float4));
                image.dump_hdr(name.c_str());
                printf("wrote %s\n", name.c_str());
            }
        if (over)
        {
            if (vp_composite(disp, accum[0], trans, nullptr, over_rgb, npix, 1.0f / spp)) { fprintf(stderr, "%s\n", vp_last_error()); return 1; }
            if (!hdr) gamma_correct(disp, disp, npix, 1.0f, 2.2f);
        }
    }
    else if (groups)
    {
        // the two mean groups as they are; their weighted sum in place of the beauty image
        if (!groups_out.empty())
            for (int k = 0; k < 2; k++)
            {
                const std::string name = groups_out + (k ? "_sky.hdr" : "_sun.hdr");
                scale(disp, k ? trans : accum[0], npix, 1.0f / spp);
                vp_download(image.buffer(), disp, (size_t)npix * sizeof(vp_float4));
                image.dump_hdr(name.c_str());
                printf("wrote %s\n", name.c_str());
            }
        if (vp_relight(disp, accum[0], trans, sun_gain, sky_gain, npix, 1.0f / spp)) { fprintf(stderr, "%s\n", vp_last_error()); return 1; }
        if (!hdr) gamma_correct(disp, disp, npix, 1.0f, 2.2f);
    }
    else if (denoise)
    {
        // the filtered mean image: the division by each pixel's count is part of the call
        // (--denoise-cross: each half with the other as guide, then the merge -- and the residual map, kept in d_resid for --resid-out)
        auto filter = [&](const vp_denoise_feature* f, int nf) -> int {
            if (!denoise_cross) return nf ? vp_denoise_guided(disp, accum[0], stats, nullptr, nullptr, f, nf, W, H, &dn) : vp_denoise(disp, accum[0], stats, nullptr, nullptr, W, H, &dn);
            if (!resid_out.empty() && !(d_resid = (float*)vp_malloc((size_t)npix * sizeof(float)))) return 1;
            return vp_denoise_guided(half_mean[0], accum[0], stats, half1, half1_stats, f, nf, W, H, &dn) ||
                   vp_denoise_guided(half_mean[1], half1, half1_stats, accum[0], stats, f, nf, W, H, &dn) ||
                   vp_merge_halves(disp, d_resid, half_mean[0], stats, half_mean[1], half1_stats, npix, noise_floor);
        };
        if (denoise_features)
        {
            // the feature pass first, then the filter with three of its channels: alpha.y, zt and the cover flag
            vp_float4* d_alpha = (vp_float4*)vp_malloc((size_t)npix * sizeof(vp_float4));
            vp_float4* d_depth = (vp_float4*)vp_malloc((size_t)npix * sizeof(vp_float4));
            const vp_denoise_feature f3[3] = {{d_alpha, 1, dn_sigma_alpha}, {d_depth, 1, dn_sigma_depth}, {d_depth, 3, dn_sigma_alpha}};
            if (!d_alpha || !d_depth || vp_render_features(d_alpha, d_depth, &P, &feat) || filter(f3, 3)
                || vp_synchronize())
            {
                fprintf(stderr, "%s\n", vp_last_error());
                return 1;
            }
            vp_free(d_alpha);
            vp_free(d_depth);
        }
        else if (filter(nullptr, 0)) { fprintf(stderr, "%s\n", vp_last_error()); return 1; }
        if (!hdr) gamma_correct(disp, disp, npix, 1.0f, 2.2f);
        printf("denoised: radius %d, patch %d, k %g\n", dn.radius, dn.patch, dn.k);
        if (denoise_cross) printf("  cross-filtered: two half-buffers, each with the other's weights, merged by their counts\n");
        if (denoise_features) printf("  weights cut by features: sigma alpha %g, sigma depth %g\n", dn_sigma_alpha, dn_sigma_depth);
    }
    else if (adaptive)
    {
        // every pixel by its own count (the reference's scale assumes one count for all)
        if (vp_scale_by_count(disp, accum[0], stats, npix, 1.0f)) { fprintf(stderr, "%s\n", vp_last_error()); return 1; }
        if (!hdr) gamma_correct(disp, disp, npix, 1.0f, 2.2f);
    }
    else if (hdr) scale(disp, accum[0], npix, 1.0f / spp);
    else gamma_correct(disp, accum[0], npix, 1.0f / spp, 2.2f);
    if (!layers || over)
    {
        vp_download(image.buffer(), disp, (size_t)npix * sizeof(vp_float4));
        if (hdr) image.dump_hdr(out.c_str());
        else image.dump_ppm(out.c_str());
        printf("wrote %s\n", out.c_str());
    }
    if (d_resid)
    {
        // the residual map of the cross-filter, grey, as HDR
        std::vector<float> resid((size_t)npix);
        if (vp_download(resid.data(), d_resid, (size_t)npix * sizeof(float))) { fprintf(stderr, "%s\n", vp_last_error()); return 1; }
        Image rm(W, H);
        for (int k = 0; k < npix; k++) { float* px = rm.buffer() + 4 * (size_t)k; px[0] = px[1] = px[2] = resid[(size_t)k]; px[3] = 1.0f; }
        rm.dump_hdr(resid_out.c_str());
        printf("wrote %s\n", resid_out.c_str());
        vp_free(d_resid);
    }
    if (adaptive && !noise_out.empty())
    {
        // the noise map: estimated standard error of the mean luminance over max(mean, floor), grey, as HDR
        float* d_noise = (float*)vp_malloc((size_t)npix * sizeof(float));
        std::vector<float> noise((size_t)npix);
        if (!d_noise || vp_stats_rel_error(d_noise, stats, npix, noise_floor) || vp_download(noise.data(), d_noise, (size_t)npix * sizeof(float)))
        {
            fprintf(stderr, "%s\n", vp_last_error());
            return 1;
        }
        Image nm(W, H);
        for (int k = 0; k < npix; k++) { float* px = nm.buffer() + 4 * (size_t)k; px[0] = px[1] = px[2] = noise[(size_t)k]; px[3] = 1.0f; }
        nm.dump_hdr(noise_out.c_str());
        printf("wrote %s\n", noise_out.c_str());
        vp_free(d_noise);
    }
    if (plane_adaptive && !plane_noise_out.empty())
        for (int k = 0; k < 2; k++)
        {
            // one noise map per plane, each with its plane's floor
            const std::string name = plane_noise_out + (layers ? (k ? "_trans.hdr" : "_fg.hdr") : (k ? "_sky.hdr" : "_sun.hdr"));
            float* d_noise = (float*)vp_malloc((size_t)npix * sizeof(float));
            std::vector<float> noise((size_t)npix);
            if (!d_noise || vp_stats_rel_error(d_noise, k ? stats2 : stats, npix, plane_floor[k]) || vp_download(noise.data(), d_noise, (size_t)npix * sizeof(float)))
            {
                fprintf(stderr, "%s\n", vp_last_error());
                return 1;
            }
            Image nm(W, H);
            for (int q = 0; q < npix; q++) { float* px = nm.buffer() + 4 * (size_t)q; px[0] = px[1] = px[2] = noise[(size_t)q]; px[3] = 1.0f; }
            nm.dump_hdr(name.c_str());
            printf("wrote %s\n", name.c_str());
            vp_free(d_noise);
        }
    if (planes_adaptive && !planes_noise_out.empty())
        for (int k = 0; k < 3; k++)
        {
            // one noise map per plane, each with its plane's floor
            static const char* const suffix[3] = {"_sun.hdr", "_sky.hdr", "_trans.hdr"};
            vp_pixel_stats* const    rec3[3] = {stats, stats2, stats3};
            const std::string name = planes_noise_out + suffix[k];
            float* d_noise = (float*)vp_malloc((size_t)npix * sizeof(float));
            std::vector<float> noise((size_t)npix);
            if (!d_noise || vp_stats_rel_error(d_noise, rec3[k], npix, planes_floor[k]) || vp_download(noise.data(), d_noise, (size_t)npix * sizeof(float)))
            {
                fprintf(stderr, "%s\n", vp_last_error());
                return 1;
            }
            Image nm(W, H);
            for (int q = 0; q < npix; q++) { float* px = nm.buffer() + 4 * (size_t)q; px[0] = px[1] = px[2] = noise[(size_t)q]; px[3] = 1.0f; }
            nm.dump_hdr(name.c_str());
            printf("wrote %s\n", name.c_str());
            vp_free(d_noise);
        }
    if (!features_out.empty())
    {
        // the feature pass: a pass of its own behind the render, on rank 0 over the whole image, one camera ray per pixel
        vp_float4* d_alpha = (vp_float4*)vp_malloc((size_t)npix * sizeof(vp_float4));
        vp_float4* d_depth = (vp_float4*)vp_malloc((size_t)npix * sizeof(vp_float4));
        if (!d_alpha || !d_depth || vp_set_shard(0, 1) || vp_set_subpixel(1) || vp_render_features(d_alpha, d_depth, &P, &feat) || vp_synchronize())
        {
            fprintf(stderr, "%s\n", vp_last_error());
            return 1;
        }
        for (int k = 0; k < 2; k++)
        {
            const std::string name = features_out + (k ? "_depth.hdr" : "_alpha.hdr");
            Image fi(W, H);
            vp_download(fi.buffer(), k ? d_depth : d_alpha, (size_t)npix * sizeof(vp_float4));
            if (k)   // RGBE has no inf: a depth that does not exist is written as 0
                for (size_t q = 0; q < (size_t)npix * 4; q++) if (std::isinf(fi.buffer()[q])) fi.buffer()[q] = 0.0f;
            fi.dump_hdr(name.c_str());
            printf("wrote %s\n", name.c_str());
        }
        vp_free(d_alpha);
        vp_free(d_depth);
    }
    if (stats) vp_free(stats);
    if (stats2) vp_free(stats2);
    if (stats3) vp_free(stats3);
    if (mean3) vp_free(mean3);
    if (trans3) vp_free(trans3);
    for (vp_float4* m2 : mean) if (m2) vp_free(m2);
    if (trans) vp_free(trans);
    if (half1) vp_free(half1);
    if (half1_stats) vp_free(half1_stats);
    for (vp_float4* m2 : half_mean) if (m2) vp_free(m2);
    vp_free(disp);
    for (int r = 0; r < gpus; r++)
    {
        use(r);
        vp_free(accum[r]);
        free_cuda_buffers();
        free_envmap();
    }
    reducer.shutdown();   // communicators first: their collectives ran on the contexts' streams
    if (gpus > 1) { vp_ctx_set_current(nullptr); for (auto c : ctx) vp_ctx_destroy(c); }
    return 0;
}
