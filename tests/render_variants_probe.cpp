// render_variants_probe.cpp -- tabulates which render_k instance and which approach kernel csrc/vp_dispatch.h launches for every
// request the API admits, through the real launcher (tests/test_render_variants_cpu.py builds and runs it).
//
// Host only: hipcc --cuda-host-only -std=c++17 -Icuda-volpath_amd/csrc [-DVP_ARITH_FAST] [-DVP_DEV_BUILD].  The kernels are host
// stand-ins with the kernels' template parameter lists that write their arguments down, hipLaunchKernelGGL calls the stand-in, and
// kernel_not_built() throws back to the loop: no HIP runtime call, no device.
//
// Output: one line per group of requests, one cell per request (the columns: tests/golden/render_variants.txt).  A cell is the
// kernel launched, `-` where the build has none (kernel_not_built), `.` where the API refuses the request; a line without a kernel
// is left out, and the last line counts the requests and the `-` among them.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <string>
#include <utility>

#include "vp_device.h"
#include "vp_kernels.h"

static std::string g_kernel, g_line;
static unsigned    g_grid[2], g_block, g_requests, g_not_built;
struct NotBuilt {};

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, shmem, stream, ...) \
    do { g_grid[0] = dim3(grid).x; g_grid[1] = dim3(grid).y; g_block = dim3(block).x; (kernel)(__VA_ARGS__); } while (0)
#define VP_SEG_CAP 96   // (vp_integrator.h's; the launcher only asserts its range)

namespace vp
{
[[noreturn]] void kernel_not_built() { throw NotBuilt{}; }
void census_record(int, int, unsigned) {}   // (the library's launch census: nothing to count here)
namespace probe
{
template <class RNG> constexpr int rng_id();
template <> constexpr int rng_id<RngSamplerH>() { return RNG_SAMPLERH; }
template <> constexpr int rng_id<RngPhilox>() { return RNG_PHILOX; }
template <> constexpr int rng_id<RngPhilox7>() { return RNG_PHILOX7; }

// render_k: its template arguments as digits, EST RNG . QUANT COUNT LDSB ACH MIS . TRK LIGHT CANCEL HALF
template <int EST, class RNG, bool QUANT, bool COUNT, int LDSB, bool ACH, bool MIS, int TRK, bool LIGHT = false, bool CANCEL = false, bool HALF = false>
void render_k(SceneDev, LaunchDev)
{
    char b[32];
    snprintf(b, sizeof b, "%d%d.%d%d%d%d%d.%d%d%d%d", EST, rng_id<RNG>(), QUANT, COUNT, LDSB, ACH, MIS, TRK, LIGHT, CANCEL, HALF);
    g_kernel = b;
}
// approach_k<RNG>: gR, approach_local_k<RNG, QUANT>: lRQ, approach_local_tab_k<RNG>: tR
template <class RNG> void approach_k(SceneDev, LaunchDev) { g_kernel = "g" + std::to_string(rng_id<RNG>()); }
template <class RNG, bool QUANT> void approach_local_k(SceneDev, LaunchDev) { g_kernel = "l" + std::to_string(rng_id<RNG>()) + (QUANT ? "1" : "0"); }
template <class RNG> void approach_local_tab_k(SceneDev, LaunchDev) { g_kernel = "t" + std::to_string(rng_id<RNG>()); }

// >>> the launchers under test
#include "vp_dispatch.h"
static const auto probe_render = dispatch_render;
static const auto probe_light = dispatch_light;
static const auto probe_approach = dispatch_approach;
// <<< the launchers under test

// one request: its cell, with `:block` unless 256 threads and `@grid` unless the grid is the `blocks` asked for (7)
template <class F>
static void cell(F launch)
{
    g_kernel.clear(); g_grid[0] = g_grid[1] = g_block = 0;
    g_requests++;
    try { launch(); }
    catch (const NotBuilt&) { g_not_built++; g_line += " -"; return; }
    g_line += " " + g_kernel;
    if (g_block != 256u) g_line += ":" + std::to_string(g_block);
    if (g_grid[0] != 7u || g_grid[1] != 1u) g_line += "@" + std::to_string(g_grid[0]) + "x" + std::to_string(g_grid[1]);
}
static void refused() { g_line += " ."; }
static void end_line(const char* key)
{
    if (g_line.find_first_not_of(" -.") != std::string::npos) printf("%s:%s\n", key, g_line.c_str());   // (a kernel in some cell)
    g_line.clear();
}
}  // namespace probe
}  // namespace vp

int main()
{
    using namespace vp;
    using namespace vp::probe;
    const bool fast = kFastArith, dev = kDevBuild;   // the domain is what vp_render.cpp check_render admits in this build's mode
    const SceneDev S{};
    static unsigned cancel_word;
    static const float4 seg_table[1] = {};
    char key[96];
    for (int est : {EST_GLOBAL, EST_DECOMP, EST_BOUNDED})
        for (int rng : {RNG_SAMPLERH, RNG_PHILOX, RNG_PHILOX7})
        {
            if (fast && (est == EST_BOUNDED || rng == RNG_SAMPLERH)) continue;
            // render_k: fmt 0 uchar, 1 float, 2 binary16; the cells of a line: trk 0 1 2 x cancel 0 1 x ach 0 1
            for (int fmt = 0; fmt < 3; fmt++)
                for (int count = 0; count < 2; count++)
                    for (int mis = 0; mis < 2; mis++)
                    {
                        std::string lines[3];   // per LDS form asked for; printed as one line, lds=*, where the form makes no difference
                        for (int lds = 0; lds < 3; lds++)
                        {
                            for (int trk = 0; trk < 3; trk++)
                                for (int cancel = 0; cancel < 2; cancel++)
                                    for (int ach = 0; ach < 2; ach++)
                                    {
                                        if ((trk && (mis || count)) || (rng == RNG_PHILOX7 && (trk || mis)) || (fast && (count || mis || trk))) { refused(); continue; }
                                        LaunchDev L{};
                                        L.cancel = cancel ? &cancel_word : nullptr;
                                        for (int c = 0; c < 3; c++) { L.P.sigma_t[c] = ach ? 1.0f : 1.0f + (float)c; L.P.albedo[c] = 0.5f; }
                                        cell([&] { probe_render(S, L, est, rng, fmt == 0, fmt == 2, count != 0, lds, mis != 0, trk, 7, nullptr); });
                                    }
                            lines[lds].swap(g_line);
                        }
                        const bool same = lines[0] == lines[1] && lines[1] == lines[2];
                        for (int lds = 0; lds < (same ? 1 : 3); lds++)
                        {
                            snprintf(key, sizeof key, "render est=%d rng=%d fmt=%d count=%d mis=%d lds=%c", est, rng, fmt, count, mis, same ? '*' : '0' + lds);
                            g_line = lines[lds];
                            end_line(key);
                        }
                    }
            // the light class is the exact build's; the development build admits the uchar volume only.  Cells: quant 1 0 x count 0 1
            for (int quant = 1; quant >= 0; quant--)
                for (int count = 0; count < 2; count++)
                {
                    if (fast || (dev && !quant)) { refused(); continue; }
                    LaunchDev L{};
                    cell([&] { probe_light(S, L, est, rng, quant != 0, count != 0, 7, nullptr); });
                }
            snprintf(key, sizeof key, "light est=%d rng=%d", est, rng);
            end_line(key);
            // the approach walk, 1000 pixel slots x 100 frames.  Cells: quant 1 0 x segment table no yes x fshift 6 3
            for (int quant = 1; quant >= 0; quant--)
                for (int tab = 0; tab < 2; tab++)
                    for (unsigned fshift : {6u, 3u})
                    {
                        LaunchDev L{};
                        L.nslots = 1000; L.nframes = 100; L.approach_fshift = fshift; L.seg_table = tab ? seg_table : nullptr;
                        cell([&] { probe_approach(S, L, est, rng, quant != 0, nullptr); });
                    }
            snprintf(key, sizeof key, "approach est=%d rng=%d", est, rng);
            end_line(key);
        }
    printf("requests %u, not built %u\n", g_requests, g_not_built);
    return 0;
}
