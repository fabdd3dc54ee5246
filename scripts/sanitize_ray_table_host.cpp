// sanitize_ray_table_host.cpp -- the host side of the per-view ray table (csrc/vp_tables.cpp ensure_ray_table: key, grow, fall-back)
// as a stand-alone program for AddressSanitizer + UndefinedBehaviorSanitizer, with stand-ins for the HIP runtime and for the launches:
// no device, nothing loaded into Python.  Built and run by scripts/sanitize_ray_table_host.sh; exit status 0 = every check held.
#include "../cuda-volpath_amd/csrc/vp_state.h"

static int    g_launches = 0, g_quiesced = 0;
static bool   g_malloc_fails = false;
static size_t g_live = 0;

// ---- the HIP runtime: the heap, so that the sanitizer sees every block the table code allocates, writes and frees
extern "C" {
hipError_t hipMalloc(void** p, size_t n)
{
    if (g_malloc_fails) { *p = nullptr; return hipErrorOutOfMemory; }
    *p = malloc(n);
    g_live++;
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipFree(void* p) { if (p) g_live--; free(p); return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "stand-in"; }
// (what the other tables of vp_tables.cpp call: not reached from here)
hipError_t hipHostFree(void*) { abort(); }
hipError_t hipHostGetDevicePointer(void**, void*, unsigned) { abort(); }
hipError_t hipHostMalloc(void**, size_t, unsigned) { abort(); }
hipError_t hipMemGetInfo(size_t*, size_t*) { abort(); }
hipError_t hipMemcpy(void*, const void*, size_t, hipMemcpyKind) { abort(); }
hipError_t hipMemcpyAsync(void*, const void*, size_t, hipMemcpyKind, hipStream_t) { abort(); }
hipError_t hipMemsetAsync(void*, int, size_t, hipStream_t) { abort(); }
}

// ---- the launches: the ray table's writes what ray_table_k writes (two float4 per slot), the others are not reached
namespace vp
{
void launch_ray_table(const SceneDev&, unsigned, unsigned, const float4* crawl, const unsigned* pixels, unsigned nslots, float4* table, hipStream_t)
{
    g_launches++;
    for (unsigned s = 0; s < nslots; s++)
    {
        const float w = (float)pixels[s] + (crawl ? crawl[0].x : 0.0f);
        table[2 * (size_t)s] = table[2 * (size_t)s + 1] = make_float4(w, w, w, w);
    }
}
float    sun_clip_step(const SceneDev&) { abort(); }
unsigned segment_table_records(void) { abort(); }
void launch_opacity(const SceneDev&, bool, bool, bool, const float*, float*, hipStream_t) { abort(); }
void launch_pack_f32(const float*, float*, int, int, int, bool, hipStream_t) { abort(); }
void launch_sun_clip(const SceneDev&, const unsigned char*, float, unsigned short*, hipStream_t) { abort(); }
void launch_thr_table(const ParamDev&, float*, unsigned, hipStream_t) { abort(); }
void launch_bound_bytes(const unsigned char*, size_t, unsigned*, hipStream_t) { abort(); }
void launch_crawl_table(const SceneDev&, bool, unsigned, unsigned, bool, const unsigned char*, float4*, hipStream_t) { abort(); }
void launch_empty_table(const SceneDev&, unsigned, unsigned, const unsigned char*, float4*, hipStream_t) { abort(); }
void launch_pixel_lists(unsigned, unsigned, unsigned, unsigned, unsigned, const unsigned*, const float4*, const unsigned char*, unsigned*, unsigned*, unsigned*,
                        hipStream_t) { abort(); }
void launch_segment_table(const SceneDev&, unsigned, unsigned, const float4*, const unsigned*, unsigned, float4*, hipStream_t) { abort(); }
void launch_light_identity(const ParamDev&, bool, const unsigned*, unsigned*, hipStream_t) { abort(); }
void launch_light_identity_fast(const ParamDev&, bool, const unsigned*, unsigned*, hipStream_t) { abort(); }
void launch_subpixel_classes(const float4*, unsigned, unsigned, unsigned, unsigned char*, hipStream_t) { abort(); }
}  // namespace vp

namespace vph
{
State& cur() { static State s; return s; }
int    la_quiesce() { g_quiesced++; return 0; }
int    ensure_device() { return 0; }
int    fail(int code, const char* fmt, ...) { fprintf(stderr, "fail(%d): %s\n", code, fmt); return code; }
}  // namespace vph

using namespace vph;

#define CHECK(cond)                                                                       \
    do                                                                                    \
    {                                                                                     \
        if (!(cond)) { fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #cond); return 1; } \
    } while (0)

int main()
{
    Param P = {};
    P.width = 37; P.height = 19;
    const unsigned cap = 8192;
    std::vector<unsigned> pixels(cap);
    for (unsigned i = 0; i < cap; i++) pixels[i] = i;
    std::vector<float4> crawl(2 * 37 * 19, make_float4(0.5f, 0.0f, 0.0f, 0.0f));
    G.est = VP_EST_GLOBAL; G.world = 1; G.rank = 0;
    G.d_tiles.p = pixels.data(); G.d_tiles.bytes = cap * sizeof(unsigned);   // (never freed through DevBuf: reset before exit)
    G.tiles_key.assign({1, 2, 3});
    G.n_general = 100;
    const float4* t = nullptr;

    // built on first use, cached on the second
    CHECK(ensure_ray_table(&P, nullptr, &t) == VP_OK && t && g_launches == 1 && G.d_ray.bytes == 100 * 32);
    CHECK(t[199].x == 99.0f);
    CHECK(ensure_ray_table(&P, nullptr, &t) == VP_OK && t == G.d_ray.p && g_launches == 1);
    // the key: camera, box, image size, shard, pixel lists, the crawl table's presence and key
    G.S.cam[3] += 1.0f;       CHECK(ensure_ray_table(&P, nullptr, &t) == VP_OK && t && g_launches == 2);
    G.S.bmax[1] = 2.0f;       CHECK(ensure_ray_table(&P, nullptr, &t) == VP_OK && t && g_launches == 3);
    P.width = 24;             CHECK(ensure_ray_table(&P, nullptr, &t) == VP_OK && t && g_launches == 4);
    G.rank = 1; G.world = 2;  CHECK(ensure_ray_table(&P, nullptr, &t) == VP_OK && t && g_launches == 5);
    G.tiles_key.push_back(9); CHECK(ensure_ray_table(&P, nullptr, &t) == VP_OK && t && g_launches == 6);
    G.crawl_key.assign({7});  CHECK(ensure_ray_table(&P, nullptr, &t) == VP_OK && t && g_launches == 6);   // (no crawl table: its key is not the table's)
    CHECK(ensure_ray_table(&P, crawl.data(), &t) == VP_OK && t && g_launches == 7 && t[0].x == 0.5f);
    G.crawl_key.assign({8});  CHECK(ensure_ray_table(&P, crawl.data(), &t) == VP_OK && t && g_launches == 8);
    CHECK(ensure_ray_table(&P, crawl.data(), &t) == VP_OK && t && g_launches == 8);
    CHECK(g_quiesced == g_launches);   // every rebuild waits for the launches that read the old table
    // fewer slots: the block is kept; more: it grows (the old block is freed first)
    G.n_general = 10;   CHECK(ensure_ray_table(&P, crawl.data(), &t) == VP_OK && t && g_launches == 9 && G.d_ray.bytes == 100 * 32);
    G.n_general = 4000; CHECK(ensure_ray_table(&P, crawl.data(), &t) == VP_OK && t && g_launches == 10 && G.d_ray.bytes == 4000 * 32 && g_live == 1);
    CHECK(t[7999].w == 3999.5f);
    // no memory: no table, no error, nothing stale -- and a table again once there is memory
    g_malloc_fails = true;
    G.n_general = cap;  CHECK(ensure_ray_table(&P, crawl.data(), &t) == VP_OK && !t && g_launches == 10 && !G.d_ray.p && !G.d_ray.bytes && G.ray_key.empty() && g_live == 0);
    CHECK(ensure_ray_table(&P, crawl.data(), &t) == VP_OK && !t && g_launches == 10);
    g_malloc_fails = false;
    CHECK(ensure_ray_table(&P, crawl.data(), &t) == VP_OK && t && g_launches == 11 && G.d_ray.bytes == (size_t)cap * 32);
    // where the configuration has no table
    G.use_ray_table = false;   CHECK(ensure_ray_table(&P, crawl.data(), &t) == VP_OK && !t); G.use_ray_table = true;
    G.est = VP_EST_DECOMP;     CHECK(ensure_ray_table(&P, crawl.data(), &t) == VP_OK && !t); G.est = VP_EST_GLOBAL;
    G.sub_shift = 1;           CHECK(ensure_ray_table(&P, crawl.data(), &t) == VP_OK && !t); G.sub_shift = 0;
    G.n_general = 0;           CHECK(ensure_ray_table(&P, crawl.data(), &t) == VP_OK && !t); G.n_general = cap;
    CHECK(ensure_ray_table(&P, crawl.data(), &t) == VP_OK && t && g_launches == 11);   // (still cached)
    G.d_ray.release();
    G.d_tiles.p = nullptr; G.d_tiles.bytes = 0;
    CHECK(g_live == 0);
    printf("ray table host code: key, grow and fall-back hold (%d builds)\n", g_launches);
    return 0;
}
