/* cli_trace_stub.c -- a stand-in libvolpath_hip.so for scripts/cli_trace.py: every symbol that host/main.cpp and host/multigpu.cpp
 * import from the real library, on the host, with no GPU.  Each call appends one line to the file named by CLI_TRACE_LOG: its name,
 * its scalar arguments as they are, array arguments by value, "device" pointers as d<ordinal of the vp_malloc that made them>.
 * vp_malloc is malloc, the memory filled with 0x5a (a missing vp_memset shows).  Every call that writes a buffer fills it with values
 * derived from a hash of its own name, its arguments and the CONTENTS of the buffers it reads, so the files volpath_render writes are
 * deterministic and differ when the calls, their order or their operands differ.  vp_download copies.  Nothing here computes an image. */
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "volpath.h"

typedef struct { char* base; size_t bytes; } Alloc;
static Alloc    g_alloc[4096];
static int      g_nalloc, g_nctx, g_subpixel = 1;
static uint64_t g_h; /* the hash of the call being made */

static void say(const char* fmt, ...)
{
    static FILE* f;
    if (!f)
    {
        const char* name = getenv("CLI_TRACE_LOG");
        f = name ? fopen(name, "a") : stderr;
        if (!f) exit(97);
    }
    va_list ap;
    va_start(ap, fmt);
    vfprintf(f, fmt, ap);
    va_end(ap);
    fflush(f);
}
static void mix(uint64_t v)
{
    g_h = (g_h ^ v) * 0x100000001b3ull;
    g_h ^= g_h >> 29;
}
static void mix_bytes(const void* p, size_t bytes)
{
    const unsigned char* b = (const unsigned char*)p;
    for (size_t i = 0; i < bytes; i++) mix(b[i]);
}
static const Alloc* owner(const void* p)
{
    for (int i = 0; i < g_nalloc; i++)
        if ((const char*)p >= g_alloc[i].base && (const char*)p < g_alloc[i].base + g_alloc[i].bytes) return &g_alloc[i];
    return NULL;
}
/* a pointer argument: its label goes to the log, what it points to (a whole device buffer) into the hash */
static void ptr(const void* p)
{
    const Alloc* a = owner(p);
    if (!p) say(" null");
    else if (a) say(" d%d", (int)(a - g_alloc));
    else say(" host");
    if (a) mix_bytes(a->base, a->bytes);
    mix(p ? 1 : 0);
}
static void begin(const char* name)
{
    g_h = 0xcbf29ce484222325ull;
    mix_bytes(name, strlen(name));
    say("%s", name);
}
static void i64(long long v) { say(" %lld", v); mix((uint64_t)v); }
static void flt(const float* v, int n)
{
    say(" [");
    for (int i = 0; i < n; i++) say(i ? " %.9g" : "%.9g", v[i]);
    say("]");
    mix_bytes(v, (size_t)n * sizeof(float));
}
static void param(const Param* p)
{
    say(" P{%u %u", p->width, p->height);
    flt(&p->density, 9);
    say("}");
    mix(p->width), mix(p->height);
}
static int done(void) { say("\n"); return 0; }
static uint64_t word(uint64_t i)
{
    uint64_t x = g_h + i * 0x9e3779b97f4a7c15ull;
    x ^= x >> 31, x *= 0xbf58476d1ce4e5b9ull, x ^= x >> 27;
    return x;
}
/* fill a whole destination buffer from the call's hash: floats in [0, 1) (images and maps), or bytes (records) */
static void fill_floats(void* dst)
{
    const Alloc* a = owner(dst);
    if (!a) return;
    float* f = (float*)a->base;
    for (size_t i = 0; i < a->bytes / sizeof(float); i++) f[i] = (float)(word(i) >> 40) * (1.0f / 16777216.0f);
}
static void fill_bytes(void* dst)
{
    const Alloc* a = owner(dst);
    for (size_t i = 0; a && i < a->bytes; i++) a->base[i] = (char)(word(i ^ 0x5555) >> 33);
}
static void result(vp_adaptive_result* r)
{
    r->samples = word(1) % 1000, r->rounds = (uint32_t)(word(2) % 10), r->active_left = (uint32_t)(word(3) % 100), r->frames_used = (uint32_t)(word(4) % 50);
}

/* ---- Part 1 */
void init_cuda(void* v, vp_extent e, bool quantized, const vp_float3* bmin, const vp_float3* bmax)
{
    begin("init_cuda"), i64((long long)e.width), i64((long long)e.height), i64((long long)e.depth), i64(quantized), flt(&bmin->x, 3), flt(&bmax->x, 3);
    mix_bytes(v, e.width * e.height * e.depth * (quantized ? 1 : 4));
    say(" volume %016llx", (unsigned long long)g_h), done();
}
void set_texture_filter_mode(bool linear) { begin("set_texture_filter_mode"), i64(linear), done(); }
void free_cuda_buffers(void) { begin("free_cuda_buffers"), done(); }
void precompute_opacity(const float* d) { begin("precompute_opacity"), flt(d, 3), done(); }
void init_envmap(const vp_float4* map, int w, int h)
{
    begin("init_envmap"), i64(w), i64(h), mix_bytes(map, (size_t)w * h * sizeof(vp_float4));
    say(" map %016llx", (unsigned long long)g_h), done();
}
void free_envmap(void) { begin("free_envmap"), done(); }
void set_sun(float* d, float* p) { begin("set_sun"), flt(d, 3), flt(p, 3), done(); }
void copy_inv_view_matrix(float* m, size_t bytes) { begin("copy_inv_view_matrix"), flt(m, 12), i64((long long)bytes), done(); }
void copy_inv_model_matrix(float* m, size_t bytes) { begin("copy_inv_model_matrix"), flt(m, 12), i64((long long)bytes), done(); }
void render_kernel(vp_dim3 g, vp_dim3 b, vp_float4* out, int spp, const Param* p)
{
    begin("render_kernel"), i64(g.x), i64(g.y), i64(g.z), i64(b.x), i64(b.y), i64(b.z), ptr(out), i64(spp), param(p), fill_floats(out), done();
}
void scale(vp_float4* dst, vp_float4* src, int n, float s) { begin("scale"), ptr(dst), ptr(src), i64(n), flt(&s, 1), fill_floats(dst), done(); }
void gamma_correct(vp_float4* dst, vp_float4* src, int n, float s, float g)
{
    begin("gamma_correct"), ptr(dst), ptr(src), i64(n), flt(&s, 1), flt(&g, 1), fill_floats(dst), done();
}

/* ---- contexts, memory, setters */
const char* vp_last_error(void) { return "cli_trace_stub: no error"; }
int vp_set_device(int d) { return begin("vp_set_device"), i64(d), done(); }
vp_ctx* vp_ctx_create(int d)
{
    begin("vp_ctx_create"), i64(d), say(" -> c%d", ++g_nctx), done();
    return (vp_ctx*)(size_t)g_nctx;
}
int vp_ctx_destroy(vp_ctx* c) { return begin("vp_ctx_destroy"), say(" c%d", (int)(size_t)c), done(); }
int vp_ctx_set_current(vp_ctx* c) { return begin("vp_ctx_set_current"), say(" c%d", (int)(size_t)c), done(); }
void* vp_get_stream(void) { begin("vp_get_stream"), done(); return NULL; }
int vp_synchronize(void) { return begin("vp_synchronize"), done(); }
void* vp_malloc(size_t bytes)
{
    if (g_nalloc == 4096 || !bytes) exit(98);
    Alloc* a = &g_alloc[g_nalloc++];
    a->base = (char*)malloc(bytes), a->bytes = bytes;
    memset(a->base, 0x5a, bytes);
    begin("vp_malloc"), i64((long long)bytes), say(" -> d%d", g_nalloc - 1), done();
    return a->base;
}
int vp_free(void* p) { return begin("vp_free"), ptr(p), done(); }   /* kept: ordinals stay unique, a use after free still has a label */
int vp_memset(void* p, int v, size_t bytes) { begin("vp_memset"), ptr(p), i64(v), i64((long long)bytes), memset(p, v, bytes); return done(); }
int vp_download(void* dst, const void* src, size_t bytes) { begin("vp_download"), ptr(src), i64((long long)bytes), memcpy(dst, src, bytes); return done(); }
int vp_accumulate(vp_float4* dst, const vp_float4* src, size_t n) { return begin("vp_accumulate"), ptr(dst), ptr(src), i64((long long)n), fill_floats(dst), done(); }
int vp_julia_voxelize(int n, unsigned char* out)
{
    begin("vp_julia_voxelize"), i64(n);
    for (size_t i = 0; i < (size_t)n * n * n; i++) out[i] = (unsigned char)(word(i) >> 56);
    return done();
}
int vp_init_volume(const void* v, vp_extent e, int format, const vp_float3* bmin, const vp_float3* bmax)
{
    begin("vp_init_volume"), i64((long long)e.width), i64((long long)e.height), i64((long long)e.depth), i64(format), flt(&bmin->x, 3), flt(&bmax->x, 3);
    mix_bytes(v, e.width * e.height * e.depth * (format == VP_VOL_U8 ? 1 : format == VP_VOL_F32 ? 4 : 2));
    return say(" volume %016llx", (unsigned long long)g_h), done();
}
#define SETTER1(name) int name(int a) { return begin(#name), i64(a), done(); }
SETTER1(vp_set_estimator) SETTER1(vp_set_tracking) SETTER1(vp_set_envmap_sampling) SETTER1(vp_set_arithmetic) SETTER1(vp_set_bound_brick)
int vp_set_subpixel(int s) { g_subpixel = s; return begin("vp_set_subpixel"), i64(s), done(); }
int vp_get_subpixel(void) { return begin("vp_get_subpixel"), say(" -> %d", g_subpixel), done(), g_subpixel; }
int vp_set_rng(int mode, uint32_t k0, uint32_t k1) { return begin("vp_set_rng"), i64(mode), i64(k0), i64(k1), done(); }
int vp_set_shard(int r, int w) { return begin("vp_set_shard"), i64(r), i64(w), done(); }
int vp_render_time_ms(double* ms, int* launches, int reset)
{
    begin("vp_render_time_ms"), i64(ms != NULL), i64(launches != NULL), i64(reset);
    if (ms) *ms = 1.5;
    if (launches) *launches = 1;
    return done();
}

/* ---- renders: accumulators gain floats, records bytes; every buffer read is part of the hash, the written ones included (they accumulate) */
#define TAIL int first, int n, const Param* p
#define FRAMES i64(first), i64(n), param(p)
int vp_render_frames(vp_float4* a, TAIL) { return begin("vp_render_frames"), ptr(a), FRAMES, fill_floats(a), done(); }
int vp_render_frames_stats(vp_float4* a, vp_pixel_stats* r, TAIL) { return begin("vp_render_frames_stats"), ptr(a), ptr(r), FRAMES, fill_floats(a), fill_bytes(r), done(); }
#define PLANES2(name)                                                                                                        \
    int name(vp_float4* a, vp_float4* b, TAIL) { return begin(#name), ptr(a), ptr(b), FRAMES, fill_floats(a), mix(7), fill_floats(b), done(); } \
    int name##_stats(vp_float4* a, vp_float4* b, vp_pixel_stats* r, vp_pixel_stats* s, TAIL)                                 \
    {                                                                                                                        \
        begin(#name "_stats"), ptr(a), ptr(b), ptr(r), ptr(s), FRAMES;                                                       \
        return fill_floats(a), mix(7), fill_floats(b), mix(7), fill_bytes(r), mix(7), fill_bytes(s), done();                  \
    }
PLANES2(vp_render_frames_layers) PLANES2(vp_render_frames_groups)
int vp_render_frames_halves_stats(vp_float4* a, vp_float4* b, vp_pixel_stats* r, vp_pixel_stats* s, TAIL)
{
    begin("vp_render_frames_halves_stats"), ptr(a), ptr(b), ptr(r), ptr(s), FRAMES;
    return fill_floats(a), mix(7), fill_floats(b), mix(7), fill_bytes(r), mix(7), fill_bytes(s), done();
}
int vp_render_frames_group_layers(vp_float4* a, vp_float4* b, vp_float4* c, TAIL)
{
    return begin("vp_render_frames_group_layers"), ptr(a), ptr(b), ptr(c), FRAMES, fill_floats(a), mix(7), fill_floats(b), mix(7), fill_floats(c), done();
}
static void three(const char* name, vp_float4* a, vp_float4* b, vp_float4* c, vp_pixel_stats* r, vp_pixel_stats* s, vp_pixel_stats* t, TAIL)
{
    begin(name), ptr(a), ptr(b), ptr(c), ptr(r), ptr(s), ptr(t), FRAMES;
}
static void fill_three(vp_float4* a, vp_float4* b, vp_float4* c, vp_pixel_stats* r, vp_pixel_stats* s, vp_pixel_stats* t)
{
    fill_floats(a), mix(7), fill_floats(b), mix(7), fill_floats(c), mix(7), fill_bytes(r), mix(7), fill_bytes(s), mix(7), fill_bytes(t);
}
int vp_render_frames_group_layers_stats(vp_float4* a, vp_float4* b, vp_float4* c, vp_pixel_stats* r, vp_pixel_stats* s, vp_pixel_stats* t, TAIL)
{
    return three("vp_render_frames_group_layers_stats", a, b, c, r, s, t, first, n, p), fill_three(a, b, c, r, s, t), done();
}
int vp_render_adaptive(vp_float4* a, vp_pixel_stats* r, TAIL, const vp_adaptive* ad, vp_adaptive_result* res)
{
    begin("vp_render_adaptive"), ptr(a), ptr(r), FRAMES, flt(&ad->rel_tol, 2), i64(ad->min_frames), i64(ad->round_frames);
    return fill_floats(a), fill_bytes(r), result(res), done();
}
#define ADAPTIVE2(name)                                                                                                                      \
    int name(vp_float4* a, vp_float4* b, vp_pixel_stats* r, vp_pixel_stats* s, TAIL, const vp_adaptive_planes* ad, vp_adaptive_result* res) \
    {                                                                                                                                        \
        begin(#name), ptr(a), ptr(b), ptr(r), ptr(s), FRAMES, flt(ad->rel_tol, 4), i64(ad->min_frames), i64(ad->round_frames);               \
        return fill_floats(a), mix(7), fill_floats(b), mix(7), fill_bytes(r), mix(7), fill_bytes(s), result(res), done();                     \
    }
ADAPTIVE2(vp_render_adaptive_groups) ADAPTIVE2(vp_render_adaptive_layers)
int vp_render_adaptive_group_layers(vp_float4* a, vp_float4* b, vp_float4* c, vp_pixel_stats* r, vp_pixel_stats* s, vp_pixel_stats* t, TAIL,
                                    const vp_adaptive_planes3* ad, vp_adaptive_result* res)
{
    three("vp_render_adaptive_group_layers", a, b, c, r, s, t, first, n, p);
    return flt(ad->rel_tol, 6), i64(ad->min_frames), i64(ad->round_frames), fill_three(a, b, c, r, s, t), result(res), done();
}
/* planes in two halves: every used entry of the two vp_plane_bufs, accumulators then records, half 0 then half 1 */
static void halves_args(const char* name, int mode, const vp_plane_bufs* h0, const vp_plane_bufs* h1, TAIL)
{
    const int np = mode == VP_PLANES_GROUP_LAYERS ? 3 : 2;
    begin(name), i64(mode);
    for (int h = 0; h < 2; h++)
        for (int k = 0; k < np; k++) ptr((h ? h1 : h0)->acc[k]), ptr((h ? h1 : h0)->rec[k]);
    FRAMES;
}
static void fill_halves(int mode, const vp_plane_bufs* h0, const vp_plane_bufs* h1)
{
    const int np = mode == VP_PLANES_GROUP_LAYERS ? 3 : 2;
    for (int h = 0; h < 2; h++)
        for (int k = 0; k < np; k++) fill_floats((h ? h1 : h0)->acc[k]), mix(7), fill_bytes((h ? h1 : h0)->rec[k]), mix(7);
}
int vp_render_frames_planes_halves_stats(int mode, const vp_plane_bufs* h0, const vp_plane_bufs* h1, TAIL)
{
    return halves_args("vp_render_frames_planes_halves_stats", mode, h0, h1, first, n, p), fill_halves(mode, h0, h1), done();
}
int vp_render_adaptive_planes_halves(int mode, const vp_plane_bufs* h0, const vp_plane_bufs* h1, TAIL, const vp_adaptive_planes3* ad, vp_adaptive_result* res)
{
    halves_args("vp_render_adaptive_planes_halves", mode, h0, h1, first, n, p);
    return flt(ad->rel_tol, 6), i64(ad->min_frames), i64(ad->round_frames), fill_halves(mode, h0, h1), result(res), done();
}
int vp_render_adaptive_halves(vp_float4* a, vp_float4* b, vp_pixel_stats* r, vp_pixel_stats* s, TAIL, const vp_adaptive* ad, vp_adaptive_result* res)
{
    begin("vp_render_adaptive_halves"), ptr(a), ptr(b), ptr(r), ptr(s), FRAMES, flt(&ad->rel_tol, 2), i64(ad->min_frames), i64(ad->round_frames);
    return fill_floats(a), mix(7), fill_floats(b), mix(7), fill_bytes(r), mix(7), fill_bytes(s), result(res), done();
}
int vp_render_features(vp_float4* alpha, vp_float4* depth, const Param* p, const vp_feature_params* fp)
{
    begin("vp_render_features"), ptr(alpha), ptr(depth), param(p), flt(&fp->step, 2), fill_floats(alpha), mix(7), fill_floats(depth);
    const Alloc* a = owner(depth);
    for (size_t i = 0; a && i < a->bytes / sizeof(float); i += 7) ((float*)a->base)[i] = INFINITY;   /* depths that do not exist */
    return done();
}

/* ---- the output stage */
int vp_scale_by_count(vp_float4* dst, const vp_float4* src, const vp_pixel_stats* r, int n, float s)
{
    return begin("vp_scale_by_count"), ptr(dst), ptr(src), ptr(r), i64(n), flt(&s, 1), fill_floats(dst), done();
}
int vp_accumulate_stats(vp_pixel_stats* dst, const vp_pixel_stats* src, size_t n)
{
    return begin("vp_accumulate_stats"), ptr(dst), ptr(src), i64((long long)n), fill_bytes(dst), done();
}
int vp_stats_rel_error(float* dst, const vp_pixel_stats* r, int n, float floor_y)
{
    return begin("vp_stats_rel_error"), ptr(dst), ptr(r), i64(n), flt(&floor_y, 1), fill_floats(dst), done();
}
int vp_denoise(vp_float4* dst, const vp_float4* src, const vp_pixel_stats* r, const vp_float4* g, const vp_pixel_stats* gr, int w, int h, const vp_denoise_params* dp)
{
    return begin("vp_denoise"), ptr(dst), ptr(src), ptr(r), ptr(g), ptr(gr), i64(w), i64(h), i64(dp->radius), i64(dp->patch), flt(&dp->k, 1), fill_floats(dst), done();
}
int vp_denoise_guided(vp_float4* dst, const vp_float4* src, const vp_pixel_stats* r, const vp_float4* g, const vp_pixel_stats* gr, const vp_denoise_feature* f, int nf,
                      int w, int h, const vp_denoise_params* dp)
{
    begin("vp_denoise_guided"), ptr(dst), ptr(src), ptr(r), ptr(g), ptr(gr), i64(f != NULL), i64(nf);
    for (int k = 0; k < nf; k++) say(" {"), ptr(f[k].plane), i64(f[k].channel), flt(&f[k].sigma, 1), say(" }");
    return i64(w), i64(h), i64(dp->radius), i64(dp->patch), flt(&dp->k, 1), fill_floats(dst), done();
}
int vp_merge_halves(vp_float4* dst, float* resid, const vp_float4* a, const vp_pixel_stats* ar, const vp_float4* b, const vp_pixel_stats* br, int n, float floor_y)
{
    return begin("vp_merge_halves"), ptr(dst), ptr(resid), ptr(a), ptr(ar), ptr(b), ptr(br), i64(n), flt(&floor_y, 1), fill_floats(dst), mix(7), fill_floats(resid), done();
}
int vp_halves_variance(float* u, float* q, const vp_pixel_stats* ar, const vp_pixel_stats* br, int n)
{
    return begin("vp_halves_variance"), ptr(u), ptr(q), ptr(ar), ptr(br), i64(n), fill_floats(u), mix(7), fill_floats(q), done();
}
int vp_filter_variance(float* dst, const float* u, const float* q, int w, int h, const vp_denoise_params* dp)
{
    return begin("vp_filter_variance"), ptr(dst), ptr(u), ptr(q), i64(w), i64(h), i64(dp->radius), i64(dp->patch), flt(&dp->k, 1), fill_floats(dst), done();
}
int vp_denoise_var(vp_float4* dst, const vp_float4* src, const vp_pixel_stats* r, const vp_float4* g, const vp_pixel_stats* gr, const float* var,
                   const vp_denoise_feature* f, int nf, int w, int h, const vp_denoise_params* dp)
{
    begin("vp_denoise_var"), ptr(dst), ptr(src), ptr(r), ptr(g), ptr(gr), ptr(var), i64(f != NULL), i64(nf);
    for (int k = 0; k < nf; k++) say(" {"), ptr(f[k].plane), i64(f[k].channel), flt(&f[k].sigma, 1), say(" }");
    return i64(w), i64(h), i64(dp->radius), i64(dp->patch), flt(&dp->k, 1), fill_floats(dst), done();
}
int vp_cross_error(float* err, const vp_float4* fa, const vp_float4* fb, const vp_float4* h0, const vp_pixel_stats* s0, const vp_float4* h1, const vp_pixel_stats* s1, int n)
{
    return begin("vp_cross_error"), ptr(err), ptr(fa), ptr(fb), ptr(h0), ptr(s0), ptr(h1), ptr(s1), i64(n), fill_floats(err), done();
}
int vp_select(vp_float4* dst, uint8_t* index, const vp_float4* const* images, const float* const* errors, int n, int w, int h, const vp_select_params* sp)
{
    begin("vp_select"), ptr(dst), ptr(index), i64(n);
    for (int k = 0; k < n; k++) say(" {"), ptr(images[k]), ptr(errors[k]), say(" }");
    return i64(w), i64(h), i64(sp->smooth_radius), i64(sp->blend_radius), fill_floats(dst), done();
}
int vp_composite(vp_float4* dst, const vp_float4* fg, const vp_float4* trans, const vp_float4* plate, const float rgb[3], int n, float s)
{
    return begin("vp_composite"), ptr(dst), ptr(fg), ptr(trans), ptr(plate), flt(rgb, 3), i64(n), flt(&s, 1), fill_floats(dst), done();
}
int vp_relight(vp_float4* dst, const vp_float4* sun, const vp_float4* sky, const float gs[3], const float gk[3], int n, float s)
{
    return begin("vp_relight"), ptr(dst), ptr(sun), ptr(sky), flt(gs, 3), flt(gk, 3), i64(n), flt(&s, 1), fill_floats(dst), done();
}
int vp_relight_composite(vp_float4* dst, const vp_float4* sun, const vp_float4* sky, const vp_float4* trans, const float gs[3], const float gk[3], const vp_float4* plate,
                         const float rgb[3], int n, float s)
{
    return begin("vp_relight_composite"), ptr(dst), ptr(sun), ptr(sky), ptr(trans), flt(gs, 3), flt(gk, 3), ptr(plate), flt(rgb, 3), i64(n), flt(&s, 1), fill_floats(dst), done();
}
