// vp_denoise.hip -- the variance-guided NL-means filter of the output stage (include/volpath.h vp_denoise).
//
// Both kernels compute the definition of the header to the bit: binary32, no contraction, the patch distance as row sums left to
// right and their sum top to bottom, the weights summed over the offsets in raster order, expf_ in the exact arithmetic (this file
// is compiled without VP_ARITH_FAST, like the output stage of vp_kernels.hip).
//   denoise_tiled_k (form 0): one 256-thread workgroup per 32 x 8 pixel tile.  (y, v) of the tile plus an R + F halo and the mean
//     colours of the tile plus an R halo are staged in LDS once, fetched with clamped coordinates; per offset the pair terms e of the
//     tile's F-halo plane are computed once each into LDS (2.1 per thread at F = 3 instead of 49) and every thread sums its patch
//     from there.  The plane is double buffered: one barrier per offset.
//   denoise_plain_k (form 1): one thread per pixel, straight from global memory, looping over the definition.  The cross-check.
//   denoise_guided_tiled_k / denoise_guided_plain_k: the two forms of vp_denoise_guided, kernels of their
//     own so that the two above stay as they are: the same passes, plus NF feature channels staged once into LDS planes shaped like
//     the colour planes and a per-pixel-pair feature distance that caps the weight.
//   vp_denoise_var's instances of these four: a trailing parameter pack V that is empty or one `const float*`, the caller's per-sample
//     variance plane; v is then plane[a] * s_a in place of the records' variance, everything else as it stands.  An empty pack leaves
//     the parameter list -- and with it the instructions -- of the instances above as they were (profiles/variance_kernel_resources.txt).
//   variance_tiled_k / variance_plain_k: the two forms of vp_filter_variance, the same passes on one scalar
//     plane u with its noise q: two staged planes with an R + F halo, the e planes, no colour planes -- u with its R halo is inside
//     the staged plane.
//   select_tiled_k / select_plain_k: the two forms of vp_select: box sums of n error planes, the smallest
//     picked per pixel, the picks blended over a window; nothing of the filter above is shared but the tile.
// LDS layout (cdna_hip_programming.md section 2: ds_read_b32 / ds_write_b32 bank = dword address mod 32 within a 32-lane half):
// every plane is one float per element, structure of arrays, and a half-wave is one tile row, so the patch reads and the colour
// reads of a half-wave are 32 consecutive dwords whatever the pitch.  The fill of the e plane walks it linearly, so a half-wave can
// straddle two of its rows; the pitch of the (y, v) planes is the e plane's plus 32, which makes the dword addresses of such a
// half-wave consecutive mod 32 again.
#include <hip/hip_runtime.h>

#include "vp_kernels.h"
#include "vp_math.h"

namespace vp
{
namespace
{
constexpr int DN_TX = 32, DN_TY = 8;   // the tile: a half-wave per row
constexpr float DN_EPS = 1e-20f;

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }
// s = 1 / n (0 where n == 0) and the mean colour A.xyz * s: the bits of scale_by_count_k with scale 1.0f
__device__ __forceinline__ float inv_count(unsigned n) { return n ? 1.0f / (float)n : 0.0f; }
__device__ __forceinline__ float luminance(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }
// variance of the mean luminance, binary64, rounded once
__device__ __forceinline__ float mean_variance(const PixelStatsDev& T)
{
    if (T.n < 2u) return 0.0f;
    const double nd  = (double)T.n;
    const double lhs = nd * T.sum_y2 - T.sum_y * T.sum_y;
    return (float)((lhs > 0.0 ? lhs : 0.0) / (nd * nd * (nd - 1.0)));
}
// the variance of the guide's mean at pixel i: from its records, or (vp_denoise_var) the caller's per-sample variance times s = 1 / n.
// V is the kernels' trailing pack: nothing, or the one plane -- `(svar[i], ...)` is then that plane's element
template <class... V>
__device__ __forceinline__ float guide_variance(const PixelStatsDev& T, float s, int i, V... svar)
{
    if constexpr (sizeof...(V) != 0) return (svar[i], ...) * s;
    else return mean_variance(T);
}
template <class... V>
__device__ __forceinline__ float guide_variance_at(const PixelStatsDev* stats, int i, V... svar)
{
    if constexpr (sizeof...(V) != 0) return (svar[i], ...) * inv_count(stats[i].n);
    else return mean_variance(stats[i]);
}
// (y, v) of the pair (accumulator, records) at pixel i
template <class... V>
__device__ __forceinline__ void guide_yv(const float4* acc, const PixelStatsDev* stats, int i, float& y, float& v, V... svar)
{
    const PixelStatsDev T = stats[i];
    const float4 A = acc[i];
    const float  s = inv_count(T.n);
    y = luminance(A.x * s, A.y * s, A.z * s);
    v = guide_variance(T, s, i, svar...);
}
__device__ __forceinline__ float pair_term(float ya, float va, float yb, float vb, float k2)
{
    const float d = ya - yb;
    return (d * d - (va + (vb < va ? vb : va))) / (DN_EPS + k2 * (va + vb));
}
__device__ __forceinline__ float patch_weight(float D, float inv_area)
{
    D = D * inv_area;
    D = D > 0.0f ? D : 0.0f;
    return expf_(-D);
}

template <int F, class... V>
__global__ __launch_bounds__(DN_TX * DN_TY) void denoise_tiled_k(float4* dst, const float4* src, const PixelStatsDev* stats, const float4* guide,
                                                                  const PixelStatsDev* gstats, int W, int H, int R, float k2, V... svar)
{
    constexpr int EW = DN_TX + 2 * F, EH = DN_TY + 2 * F;   // the e plane: the tile plus an F halo
    constexpr int YW = EW + 32;                             // pitch of the (y, v) planes (>= DN_TX + 2 (R + F) for R <= 16)
    extern __shared__ float lds[];
    const int YH = DN_TY + 2 * (R + F), CW = DN_TX + 2 * R, CH = DN_TY + 2 * R;
    float* Ly = lds;
    float* Lv = Ly + YW * YH;
    float* Lc = Lv + YW * YH;             // three planes of CW * CH
    float* Le = Lc + 3 * CW * CH;         // two planes of EW * EH
    const int tid = threadIdx.x, tx = tid & (DN_TX - 1), ty = tid / DN_TX;
    const int x0 = blockIdx.x * DN_TX, y0 = blockIdx.y * DN_TY;
    const int px = x0 + tx, py = y0 + ty;
    const bool inside = px < W && py < H;
    const int  pi = clampi(py, H - 1) * W + clampi(px, W - 1);
    // the thread's own pixel: mean colour, heat and the guide's variance
    const float4 A  = src[pi];
    const float  sp = inv_count(stats[pi].n);
    const float  vme = guide_variance_at(gstats, pi, svar...);
    float4 out = make_float4(A.x * sp, A.y * sp, A.z * sp, A.w * sp);
    // a tile without a noisy pixel (the per-pixel-constant classes) is the plain output stage
    if (!__syncthreads_or(inside && vme != 0.0f))
    {
        if (inside) dst[pi] = out;
        return;
    }
    const int halo = R + F;
    for (int i = tid; i < (DN_TX + 2 * halo) * YH; i += DN_TX * DN_TY)
    {
        const int r = i / (DN_TX + 2 * halo), c = i - r * (DN_TX + 2 * halo);
        float y, v;
        guide_yv(guide, gstats, clampi(y0 - halo + r, H - 1) * W + clampi(x0 - halo + c, W - 1), y, v, svar...);
        Ly[r * YW + c] = y;
        Lv[r * YW + c] = v;
    }
    for (int i = tid; i < CW * CH; i += DN_TX * DN_TY)
    {
        const int r = i / CW, c = i - r * CW;
        const int g = clampi(y0 - R + r, H - 1) * W + clampi(x0 - R + c, W - 1);
        const float4 B = src[g];
        const float  s = inv_count(stats[g].n);
        Lc[i] = B.x * s;
        Lc[CW * CH + i] = B.y * s;
        Lc[2 * CW * CH + i] = B.z * s;
    }
    __syncthreads();
    const bool  filtered = inside && vme != 0.0f;
    const float inv_area = 1.0f / (float)((2 * F + 1) * (2 * F + 1));
    float den = 0.0f, nr = 0.0f, ng = 0.0f, nb = 0.0f;
    int buf = 0;
    for (int oy = -R; oy <= R; oy++)
        for (int ox = -R; ox <= R; ox++, buf ^= 1)
        {
            float* E = Le + buf * (EW * EH);
            const int shift = oy * YW + ox;
            for (int i = tid; i < EW * EH; i += DN_TX * DN_TY)
            {
                const int r = i / EW, c = i - r * EW;
                const int a = (r + R) * YW + (c + R);
                E[i] = pair_term(Ly[a], Lv[a], Ly[a + shift], Lv[a + shift], k2);
            }
            __syncthreads();   // (the other buffer is written next: its readers passed this barrier)
            const int qx = px + ox, qy = py + oy;
            if (filtered && qx >= 0 && qx < W && qy >= 0 && qy < H)
            {
                float D = 0.0f;
#pragma unroll
                for (int dy = 0; dy <= 2 * F; dy++)
                {
                    float row = 0.0f;
#pragma unroll
                    for (int dx = 0; dx <= 2 * F; dx++) row = row + E[(ty + dy) * EW + tx + dx];
                    D = D + row;
                }
                const float w = patch_weight(D, inv_area);
                const int   ci = (ty + R + oy) * CW + tx + R + ox;
                den = den + w;
                nr  = nr + w * Lc[ci];
                ng  = ng + w * Lc[CW * CH + ci];
                nb  = nb + w * Lc[2 * CW * CH + ci];
            }
        }
    if (filtered) { out.x = nr / den; out.y = ng / den; out.z = nb / den; }
    if (inside) dst[pi] = out;
}

template <class... V>
__global__ __launch_bounds__(256) void denoise_plain_k(float4* dst, const float4* src, const PixelStatsDev* stats, const float4* guide,
                                                       const PixelStatsDev* gstats, int W, int H, int R, int F, float k2, V... svar)
{
    const int idx = threadIdx.x + blockIdx.x * blockDim.x;
    if (idx >= W * H) return;
    const int py = idx / W, px = idx - py * W;
    const float4 A  = src[idx];
    const float  sp = inv_count(stats[idx].n);
    float4 out = make_float4(A.x * sp, A.y * sp, A.z * sp, A.w * sp);
    if (guide_variance_at(gstats, idx, svar...) != 0.0f)
    {
        const float inv_area = 1.0f / (float)((2 * F + 1) * (2 * F + 1));
        float den = 0.0f, nr = 0.0f, ng = 0.0f, nb = 0.0f;
        for (int oy = -R; oy <= R; oy++)
            for (int ox = -R; ox <= R; ox++)
            {
                const int qx = px + ox, qy = py + oy;
                if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                float D = 0.0f;
                for (int dy = -F; dy <= F; dy++)
                {
                    float row = 0.0f;
                    for (int dx = -F; dx <= F; dx++)
                    {
                        float ya, va, yb, vb;
                        guide_yv(guide, gstats, clampi(py + dy, H - 1) * W + clampi(px + dx, W - 1), ya, va, svar...);
                        guide_yv(guide, gstats, clampi(qy + dy, H - 1) * W + clampi(qx + dx, W - 1), yb, vb, svar...);
                        row = row + pair_term(ya, va, yb, vb, k2);
                    }
                    D = D + row;
                }
                const float  w = patch_weight(D, inv_area);
                const int    q = qy * W + qx;
                const float4 B = src[q];
                const float  s = inv_count(stats[q].n);
                den = den + w;
                nr  = nr + w * (B.x * s);
                ng  = ng + w * (B.y * s);
                nb  = nb + w * (B.z * s);
            }
        out.x = nr / den; out.y = ng / den; out.z = nb / den;
    }
    dst[idx] = out;
}

// ---- vp_denoise_guided: the same filter with the weight of an offset cut by a distance of noise-free features
// the patch distance as patch_weight scales and clamps it, before the exponential
__device__ __forceinline__ float patch_distance(float D, float inv_area)
{
    D = D * inv_area;
    return D > 0.0f ? D : 0.0f;
}
// t_j of the header: equal values -- two equal infinities among them -- agree exactly
__device__ __forceinline__ float feature_term(float fa, float fb, float g)
{
    const float d = fa - fb;
    return fa == fb ? 0.0f : (d * d) * g;
}
__device__ __forceinline__ float guided_weight(float D, float Df) { return expf_(-(Df > D ? Df : D)); }

// denoise_tiled_k with NF feature planes of the tile plus an R halo behind the e planes, pitch and indexing of the colour planes:
// fb of a half-wave is 32 consecutive dwords, fa stays in registers, no barrier more than denoise_tiled_k has
template <int F, int NF, class... V>
__global__ __launch_bounds__(DN_TX * DN_TY) void denoise_guided_tiled_k(float4* dst, const float4* src, const PixelStatsDev* stats, const float4* guide,
                                                                         const PixelStatsDev* gstats, DenoiseFeaturesDev feat, int W, int H, int R, float k2,
                                                                         V... svar)
{
    constexpr int EW = DN_TX + 2 * F, EH = DN_TY + 2 * F;
    constexpr int YW = EW + 32;
    extern __shared__ float lds[];
    const int YH = DN_TY + 2 * (R + F), CW = DN_TX + 2 * R, CH = DN_TY + 2 * R;
    float* Ly = lds;
    float* Lv = Ly + YW * YH;
    float* Lc = Lv + YW * YH;             // three planes of CW * CH
    float* Le = Lc + 3 * CW * CH;         // two planes of EW * EH
    float* Lf = Le + 2 * EW * EH;         // NF planes of CW * CH
    const int tid = threadIdx.x, tx = tid & (DN_TX - 1), ty = tid / DN_TX;
    const int x0 = blockIdx.x * DN_TX, y0 = blockIdx.y * DN_TY;
    const int px = x0 + tx, py = y0 + ty;
    const bool inside = px < W && py < H;
    const int  pi = clampi(py, H - 1) * W + clampi(px, W - 1);
    const float4 A  = src[pi];
    const float  sp = inv_count(stats[pi].n);
    const float  vme = guide_variance_at(gstats, pi, svar...);
    float4 out = make_float4(A.x * sp, A.y * sp, A.z * sp, A.w * sp);
    if (!__syncthreads_or(inside && vme != 0.0f))
    {
        if (inside) dst[pi] = out;
        return;
    }
    const int halo = R + F;
    for (int i = tid; i < (DN_TX + 2 * halo) * YH; i += DN_TX * DN_TY)
    {
        const int r = i / (DN_TX + 2 * halo), c = i - r * (DN_TX + 2 * halo);
        float y, v;
        guide_yv(guide, gstats, clampi(y0 - halo + r, H - 1) * W + clampi(x0 - halo + c, W - 1), y, v, svar...);
        Ly[r * YW + c] = y;
        Lv[r * YW + c] = v;
    }
    for (int i = tid; i < CW * CH; i += DN_TX * DN_TY)
    {
        const int r = i / CW, c = i - r * CW;
        const int g = clampi(y0 - R + r, H - 1) * W + clampi(x0 - R + c, W - 1);
        const float4 B = src[g];
        const float  s = inv_count(stats[g].n);
        Lc[i] = B.x * s;
        Lc[CW * CH + i] = B.y * s;
        Lc[2 * CW * CH + i] = B.z * s;
        // (a clamped position's feature is staged but never read: offsets that leave the image are skipped)
#pragma unroll
        for (int j = 0; j < NF; j++) Lf[j * (CW * CH) + i] = feat.chan[j][4 * (size_t)g];
    }
    __syncthreads();
    const bool  filtered = inside && vme != 0.0f;
    const float inv_area = 1.0f / (float)((2 * F + 1) * (2 * F + 1));
    float fa[NF];
#pragma unroll
    for (int j = 0; j < NF; j++) fa[j] = Lf[j * (CW * CH) + (ty + R) * CW + tx + R];
    float den = 0.0f, nr = 0.0f, ng = 0.0f, nb = 0.0f;
    int buf = 0;
    for (int oy = -R; oy <= R; oy++)
        for (int ox = -R; ox <= R; ox++, buf ^= 1)
        {
            float* E = Le + buf * (EW * EH);
            const int shift = oy * YW + ox;
            for (int i = tid; i < EW * EH; i += DN_TX * DN_TY)
            {
                const int r = i / EW, c = i - r * EW;
                const int a = (r + R) * YW + (c + R);
                E[i] = pair_term(Ly[a], Lv[a], Ly[a + shift], Lv[a + shift], k2);
            }
            __syncthreads();   // (the other buffer is written next: its readers passed this barrier)
            const int qx = px + ox, qy = py + oy;
            if (filtered && qx >= 0 && qx < W && qy >= 0 && qy < H)
            {
                float D = 0.0f;
#pragma unroll
                for (int dy = 0; dy <= 2 * F; dy++)
                {
                    float row = 0.0f;
#pragma unroll
                    for (int dx = 0; dx <= 2 * F; dx++) row = row + E[(ty + dy) * EW + tx + dx];
                    D = D + row;
                }
                const int ci = (ty + R + oy) * CW + tx + R + ox;
                float Df = 0.0f;
#pragma unroll
                for (int j = 0; j < NF; j++) Df = Df + feature_term(fa[j], Lf[j * (CW * CH) + ci], feat.g[j]);
                const float w = guided_weight(patch_distance(D, inv_area), Df);
                den = den + w;
                nr  = nr + w * Lc[ci];
                ng  = ng + w * Lc[CW * CH + ci];
                nb  = nb + w * Lc[2 * CW * CH + ci];
            }
        }
    if (filtered) { out.x = nr / den; out.y = ng / den; out.z = nb / den; }
    if (inside) dst[pi] = out;
}

template <class... V>
__global__ __launch_bounds__(256) void denoise_guided_plain_k(float4* dst, const float4* src, const PixelStatsDev* stats, const float4* guide,
                                                              const PixelStatsDev* gstats, DenoiseFeaturesDev feat, int W, int H, int R, int F, float k2,
                                                              V... svar)
{
    const int idx = threadIdx.x + blockIdx.x * blockDim.x;
    if (idx >= W * H) return;
    const int py = idx / W, px = idx - py * W;
    const float4 A  = src[idx];
    const float  sp = inv_count(stats[idx].n);
    float4 out = make_float4(A.x * sp, A.y * sp, A.z * sp, A.w * sp);
    if (guide_variance_at(gstats, idx, svar...) != 0.0f)
    {
        const float inv_area = 1.0f / (float)((2 * F + 1) * (2 * F + 1));
        float den = 0.0f, nr = 0.0f, ng = 0.0f, nb = 0.0f;
        for (int oy = -R; oy <= R; oy++)
            for (int ox = -R; ox <= R; ox++)
            {
                const int qx = px + ox, qy = py + oy;
                if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                float D = 0.0f;
                for (int dy = -F; dy <= F; dy++)
                {
                    float row = 0.0f;
                    for (int dx = -F; dx <= F; dx++)
                    {
                        float ya, va, yb, vb;
                        guide_yv(guide, gstats, clampi(py + dy, H - 1) * W + clampi(px + dx, W - 1), ya, va, svar...);
                        guide_yv(guide, gstats, clampi(qy + dy, H - 1) * W + clampi(qx + dx, W - 1), yb, vb, svar...);
                        row = row + pair_term(ya, va, yb, vb, k2);
                    }
                    D = D + row;
                }
                const int q = qy * W + qx;
                float Df = 0.0f;
#pragma unroll   // (constant indices into the by-value struct: it stays in scalar registers)
                for (int j = 0; j < 4; j++)
                    if (j < feat.n) Df = Df + feature_term(feat.chan[j][4 * (size_t)idx], feat.chan[j][4 * (size_t)q], feat.g[j]);
                const float  w = guided_weight(patch_distance(D, inv_area), Df);
                const float4 B = src[q];
                const float  s = inv_count(stats[q].n);
                den = den + w;
                nr  = nr + w * (B.x * s);
                ng  = ng + w * (B.y * s);
                nb  = nb + w * (B.z * s);
            }
        out.x = nr / den; out.y = ng / den; out.z = nb / den;
    }
    dst[idx] = out;
}

// ---- vp_filter_variance: the filter on one scalar plane u with the noise q of its values: y := u, v := q and
// the one colour c := u of vp_denoise's definition; a pixel with u == 0 stays 0.
// denoise_tiled_k's passes with the planes it needs: (u, q) of the tile plus an R + F halo at the pitch of its (y, v) planes, and the
// double-buffered e plane.  The colour of an offset is u itself, R inside the staged plane's halo: a half-wave reads 32 consecutive
// dwords of one row of it, as it would of a colour plane.  2 yv + 2 e floats of LDS: denoise_tiled_k's less its three colour planes.
template <int F>
__global__ __launch_bounds__(DN_TX * DN_TY) void variance_tiled_k(float* dst, const float* u, const float* q, int W, int H, int R, float k2)
{
    constexpr int EW = DN_TX + 2 * F, EH = DN_TY + 2 * F;   // the e plane: the tile plus an F halo
    constexpr int YW = EW + 32;                             // pitch of the (u, q) planes (>= DN_TX + 2 (R + F) for R <= 16)
    extern __shared__ float lds[];
    const int halo = R + F, YH = DN_TY + 2 * halo;
    float* Lu = lds;
    float* Lq = Lu + YW * YH;
    float* Le = Lq + YW * YH;             // two planes of EW * EH
    const int tid = threadIdx.x, tx = tid & (DN_TX - 1), ty = tid / DN_TX;
    const int x0 = blockIdx.x * DN_TX, y0 = blockIdx.y * DN_TY;
    const int px = x0 + tx, py = y0 + ty;
    const bool inside = px < W && py < H;
    const int  pi = clampi(py, H - 1) * W + clampi(px, W - 1);
    const bool filtered = inside && u[pi] != 0.0f;
    // a tile of constants -- u == 0 in both halves -- stays one
    if (!__syncthreads_or(filtered))
    {
        if (inside) dst[pi] = 0.0f;
        return;
    }
    for (int i = tid; i < (DN_TX + 2 * halo) * YH; i += DN_TX * DN_TY)
    {
        const int r = i / (DN_TX + 2 * halo), c = i - r * (DN_TX + 2 * halo);
        const int g = clampi(y0 - halo + r, H - 1) * W + clampi(x0 - halo + c, W - 1);
        Lu[r * YW + c] = u[g];
        Lq[r * YW + c] = q[g];
    }
    __syncthreads();
    const float inv_area = 1.0f / (float)((2 * F + 1) * (2 * F + 1));
    float den = 0.0f, num = 0.0f;
    int buf = 0;
    for (int oy = -R; oy <= R; oy++)
        for (int ox = -R; ox <= R; ox++, buf ^= 1)
        {
            float* E = Le + buf * (EW * EH);
            const int shift = oy * YW + ox;
            for (int i = tid; i < EW * EH; i += DN_TX * DN_TY)
            {
                const int r = i / EW, c = i - r * EW;
                const int a = (r + R) * YW + (c + R);
                E[i] = pair_term(Lu[a], Lq[a], Lu[a + shift], Lq[a + shift], k2);
            }
            __syncthreads();   // (the other buffer is written next: its readers passed this barrier)
            const int qx = px + ox, qy = py + oy;
            if (filtered && qx >= 0 && qx < W && qy >= 0 && qy < H)
            {
                float D = 0.0f;
#pragma unroll
                for (int dy = 0; dy <= 2 * F; dy++)
                {
                    float row = 0.0f;
#pragma unroll
                    for (int dx = 0; dx <= 2 * F; dx++) row = row + E[(ty + dy) * EW + tx + dx];
                    D = D + row;
                }
                const float w = patch_weight(D, inv_area);
                den = den + w;
                num = num + w * Lu[(ty + halo + oy) * YW + tx + halo + ox];
            }
        }
    if (inside) dst[pi] = filtered ? num / den : 0.0f;
}

__global__ __launch_bounds__(256) void variance_plain_k(float* dst, const float* u, const float* q, int W, int H, int R, int F, float k2)
{
    const int idx = threadIdx.x + blockIdx.x * blockDim.x;
    if (idx >= W * H) return;
    const int py = idx / W, px = idx - py * W;
    float out = 0.0f;
    if (u[idx] != 0.0f)
    {
        const float inv_area = 1.0f / (float)((2 * F + 1) * (2 * F + 1));
        float den = 0.0f, num = 0.0f;
        for (int oy = -R; oy <= R; oy++)
            for (int ox = -R; ox <= R; ox++)
            {
                const int qx = px + ox, qy = py + oy;
                if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                float D = 0.0f;
                for (int dy = -F; dy <= F; dy++)
                {
                    float row = 0.0f;
                    for (int dx = -F; dx <= F; dx++)
                    {
                        const int a = clampi(py + dy, H - 1) * W + clampi(px + dx, W - 1);
                        const int b = clampi(qy + dy, H - 1) * W + clampi(qx + dx, W - 1);
                        row = row + pair_term(u[a], q[a], u[b], q[b], k2);
                    }
                    D = D + row;
                }
                const float w = patch_weight(D, inv_area);
                den = den + w;
                num = num + w * u[qy * W + qx];
            }
        out = num / den;
    }
    dst[idx] = out;
}

// ---- vp_select: per-pixel selection among n candidates by their smoothed error estimates
// the number of in-image positions among p - R .. p + R
__device__ __forceinline__ int span_in(int p, int R, int N)
{
    const int lo = p - R < 0 ? 0 : p - R, hi = p + R > N - 1 ? N - 1 : p + R;
    return hi - lo + 1;
}
// W_c, the pick's own count and the blend of the header from the four counts and the candidates' values at p
__device__ __forceinline__ float4 select_blend(const float4 (&v)[SELECT_MAX], const int (&cnt)[SELECT_MAX], int n, int k, int T)
{
    // the pick's value and count by masks (a chain of selects becomes an indexed load from a private array: scratch)
    unsigned bx = 0, by = 0, bz = 0, bw = 0;
    int      wk = 0;
#pragma unroll
    for (int c = 0; c < SELECT_MAX; c++)
    {
        const unsigned m = c == k ? ~0u : 0u;
        bx |= __float_as_uint(v[c].x) & m;
        by |= __float_as_uint(v[c].y) & m;
        bz |= __float_as_uint(v[c].z) & m;
        bw |= __float_as_uint(v[c].w) & m;
        wk |= cnt[c] & (int)m;
    }
    const float4 pick = make_float4(__uint_as_float(bx), __uint_as_float(by), __uint_as_float(bz), __uint_as_float(bw));
    if (wk == T) return pick;
    float nx = 0.0f, ny = 0.0f, nz = 0.0f;
#pragma unroll
    for (int c = 0; c < SELECT_MAX; c++)
        if (c < n)
        {
            const float w = (float)cnt[c];
            nx = nx + w * v[c].x;
            ny = ny + w * v[c].y;
            nz = nz + w * v[c].z;
        }
    const float t = (float)T;
    return make_float4(nx / t, ny / t, nz / t, pick.w);
}

// One 256-thread workgroup per 32 x 8 tile.  The n error planes of the tile plus an Rs + Rb halo are staged once, 0.0f where the
// position is outside the image: the sums of the definition start at +0.0f and a sum of binary32 values that starts there is never
// -0.0f, so adding +0.0f for a skipped position or a skipped row leaves every bit as it was.  Per candidate: the row sums of the tile
// plus an Rb halo (all staged rows) into the one h plane, a barrier, the column sums, the divide and the comparison in registers -- a
// thread owns up to 2 x 2 positions of the pick plane --, a barrier.  Then the picks into the index plane (-1 outside the image), and
// every thread counts its blend window from there.  The candidates' colours are read from global memory at p only.
// Every pass gives a half-wave one row and 32 consecutive columns: 32 consecutive dwords, conflict-free at any pitch, so the planes are
// dense (the second column chunk of a row has 2 Rb lanes at work: 6 of 32 at most, on 3 of 20 rows' worth of work).  The index plane
// is one dword per position: four lanes on the bytes of one dword would be four addresses on one bank.
__global__ __launch_bounds__(DN_TX * DN_TY) void select_tiled_k(float4* dst, unsigned char* index, SelectDev S, int W, int H, int Rs, int Rb)
{
    extern __shared__ float lds[];
    const int halo = Rs + Rb, RW = DN_TX + 2 * halo, RH = DN_TY + 2 * halo, PW = DN_TX + 2 * Rb, PH = DN_TY + 2 * Rb;
    float* Lr = lds;                        // n planes of RW * RH
    float* Lh = Lr + S.n * (RW * RH);       // one plane of PW * RH
    int*   Lk = (int*)(Lh + PW * RH);       // PW * PH
    const int tid = threadIdx.x, tx = tid & (DN_TX - 1), ty = tid / DN_TX;
    const int x0 = blockIdx.x * DN_TX, y0 = blockIdx.y * DN_TY;
#pragma unroll
    for (int c = 0; c < SELECT_MAX; c++)
        if (c < S.n)
            for (int i = tid; i < RW * RH; i += DN_TX * DN_TY)
            {
                const int r = i / RW, col = i - r * RW;
                const int gx = x0 - halo + col, gy = y0 - halo + r;
                Lr[c * (RW * RH) + i] = (gx >= 0 && gx < W && gy >= 0 && gy < H) ? S.err[c][(size_t)gy * W + gx] : 0.0f;
            }
    __syncthreads();
    // the thread's positions of the pick plane: rows ty, ty + 8, columns tx, tx + 32
    float best[2][2];
    int   pick[2][2] = {};
#pragma unroll
    for (int c = 0; c < SELECT_MAX; c++)
        if (c < S.n)   // (uniform: the barriers inside are reached by all or none)
        {
            const float* R0 = Lr + c * (RW * RH);
            for (int r = ty; r < RH; r += DN_TY)
                for (int col = tx; col < PW; col += DN_TX)
                {
                    float row = 0.0f;
                    for (int t = 0; t <= 2 * Rs; t++) row = row + R0[r * RW + col + t];
                    Lh[r * PW + col] = row;
                }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 2; j++)
#pragma unroll
                for (int i = 0; i < 2; i++)
                {
                    const int r = ty + j * DN_TY, col = tx + i * DN_TX;
                    if (r >= PH || col >= PW) continue;
                    float sum = 0.0f;
                    for (int t = 0; t <= 2 * Rs; t++) sum = sum + Lh[(r + t) * PW + col];
                    const int gx = x0 - Rb + col, gy = y0 - Rb + r;
                    // (outside the image the count is not one of a window; the position is marked below and its E never used)
                    const float E = sum / (float)(span_in(clampi(gx, W - 1), Rs, W) * span_in(clampi(gy, H - 1), Rs, H));
                    if (c == 0 || E < best[j][i]) { best[j][i] = E; pick[j][i] = c; }
                }
            __syncthreads();   // (the h plane is written next)
        }
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
        for (int i = 0; i < 2; i++)
        {
            const int r = ty + j * DN_TY, col = tx + i * DN_TX;
            if (r >= PH || col >= PW) continue;
            const int gx = x0 - Rb + col, gy = y0 - Rb + r;
            Lk[r * PW + col] = (gx >= 0 && gx < W && gy >= 0 && gy < H) ? pick[j][i] : -1;
        }
    __syncthreads();
    const int px = x0 + tx, py = y0 + ty;
    if (px >= W || py >= H) return;
    int cnt[SELECT_MAX] = {};
    for (int dy = 0; dy <= 2 * Rb; dy++)
        for (int dx = 0; dx <= 2 * Rb; dx++)
        {
            const int k = Lk[(ty + dy) * PW + tx + dx];
#pragma unroll
            for (int c = 0; c < SELECT_MAX; c++) cnt[c] += k == c;
        }
    const int    k = Lk[(ty + Rb) * PW + tx + Rb];
    const size_t p = (size_t)py * W + px;
    float4 v[SELECT_MAX];
#pragma unroll
    for (int c = 0; c < SELECT_MAX; c++) v[c] = c < S.n ? S.img[c][p] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    dst[p] = select_blend(v, cnt, S.n, k, span_in(px, Rb, W) * span_in(py, Rb, H));
    if (index) index[p] = (unsigned char)k;
}

// k(q) of the header straight from global memory: positions outside the image skipped, as the definition says it
__device__ __forceinline__ int select_pick_at(const SelectDev& S, int qx, int qy, int W, int H, int Rs)
{
    const float count = (float)(span_in(qx, Rs, W) * span_in(qy, Rs, H));
    float best = 0.0f;
    int   k = 0;
#pragma unroll
    for (int c = 0; c < SELECT_MAX; c++)
        if (c < S.n)
        {
            float sum = 0.0f;
            for (int ty = -Rs; ty <= Rs; ty++)
            {
                const int y = qy + ty;
                if (y < 0 || y >= H) continue;
                float row = 0.0f;
                for (int tx = -Rs; tx <= Rs; tx++)
                {
                    const int x = qx + tx;
                    if (x < 0 || x >= W) continue;
                    row = row + S.err[c][(size_t)y * W + x];
                }
                sum = sum + row;
            }
            const float E = sum / count;
            if (c == 0 || E < best) { best = E; k = c; }
        }
    return k;
}
__global__ __launch_bounds__(256) void select_plain_k(float4* dst, unsigned char* index, SelectDev S, int W, int H, int Rs, int Rb)
{
    const int idx = threadIdx.x + blockIdx.x * blockDim.x;
    if (idx >= W * H) return;
    const int py = idx / W, px = idx - py * W;
    int cnt[SELECT_MAX] = {};
    int T = 0;
    for (int dy = -Rb; dy <= Rb; dy++)
        for (int dx = -Rb; dx <= Rb; dx++)
        {
            const int qx = px + dx, qy = py + dy;
            if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
            const int k = select_pick_at(S, qx, qy, W, H, Rs);
#pragma unroll
            for (int c = 0; c < SELECT_MAX; c++) cnt[c] += k == c;
            T++;
        }
    const int k = select_pick_at(S, px, py, W, H, Rs);
    float4 v[SELECT_MAX];
#pragma unroll
    for (int c = 0; c < SELECT_MAX; c++) v[c] = c < S.n ? S.img[c][idx] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    dst[idx] = select_blend(v, cnt, S.n, k, T);
    if (index) index[idx] = (unsigned char)k;
}

template <int F, class... V>
void launch_guided_tiled(int NF, dim3 grid, dim3 block, size_t lds, hipStream_t st, float4* dst, const float4* src, const PixelStatsDev* stats,
                         const float4* guide, const PixelStatsDev* gstats, const DenoiseFeaturesDev& feat, int W, int H, int R, float k2, V... svar)
{
    switch (NF)
    {
    case 1: hipLaunchKernelGGL((denoise_guided_tiled_k<F, 1, V...>), grid, block, lds, st, dst, src, stats, guide, gstats, feat, W, H, R, k2, svar...); break;
    case 2: hipLaunchKernelGGL((denoise_guided_tiled_k<F, 2, V...>), grid, block, lds, st, dst, src, stats, guide, gstats, feat, W, H, R, k2, svar...); break;
    case 3: hipLaunchKernelGGL((denoise_guided_tiled_k<F, 3, V...>), grid, block, lds, st, dst, src, stats, guide, gstats, feat, W, H, R, k2, svar...); break;
    default: hipLaunchKernelGGL((denoise_guided_tiled_k<F, 4, V...>), grid, block, lds, st, dst, src, stats, guide, gstats, feat, W, H, R, k2, svar...); break;
    }
}
// the two launchers with the pack of the kernels: empty for vp_denoise / vp_denoise_guided, the variance plane for vp_denoise_var
template <class... V>
void launch_denoise_v(float4* dst, const float4* src, const PixelStatsDev* stats, const float4* guide, const PixelStatsDev* gstats, int W, int H, int R, int F,
                      float k2, int form, hipStream_t st, V... svar)
{
    if (form == 1)
    {
        hipLaunchKernelGGL((denoise_plain_k<V...>), dim3((unsigned)(((size_t)W * H + 255) / 256)), dim3(256), 0, st, dst, src, stats, guide, gstats, W, H, R, F, k2,
                           svar...);
        return;
    }
    const dim3   grid((W + DN_TX - 1) / DN_TX, (H + DN_TY - 1) / DN_TY), block(DN_TX * DN_TY);
    const size_t lds = denoise_lds_bytes(R, F);
    switch (F)
    {
    case 0: hipLaunchKernelGGL((denoise_tiled_k<0, V...>), grid, block, lds, st, dst, src, stats, guide, gstats, W, H, R, k2, svar...); break;
    case 1: hipLaunchKernelGGL((denoise_tiled_k<1, V...>), grid, block, lds, st, dst, src, stats, guide, gstats, W, H, R, k2, svar...); break;
    case 2: hipLaunchKernelGGL((denoise_tiled_k<2, V...>), grid, block, lds, st, dst, src, stats, guide, gstats, W, H, R, k2, svar...); break;
    default: hipLaunchKernelGGL((denoise_tiled_k<3, V...>), grid, block, lds, st, dst, src, stats, guide, gstats, W, H, R, k2, svar...); break;
    }
}
template <class... V>
void launch_denoise_guided_v(float4* dst, const float4* src, const PixelStatsDev* stats, const float4* guide, const PixelStatsDev* gstats,
                             const DenoiseFeaturesDev& feat, int W, int H, int R, int F, float k2, int form, hipStream_t st, V... svar)
{
    if (form == 1)
    {
        hipLaunchKernelGGL((denoise_guided_plain_k<V...>), dim3((unsigned)(((size_t)W * H + 255) / 256)), dim3(256), 0, st, dst, src, stats, guide, gstats, feat, W,
                           H, R, F, k2, svar...);
        return;
    }
    const dim3   grid((W + DN_TX - 1) / DN_TX, (H + DN_TY - 1) / DN_TY), block(DN_TX * DN_TY);
    const size_t lds = denoise_guided_lds_bytes(R, F, feat.n);
    switch (F)
    {
    case 0: launch_guided_tiled<0>(feat.n, grid, block, lds, st, dst, src, stats, guide, gstats, feat, W, H, R, k2, svar...); break;
    case 1: launch_guided_tiled<1>(feat.n, grid, block, lds, st, dst, src, stats, guide, gstats, feat, W, H, R, k2, svar...); break;
    case 2: launch_guided_tiled<2>(feat.n, grid, block, lds, st, dst, src, stats, guide, gstats, feat, W, H, R, k2, svar...); break;
    default: launch_guided_tiled<3>(feat.n, grid, block, lds, st, dst, src, stats, guide, gstats, feat, W, H, R, k2, svar...); break;
    }
}
}  // namespace

size_t denoise_lds_bytes(int R, int F)
{
    const size_t yv = (size_t)(DN_TX + 2 * F + 32) * (DN_TY + 2 * (R + F));
    const size_t c  = (size_t)(DN_TX + 2 * R) * (DN_TY + 2 * R);
    const size_t e  = (size_t)(DN_TX + 2 * F) * (DN_TY + 2 * F);
    return (2 * yv + 3 * c + 2 * e) * sizeof(float);
}
void launch_denoise(float4* dst, const float4* src, const PixelStatsDev* stats, const float4* guide, const PixelStatsDev* gstats, int W, int H, int R,
                    int F, float k2, int form, hipStream_t st)
{
    launch_denoise_v(dst, src, stats, guide, gstats, W, H, R, F, k2, form, st);
}
size_t denoise_guided_lds_bytes(int R, int F, int n_features)
{
    return denoise_lds_bytes(R, F) + (size_t)n_features * (DN_TX + 2 * R) * (DN_TY + 2 * R) * sizeof(float);
}
void launch_denoise_guided(float4* dst, const float4* src, const PixelStatsDev* stats, const float4* guide, const PixelStatsDev* gstats,
                           const DenoiseFeaturesDev& feat, int W, int H, int R, int F, float k2, int form, hipStream_t st)
{
    launch_denoise_guided_v(dst, src, stats, guide, gstats, feat, W, H, R, F, k2, form, st);
}
void launch_denoise_var(float4* dst, const float4* src, const PixelStatsDev* stats, const float4* guide, const PixelStatsDev* gstats, const float* svar,
                        const DenoiseFeaturesDev& feat, int W, int H, int R, int F, float k2, int form, hipStream_t st)
{
    if (feat.n) launch_denoise_guided_v(dst, src, stats, guide, gstats, feat, W, H, R, F, k2, form, st, svar);
    else launch_denoise_v(dst, src, stats, guide, gstats, W, H, R, F, k2, form, st, svar);
}
size_t variance_lds_bytes(int R, int F)
{
    const size_t uq = (size_t)(DN_TX + 2 * F + 32) * (DN_TY + 2 * (R + F));
    const size_t e  = (size_t)(DN_TX + 2 * F) * (DN_TY + 2 * F);
    return (2 * uq + 2 * e) * sizeof(float);
}
void launch_filter_variance(float* dst, const float* u, const float* q, int W, int H, int R, int F, float k2, int form, hipStream_t st)
{
    if (form == 1)
    {
        hipLaunchKernelGGL(variance_plain_k, dim3((unsigned)(((size_t)W * H + 255) / 256)), dim3(256), 0, st, dst, u, q, W, H, R, F, k2);
        return;
    }
    const dim3   grid((W + DN_TX - 1) / DN_TX, (H + DN_TY - 1) / DN_TY), block(DN_TX * DN_TY);
    const size_t lds = variance_lds_bytes(R, F);
    switch (F)
    {
    case 0: hipLaunchKernelGGL(variance_tiled_k<0>, grid, block, lds, st, dst, u, q, W, H, R, k2); break;
    case 1: hipLaunchKernelGGL(variance_tiled_k<1>, grid, block, lds, st, dst, u, q, W, H, R, k2); break;
    case 2: hipLaunchKernelGGL(variance_tiled_k<2>, grid, block, lds, st, dst, u, q, W, H, R, k2); break;
    default: hipLaunchKernelGGL(variance_tiled_k<3>, grid, block, lds, st, dst, u, q, W, H, R, k2); break;
    }
}
size_t select_lds_bytes(int n, int Rs, int Rb)
{
    const size_t halo = (size_t)Rs + Rb;
    const size_t r = (DN_TX + 2 * halo) * (DN_TY + 2 * halo), h = (size_t)(DN_TX + 2 * Rb) * (DN_TY + 2 * halo), k = (size_t)(DN_TX + 2 * Rb) * (DN_TY + 2 * Rb);
    return (n * r + h + k) * sizeof(float);
}
void launch_select(float4* dst, unsigned char* index, const SelectDev& S, int W, int H, int Rs, int Rb, int form, hipStream_t st)
{
    if (form == 1)
    {
        hipLaunchKernelGGL(select_plain_k, dim3((unsigned)(((size_t)W * H + 255) / 256)), dim3(256), 0, st, dst, index, S, W, H, Rs, Rb);
        return;
    }
    const dim3 grid((W + DN_TX - 1) / DN_TX, (H + DN_TY - 1) / DN_TY), block(DN_TX * DN_TY);
    hipLaunchKernelGGL(select_tiled_k, grid, block, select_lds_bytes(S.n, Rs, Rb), st, dst, index, S, W, H, Rs, Rb);
}
}  // namespace vp
