// vp_denoise.hip -- the variance-guided NL-means filter of the output stage (include/volpath.h vp_denoise).
//
// Every kernel computes the definition of the header to the bit: binary32, no contraction, the patch distance as row sums left to
// right and their sum top to bottom, the weights summed over the offsets in raster order, expf_ in the exact arithmetic (this file
// is compiled without VP_ARITH_FAST, like the output stage of vp_kernels.hip).
// Each pass is written once, as a __device__ __forceinline__ template over a loader that gives (y, v) at a clamped pixel index and an
// accumulator that takes an offset's patch sum; the __global__ kernels are instances of these:
//   stage_yv + tiled_offsets (form 0): one 256-thread workgroup per 32 x 8 pixel tile.  (y, v) of the tile plus an R + F halo are
//     staged in LDS once, fetched with clamped coordinates; per offset the pair terms e of the tile's F-halo plane are computed once
//     each into LDS (2.1 per thread at F = 3 instead of 49) and every thread sums its patch from there.  The plane is double
//     buffered: one barrier per offset.
//   plain_offsets (form 1): one thread per pixel, straight from global memory, looping over the definition.  The cross-check.
//   denoise_tiled<F, NF>: the tiled colour filter on these.  The loader is guide_yv, the mean colours of the tile plus an R halo are
//     staged beside (y, v), the sums are a ColourSum.  NF = 0 is vp_denoise (denoise_tiled_k); otherwise vp_denoise_guided (DESIGN.md
//     section 2.13; denoise_guided_tiled_k): NF feature channels staged once into LDS planes shaped like the colour planes and a
//     per-pixel-pair feature distance that caps the weight.  With NF = 0 the feature planes, their staging and the distance are no code.
//   denoise_plain_k is plain_offsets with guide_yv and a ColourSum.  denoise_guided_plain_k keeps loops of its own: on plain_offsets it
//     was half a per cent slower on a 1280 x 720 image, the same in every run, with the same instructions in its loops in another
//     arrangement (profiles/denoise_fold_kernel_resources.txt); as it stands it is the kernel it was, instruction for instruction.
//   vp_denoise_var's instances of these four: a trailing parameter pack V that is empty or one `const float*`, the caller's per-sample
//     variance plane; v is then plane[a] * s_a in place of the records' variance, everything else as it stands.  An empty pack adds
//     no kernel parameter (profiles/variance_kernel_resources.txt, profiles/denoise_fold_kernel_resources.txt).
//   variance_tiled_k / variance_plain_k: the two forms of vp_filter_variance, the same passes on one scalar
//     plane u with its noise q: the loader is (u[g], q[g]), there are no colour planes -- u with its R halo is inside the staged
//     plane -- and a pixel is filtered where u != 0.
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
// vp_denoise_guided: the weight of an offset cut by a distance of noise-free features
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
// the weight of an offset from its patch sum D; Df, the feature distance, is read by the guided filter only
template <bool GUIDED>
__device__ __forceinline__ float offset_weight(float D, float inv_area, float Df)
{
    if constexpr (GUIDED) return guided_weight(patch_distance(D, inv_area), Df);
    else return patch_weight(D, inv_area);
}
__device__ __forceinline__ float patch_inv_area(int F) { return 1.0f / (float)((2 * F + 1) * (2 * F + 1)); }
// the colour kernels' sums over the offsets and the quotient that is the filtered colour
struct ColourSum
{
    float den = 0.0f, nr = 0.0f, ng = 0.0f, nb = 0.0f;
    __device__ __forceinline__ void add(float w, float r, float g, float b)
    {
        den = den + w;
        nr  = nr + w * r;
        ng  = ng + w * g;
        nb  = nb + w * b;
    }
    __device__ __forceinline__ void divide_into(float4& out) const { out.x = nr / den; out.y = ng / den; out.z = nb / den; }
};

// ---- form 0: the tile
// the planes of a tile at patch radius F: the e plane is the tile plus an F halo; YW is the pitch of the two staged (y, v) planes
// (>= DN_TX + 2 (R + F) for R <= 16), which have DN_TY + 2 (R + F) rows
template <int F>
struct TilePlanes
{
    static constexpr int EW = DN_TX + 2 * F, EH = DN_TY + 2 * F, YW = EW + 32;
};
// a thread's place: its tile's origin, its pixel (px, py), whether that is inside the image, and the pixel's index clamped into it.
// Every function that needs it makes its own from the built-in indices: the compiler knows their ranges there, and merges the copies
struct TilePos
{
    int  tid, tx, ty, x0, y0, px, py, pi;
    bool inside;
    __device__ __forceinline__ TilePos(int W, int H)
    {
        tid = threadIdx.x; tx = tid & (DN_TX - 1); ty = tid / DN_TX;
        x0 = blockIdx.x * DN_TX; y0 = blockIdx.y * DN_TY;
        px = x0 + tx; py = y0 + ty;
        inside = px < W && py < H;
        pi = clampi(py, H - 1) * W + clampi(px, W - 1);
    }
};
// (y, v) of the tile plus a halo of R + F, YH = DN_TY + 2 halo rows, into the planes Ly, Lv, fetched with clamped coordinates:
// load(g, y, v) gives the two at pixel g.  halo and YH are the caller's, which lays out its planes with them: derived once more in
// here they cost the F >= 2 instances two VGPRs (profiles/denoise_fold_kernel_resources.txt)
template <int F, class Load>
__device__ __forceinline__ void stage_yv(float* Ly, float* Lv, int W, int H, int halo, int YH, Load load)
{
    constexpr int YW = TilePlanes<F>::YW;
    const TilePos t(W, H);
    for (int i = t.tid; i < (DN_TX + 2 * halo) * YH; i += DN_TX * DN_TY)
    {
        const int r = i / (DN_TX + 2 * halo), c = i - r * (DN_TX + 2 * halo);
        float y, v;
        load(clampi(t.y0 - halo + r, H - 1) * W + clampi(t.x0 - halo + c, W - 1), y, v);
        Ly[r * YW + c] = y;
        Lv[r * YW + c] = v;
    }
}
// the offsets in raster order.  Per offset: the e plane of the tile from the staged (y, v) into one of the two buffers at Le, one
// barrier, and where the thread's pixel is filtered and the offset stays inside the image, acc(D, ox, oy) with the patch sum D
template <int F, class Acc>
__device__ __forceinline__ void tiled_offsets(const float* Ly, const float* Lv, float* Le, bool filtered, int W, int H, int R, float k2, Acc acc)
{
    constexpr int EW = TilePlanes<F>::EW, EH = TilePlanes<F>::EH, YW = TilePlanes<F>::YW;
    const TilePos t(W, H);
    int buf = 0;
    for (int oy = -R; oy <= R; oy++)
        for (int ox = -R; ox <= R; ox++, buf ^= 1)
        {
            float* E = Le + buf * (EW * EH);
            const int shift = oy * YW + ox;
            for (int i = t.tid; i < EW * EH; i += DN_TX * DN_TY)
            {
                const int r = i / EW, c = i - r * EW;
                const int a = (r + R) * YW + (c + R);
                E[i] = pair_term(Ly[a], Lv[a], Ly[a + shift], Lv[a + shift], k2);
            }
            __syncthreads();   // (the other buffer is written next: its readers passed this barrier)
            const int qx = t.px + ox, qy = t.py + oy;
            if (filtered && qx >= 0 && qx < W && qy >= 0 && qy < H)
            {
                float D = 0.0f;
#pragma unroll
                for (int dy = 0; dy <= 2 * F; dy++)
                {
                    float row = 0.0f;
#pragma unroll
                    for (int dx = 0; dx <= 2 * F; dx++) row = row + E[(t.ty + dy) * EW + t.tx + dx];
                    D = D + row;
                }
                acc(D, ox, oy);
            }
        }
}

// ---- form 1: the definition at pixel (px, py) from global memory.  Per offset that stays inside the image, in raster order: the patch
// sum D over clamped positions, load(g, y, v) giving the two planes at pixel g, and acc(D, q) with the offset's pixel index q
template <class Load, class Acc>
__device__ __forceinline__ void plain_offsets(int px, int py, int W, int H, int R, int F, float k2, Load load, Acc acc)
{
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
                    load(clampi(py + dy, H - 1) * W + clampi(px + dx, W - 1), ya, va);
                    load(clampi(qy + dy, H - 1) * W + clampi(qx + dx, W - 1), yb, vb);
                    row = row + pair_term(ya, va, yb, vb, k2);
                }
                D = D + row;
            }
            acc(D, qy * W + qx);
        }
}

// ---- the colour filter: vp_denoise (NF == 0, feat unused), vp_denoise_guided (NF features) and vp_denoise_var's instances of both.
// LDS: the two (y, v) planes, the mean colours of the tile plus an R halo, the two e planes (denoise_lds_bytes) and behind them NF
// feature planes at the pitch and indexing of the colour planes (denoise_guided_lds_bytes): fb of a half-wave is 32 consecutive dwords,
// fa stays in registers, and the features cost no barrier
template <int F, int NF, class... V>
__device__ __forceinline__ void denoise_tiled(float4* dst, const float4* src, const PixelStatsDev* stats, const float4* guide, const PixelStatsDev* gstats,
                                              DenoiseFeaturesDev feat, int W, int H, int R, float k2, V... svar)
{
    using P = TilePlanes<F>;
    extern __shared__ float lds[];
    const int YH = DN_TY + 2 * (R + F), CW = DN_TX + 2 * R, CH = DN_TY + 2 * R;
    float* Ly = lds;
    float* Lv = Ly + P::YW * YH;
    float* Lc = Lv + P::YW * YH;              // three planes of CW * CH
    float* Le = Lc + 3 * CW * CH;             // two planes of EW * EH
    float* Lf = Le + 2 * P::EW * P::EH;       // NF planes of CW * CH
    const TilePos t(W, H);
    // the thread's own pixel: mean colour, heat and the guide's variance
    const float4 A  = src[t.pi];
    const float  sp = inv_count(stats[t.pi].n);
    const float  vme = guide_variance_at(gstats, t.pi, svar...);
    float4 out = make_float4(A.x * sp, A.y * sp, A.z * sp, A.w * sp);
    // a tile without a noisy pixel (the per-pixel-constant classes) is the plain output stage
    if (!__syncthreads_or(t.inside && vme != 0.0f))
    {
        if (t.inside) dst[t.pi] = out;
        return;
    }
    const int halo = R + F;
    stage_yv<F>(Ly, Lv, W, H, halo, YH, [&](int g, float& y, float& v) { guide_yv(guide, gstats, g, y, v, svar...); });
    for (int i = t.tid; i < CW * CH; i += DN_TX * DN_TY)
    {
        const int r = i / CW, c = i - r * CW;
        const int g = clampi(t.y0 - R + r, H - 1) * W + clampi(t.x0 - R + c, W - 1);
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
    const bool  filtered = t.inside && vme != 0.0f;
    const float inv_area = patch_inv_area(F);
    float fa[NF ? NF : 1];
#pragma unroll
    for (int j = 0; j < NF; j++) fa[j] = Lf[j * (CW * CH) + (t.ty + R) * CW + t.tx + R];
    ColourSum sum;
    tiled_offsets<F>(Ly, Lv, Le, filtered, W, H, R, k2, [&](float D, int ox, int oy) {
        const int ci = (t.ty + R + oy) * CW + t.tx + R + ox;
        float Df = 0.0f;
#pragma unroll
        for (int j = 0; j < NF; j++) Df = Df + feature_term(fa[j], Lf[j * (CW * CH) + ci], feat.g[j]);
        sum.add(offset_weight<NF != 0>(D, inv_area, Df), Lc[ci], Lc[CW * CH + ci], Lc[2 * CW * CH + ci]);
    });
    if (filtered) sum.divide_into(out);
    if (t.inside) dst[t.pi] = out;
}

template <int F, class... V>
__global__ __launch_bounds__(DN_TX * DN_TY) void denoise_tiled_k(float4* dst, const float4* src, const PixelStatsDev* stats, const float4* guide,
                                                                  const PixelStatsDev* gstats, int W, int H, int R, float k2, V... svar)
{
    denoise_tiled<F, 0>(dst, src, stats, guide, gstats, DenoiseFeaturesDev{}, W, H, R, k2, svar...);
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
        const float inv_area = patch_inv_area(F);
        ColourSum sum;
        plain_offsets(px, py, W, H, R, F, k2, [&](int g, float& y, float& v) { guide_yv(guide, gstats, g, y, v, svar...); }, [&](float D, int q) {
            const float  w = patch_weight(D, inv_area);
            const float4 B = src[q];
            const float  s = inv_count(stats[q].n);
            sum.add(w, B.x * s, B.y * s, B.z * s);
        });
        sum.divide_into(out);
    }
    dst[idx] = out;
}
template <int F, int NF, class... V>
__global__ __launch_bounds__(DN_TX * DN_TY) void denoise_guided_tiled_k(float4* dst, const float4* src, const PixelStatsDev* stats, const float4* guide,
                                                                         const PixelStatsDev* gstats, DenoiseFeaturesDev feat, int W, int H, int R, float k2,
                                                                         V... svar)
{
    denoise_tiled<F, NF>(dst, src, stats, guide, gstats, feat, W, H, R, k2, svar...);
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
        // (plain_offsets and ColourSum written out: see the file header)
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
// The colour of an offset is u itself, R inside the staged plane's halo: a half-wave reads 32 consecutive dwords of one row of it, as
// it would of a colour plane.  2 yv + 2 e floats of LDS: denoise_tiled's less its three colour planes.
template <int F>
__global__ __launch_bounds__(DN_TX * DN_TY) void variance_tiled_k(float* dst, const float* u, const float* q, int W, int H, int R, float k2)
{
    using P = TilePlanes<F>;
    extern __shared__ float lds[];
    const int halo = R + F, YH = DN_TY + 2 * halo;
    float* Lu = lds;
    float* Lq = Lu + P::YW * YH;
    float* Le = Lq + P::YW * YH;              // two planes of EW * EH
    const TilePos t(W, H);
    const bool filtered = t.inside && u[t.pi] != 0.0f;
    // a tile of constants -- u == 0 in both halves -- stays one
    if (!__syncthreads_or(filtered))
    {
        if (t.inside) dst[t.pi] = 0.0f;
        return;
    }
    stage_yv<F>(Lu, Lq, W, H, halo, YH, [&](int g, float& y, float& v) { y = u[g]; v = q[g]; });
    __syncthreads();
    const float inv_area = patch_inv_area(F);
    float den = 0.0f, num = 0.0f;
    tiled_offsets<F>(Lu, Lq, Le, filtered, W, H, R, k2, [&](float D, int ox, int oy) {
        const float w = patch_weight(D, inv_area);
        den = den + w;
        num = num + w * Lu[(t.ty + halo + oy) * P::YW + t.tx + halo + ox];
    });
    if (t.inside) dst[t.pi] = filtered ? num / den : 0.0f;
}

__global__ __launch_bounds__(256) void variance_plain_k(float* dst, const float* u, const float* q, int W, int H, int R, int F, float k2)
{
    const int idx = threadIdx.x + blockIdx.x * blockDim.x;
    if (idx >= W * H) return;
    const int py = idx / W, px = idx - py * W;
    float out = 0.0f;
    if (u[idx] != 0.0f)
    {
        const float inv_area = patch_inv_area(F);
        float den = 0.0f, num = 0.0f;
        plain_offsets(px, py, W, H, R, F, k2, [&](int g, float& y, float& v) { y = u[g]; v = q[g]; }, [&](float D, int g) {
            const float w = patch_weight(D, inv_area);
            den = den + w;
            num = num + w * u[g];
        });
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
size_t denoise_guided_lds_bytes(int R, int F, int n_features)
{
    return denoise_lds_bytes(R, F) + (size_t)n_features * (DN_TX + 2 * R) * (DN_TY + 2 * R) * sizeof(float);
}
// the colour filter's one launcher: svar null or the per-sample variance plane, feat.n == 0 or the features
void launch_denoise(float4* dst, const float4* src, const PixelStatsDev* stats, const float4* guide, const PixelStatsDev* gstats, const float* svar,
                    const DenoiseFeaturesDev& feat, int W, int H, int R, int F, float k2, int form, hipStream_t st)
{
    if (feat.n && svar) launch_denoise_guided_v(dst, src, stats, guide, gstats, feat, W, H, R, F, k2, form, st, svar);
    else if (feat.n) launch_denoise_guided_v(dst, src, stats, guide, gstats, feat, W, H, R, F, k2, form, st);
    else if (svar) launch_denoise_v(dst, src, stats, guide, gstats, W, H, R, F, k2, form, st, svar);
    else launch_denoise_v(dst, src, stats, guide, gstats, W, H, R, F, k2, form, st);
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
