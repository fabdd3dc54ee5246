/* ref_harness.cpp -- TEST INFRASTRUCTURE (oracle/refshim).  Not part of the product.
 *
 * The one translation unit of oracle/_ref/libkernel_ref*.so.  oracle/Makefile (target `ref`) writes two files next to a copy of
 * this one in a temporary directory -- ref_kernel.inc, the reference's kernel file with its launches spelled SHIM_LAUNCH, and
 * ref_bounds.inc, the bound builder of the reference's host file -- and deletes them after the compile.  Including them here
 * makes the reference's own extern "C" entry points (init_cuda, set_texture_filter_mode, precompute_opacity, init_envmap,
 * set_sun, copy_inv_view_matrix, scale, gamma_correct, render_kernel, ...) exist as they are; this file adds a way to run each
 * of the three render kernels one "thread" per pixel and to read back the tables the reference builds.
 *
 * The library keeps its scene in file-scope symbols, as the reference does: one scene per library, not thread-safe.
 */
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <utility>

#include "cuda_runtime.h"
#include "cuda_helpers.h"

thread_local uint3 threadIdx, blockIdx;
thread_local dim3  blockDim, gridDim;

/* the bound builder times its sweeps */
struct Timer
{
    void  record() {}
    float elapsed() { return 0.0f; }
};

#include "shim_math.h" /* after every standard header */

#define USE_OPENVDB 1 /* the volume-texture branch of vol_sigma_t / vol_bound: the only one that compiles */
#undef M_PI_2         /* vecmath.h declares these two as constants */
#undef M_1_PI

#include "ref_kernel.inc"
#include "ref_bounds.inc"

extern "C" {

/* init_cuda + set_texture_filter_mode; box_min/box_max NULL = the reference's default box */
void ref_init_volume(void* volume, int nx, int ny, int nz, int quantized, const float* bmin, const float* bmax, int linear)
{
    float3 lo, hi;
    if (bmin && bmax)
    {
        lo = make_float3(bmin[0], bmin[1], bmin[2]);
        hi = make_float3(bmax[0], bmax[1], bmax[2]);
    }
    TextureVolume::init_cuda(volume, make_cudaExtent(nx, ny, nz), quantized != 0, bmin && bmax ? &lo : nullptr,
                             bmin && bmax ? &hi : nullptr);
    TextureVolume::set_texture_filter_mode(linear != 0);
}

/* which: 0 __d_render, 1 __d_render_bounded_decomp, 2 __d_render_bounded (the numbering of vp_oracle.h's estimators);
 * out: width * height float4, accumulated into as the kernels do */
int ref_render(int which, float* out, int frame, const Param* P)
{
    if (which < 0 || which > 2) return -1;
    gridDim   = dim3(P->width, P->height, 1);
    blockDim  = dim3(1, 1, 1);
    threadIdx = make_uint3(0, 0, 0);
    for (unsigned y = 0; y < P->height; y++)
        for (unsigned x = 0; x < P->width; x++)
        {
            blockIdx = make_uint3(x, y, 0);
            if (which == 0) __d_render((float4*)out, frame, *P);
            else if (which == 1) __d_render_bounded_decomp((float4*)out, frame, *P);
            else __d_render_bounded((float4*)out, frame, *P);
        }
    return 0;
}

static size_t copy_array(const cudaArray* a, void* out)
{
    if (!a) return 0;
    size_t n = a->w * a->h * a->d * a->elem;
    if (out) memcpy(out, a->data, n);
    return n;
}
/* the (max, min) bound table: uchar2 or float2 per voxel; returns its size in bytes */
size_t ref_get_bounds(void* out) { return copy_array(TextureVolume::h_volume_bound_array.array, out); }
/* the optical-depth table of the last precompute_opacity */
size_t ref_get_opacity(void* out) { return copy_array(TextureVolume::h_opacity_array.array, out); }
/* which: 0 the environment texels, 1 pdfY, 2 cdfY, 3 pdfX, 4 cdfX */
size_t ref_get_env(int which, void* out)
{
    const cudaArray* a[5] = {Envmap::HDRtexture_, Envmap::EnvmapPdfY_, Envmap::EnvmapCdfY_, Envmap::EnvmapPdfX_, Envmap::EnvmapCdfX_};
    return which < 0 || which > 4 ? 0 : copy_array(a[which], out);
}
float ref_get_pdfnorm_alt() { return Envmap::HDRpdfnormAlt; }
/* direction, directional power, disc radiance */
void ref_get_sun(float* out9)
{
    memcpy(out9, &sun_light_dir, 12);
    memcpy(out9 + 3, &sun_light_power, 12);
    memcpy(out9 + 6, &sun_light_power_original, 12);
}
/* which of the reference's compile-time switches this library was built with */
void ref_get_config(int* out3)
{
    out3[0] = PASSIVE_ENVMAP;
    out3[1] = SPECTRAL_TRACKING;
    out3[2] = MULTI_CHANNEL;
}
}
