/* cuda_runtime.h -- TEST INFRASTRUCTURE (oracle/refshim).  Not part of the product.
 *
 * A host-memory stand-in for the part of the CUDA runtime that the reference's kernel file uses, so that the
 * file compiles for the CPU and its own control flow can be compared with oracle/vp_oracle.c (oracle/Makefile,
 * target `ref`).  Written from the CUDA runtime's documented signatures; nothing here is taken from the
 * reference or from its helper headers.
 *
 * Two things in this directory are DEFINITION rather than measurement, because CUDA hardware is not here to ask:
 * the texture fetch rule below (texel-centre coordinates, clamp addressing, 8-bit filter weights, uchar texels
 * filtered in integers -- the rule vp_oracle.c states for tex3D) and the elementary functions of shim_math.h.
 * Everything else the built library does is the reference's own code.
 */
#ifndef REFSHIM_CUDA_RUNTIME_H
#define REFSHIM_CUDA_RUNTIME_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define __host__
#define __device__
#define __global__
#define __constant__
#define __shared__
#define __forceinline__ inline

#define fprintf_s fprintf
#define printf_s(...) ((void)0) /* the bound builder's progress lines */

/* ------------------------------------------------------------------ vector types -- */
#define SHIM_VEC(T, N)                                                                                       \
    struct N##1 { T x; };                                                                                    \
    struct N##2 { T x, y; };                                                                                 \
    struct N##3 { T x, y, z; };                                                                              \
    struct N##4 { T x, y, z, w; };                                                                           \
    static inline N##1 make_##N##1(T x) { N##1 v = {x}; return v; }                                          \
    static inline N##2 make_##N##2(T x, T y) { N##2 v = {x, y}; return v; }                                  \
    static inline N##3 make_##N##3(T x, T y, T z) { N##3 v = {x, y, z}; return v; }                          \
    static inline N##4 make_##N##4(T x, T y, T z, T w) { N##4 v = {x, y, z, w}; return v; }
SHIM_VEC(float, float)
SHIM_VEC(int, int)
SHIM_VEC(unsigned int, uint)
SHIM_VEC(unsigned char, uchar)
SHIM_VEC(short, short)
SHIM_VEC(unsigned short, ushort)
#undef SHIM_VEC

struct dim3
{
    unsigned int x, y, z;
    dim3(unsigned int x_ = 1, unsigned int y_ = 1, unsigned int z_ = 1) : x(x_), y(y_), z(z_) {}
};

/* one "GPU thread" at a time per host thread */
extern thread_local uint3 threadIdx, blockIdx;
extern thread_local dim3  blockDim, gridDim;

static inline float __uint_as_float(unsigned int u) { float f; memcpy(&f, &u, 4); return f; }

typedef int cudaError_t;
enum { cudaSuccess = 0 };
enum cudaMemcpyKind { cudaMemcpyHostToHost, cudaMemcpyHostToDevice, cudaMemcpyDeviceToHost, cudaMemcpyDeviceToDevice };
static inline cudaError_t cudaDeviceSynchronize() { return cudaSuccess; }

/* ------------------------------------------------------------------------ arrays -- */
enum cudaChannelFormatKind { cudaChannelFormatKindSigned, cudaChannelFormatKindUnsigned, cudaChannelFormatKindFloat };
struct cudaChannelFormatDesc { int x, y, z, w; cudaChannelFormatKind f; };
template <typename T> struct shim_channel;
#define SHIM_CHANNEL(T, X, Y, Z, W, F)                                                                       \
    template <> struct shim_channel<T> { static cudaChannelFormatDesc get() { cudaChannelFormatDesc d = {X, Y, Z, W, F}; return d; } };
SHIM_CHANNEL(float, 32, 0, 0, 0, cudaChannelFormatKindFloat)
SHIM_CHANNEL(float2, 32, 32, 0, 0, cudaChannelFormatKindFloat)
SHIM_CHANNEL(float4, 32, 32, 32, 32, cudaChannelFormatKindFloat)
SHIM_CHANNEL(unsigned char, 8, 0, 0, 0, cudaChannelFormatKindUnsigned)
SHIM_CHANNEL(uchar2, 8, 8, 0, 0, cudaChannelFormatKindUnsigned)
#undef SHIM_CHANNEL
template <typename T> static inline cudaChannelFormatDesc cudaCreateChannelDesc() { return shim_channel<T>::get(); }

struct cudaExtent { size_t width, height, depth; };
static inline cudaExtent make_cudaExtent(size_t w, size_t h, size_t d) { cudaExtent e = {w, h, d}; return e; }
struct cudaPitchedPtr { void* ptr; size_t pitch, xsize, ysize; };
static inline cudaPitchedPtr make_cudaPitchedPtr(void* p, size_t pitch, size_t xs, size_t ys)
{
    cudaPitchedPtr r = {p, pitch, xs, ys};
    return r;
}

/* a host-memory array: x fastest, rows and slices packed */
struct cudaArray
{
    cudaChannelFormatDesc desc;
    size_t                w, h, d; /* h and d are at least 1 */
    size_t                elem;    /* bytes per texel */
    unsigned char*        data;
};
typedef cudaArray*       cudaArray_t;
typedef const cudaArray* cudaArray_const_t;

static inline cudaError_t shim_alloc_array(cudaArray_t* a, const cudaChannelFormatDesc* desc, size_t w, size_t h, size_t d)
{
    cudaArray* r = new cudaArray;
    r->desc = *desc;
    r->w = w;
    r->h = h ? h : 1;
    r->d = d ? d : 1;
    r->elem = (size_t)(desc->x + desc->y + desc->z + desc->w) / 8;
    r->data = (unsigned char*)calloc(r->w * r->h * r->d, r->elem);
    *a = r;
    return cudaSuccess;
}
static inline cudaError_t cudaMalloc3DArray(cudaArray_t* a, const cudaChannelFormatDesc* desc, cudaExtent e, unsigned int = 0)
{
    return shim_alloc_array(a, desc, e.width, e.height, e.depth);
}
static inline cudaError_t cudaMallocArray(cudaArray_t* a, const cudaChannelFormatDesc* desc, size_t w, size_t h = 0, unsigned int = 0)
{
    return shim_alloc_array(a, desc, w, h, 0);
}
static inline cudaError_t cudaFreeArray(cudaArray_t a)
{
    if (a) { free(a->data); delete a; }
    return cudaSuccess;
}

struct cudaPos { size_t x, y, z; };
struct cudaMemcpy3DParms
{
    cudaArray_t    srcArray;
    cudaPos        srcPos;
    cudaPitchedPtr srcPtr;
    cudaArray_t    dstArray;
    cudaPos        dstPos;
    cudaPitchedPtr dstPtr;
    cudaExtent     extent;
    cudaMemcpyKind kind;
};
/* host pitched pointer -> array, the one direction in use; with an array on one side the extent is in elements */
static inline cudaError_t cudaMemcpy3D(const cudaMemcpy3DParms* p)
{
    cudaArray*           a   = p->dstArray;
    const unsigned char* src = (const unsigned char*)p->srcPtr.ptr;
    size_t               row = p->extent.width * a->elem;
    for (size_t k = 0; k < p->extent.depth; k++)
        for (size_t j = 0; j < p->extent.height; j++)
            memcpy(a->data + (j + a->h * k) * a->w * a->elem, src + (j + p->srcPtr.ysize * k) * p->srcPtr.pitch, row);
    return cudaSuccess;
}
/* width in bytes, as documented */
static inline cudaError_t cudaMemcpy2DToArray(cudaArray_t a, size_t wo, size_t ho, const void* src, size_t spitch, size_t width,
                                              size_t height, cudaMemcpyKind)
{
    for (size_t j = 0; j < height; j++)
        memcpy(a->data + (j + ho) * a->w * a->elem + wo, (const unsigned char*)src + j * spitch, width);
    return cudaSuccess;
}
static inline cudaError_t cudaMemcpy2DToArrayAsync(cudaArray_t a, size_t wo, size_t ho, const void* src, size_t spitch, size_t width,
                                                   size_t height, cudaMemcpyKind k, void* = nullptr)
{
    return cudaMemcpy2DToArray(a, wo, ho, src, spitch, width, height, k);
}
static inline cudaError_t cudaMemcpyToArray(cudaArray_t a, size_t wo, size_t ho, const void* src, size_t count, cudaMemcpyKind)
{
    memcpy(a->data + ho * a->w * a->elem + wo, src, count);
    return cudaSuccess;
}
template <typename T>
static inline cudaError_t cudaMemcpyToSymbolAsync(T& symbol, const void* src, size_t count, size_t offset = 0,
                                                  cudaMemcpyKind = cudaMemcpyHostToDevice, void* = nullptr)
{
    memcpy((char*)&symbol + offset, src, count);
    return cudaSuccess;
}

/* ---------------------------------------------------------- the texture fetch rule -- */
enum cudaTextureAddressMode { cudaAddressModeWrap, cudaAddressModeClamp, cudaAddressModeMirror, cudaAddressModeBorder };
enum cudaTextureFilterMode { cudaFilterModePoint, cudaFilterModeLinear };
enum cudaTextureReadMode { cudaReadModeElementType, cudaReadModeNormalizedFloat };

static inline int shim_clampi(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }
/* linear: texel-centre split of pn * n - 0.5 (the scaling and the offset in one rounding), weight rounded to 8 bits */
static inline void shim_axis_linear(float pn, int n, int* i0, int* i1, int* w)
{
    float xb = fmaf(pn, (float)n, -0.5f);
    float fl = floorf(xb);
    float fr = xb - fl;
    int   i  = (int)fl;
    *w  = (int)fmaf(fr, 256.0f, 0.5f);
    *i0 = shim_clampi(i, n);
    *i1 = shim_clampi(i + 1, n);
}
/* point: floor of the texel coordinate, clamped */
static inline int shim_axis_point(float x, int n, int normalized)
{
    return shim_clampi((int)floorf(normalized ? x * (float)n : x), n);
}
#define SHIM_U8_TRI_SCALE 2.3374372e-10f /* fl(1 / (255 * 2^24)): the full-scale integer trilinear sum becomes exactly 1.0f */
#define SHIM_U8_SCALE 0.003921569f      /* fl(1 / 255) */
static inline float shim_lerp(float a, float b, float w) { return a * (1.0f - w) + b * w; }

/* ------------------------------------------------------- texture / surface objects -- */
enum cudaResourceType { cudaResourceTypeArray, cudaResourceTypeMipmappedArray, cudaResourceTypeLinear, cudaResourceTypePitch2D };
struct cudaResourceDesc
{
    cudaResourceType resType;
    union
    {
        struct { cudaArray_t array; } array;
        struct { void* devPtr; cudaChannelFormatDesc desc; size_t sizeInBytes; } linear;
    } res;
};
struct cudaTextureDesc
{
    cudaTextureAddressMode addressMode[3];
    cudaTextureFilterMode  filterMode;
    cudaTextureReadMode    readMode;
    int                    sRGB;
    float                  borderColor[4];
    int                    normalizedCoords;
    unsigned int           maxAnisotropy;
};
struct cudaResourceViewDesc;
struct shim_texobj { cudaArray_t array; cudaTextureDesc desc; };
typedef unsigned long long cudaTextureObject_t;
typedef unsigned long long cudaSurfaceObject_t;

static inline cudaError_t cudaCreateTextureObject(cudaTextureObject_t* t, const cudaResourceDesc* r, const cudaTextureDesc* d,
                                                  const cudaResourceViewDesc*)
{
    shim_texobj* o = new shim_texobj;
    o->array = r->res.array.array;
    o->desc  = *d;
    *t = (cudaTextureObject_t)(uintptr_t)o;
    return cudaSuccess;
}
static inline cudaError_t cudaDestroyTextureObject(cudaTextureObject_t t)
{
    delete (shim_texobj*)(uintptr_t)t;
    return cudaSuccess;
}
static inline cudaError_t cudaCreateSurfaceObject(cudaSurfaceObject_t* s, const cudaResourceDesc* r)
{
    *s = (cudaSurfaceObject_t)(uintptr_t)r->res.array.array;
    return cudaSuccess;
}
static inline cudaError_t cudaDestroySurfaceObject(cudaSurfaceObject_t) { return cudaSuccess; }

template <typename T> T tex3D(cudaTextureObject_t t, float x, float y, float z);

/* one channel: a uchar array read as normalised float, or a float array; linear or point */
template <>
inline float tex3D<float>(cudaTextureObject_t t, float x, float y, float z)
{
    const shim_texobj* o = (const shim_texobj*)(uintptr_t)t;
    const cudaArray*   a = o->array;
    int nx = (int)a->w, ny = (int)a->h, nz = (int)a->d;
    int i0, i1, j0, j1, k0, k1, wx, wy, wz;
    if (o->desc.filterMode == cudaFilterModeLinear)
    {
        shim_axis_linear(x, nx, &i0, &i1, &wx);
        shim_axis_linear(y, ny, &j0, &j1, &wy);
        shim_axis_linear(z, nz, &k0, &k1, &wz);
    }
    else
    {
        i0 = i1 = shim_axis_point(x, nx, 1);
        j0 = j1 = shim_axis_point(y, ny, 1);
        k0 = k1 = shim_axis_point(z, nz, 1);
        wx = wy = wz = 0;
    }
#define SHIM_IDX(i, j, k) ((size_t)(i) + (size_t)nx * ((size_t)(j) + (size_t)ny * (size_t)(k)))
    if (a->desc.f == cudaChannelFormatKindUnsigned)
    {
        const unsigned char* g = a->data;
        uint32_t t000 = g[SHIM_IDX(i0, j0, k0)], t100 = g[SHIM_IDX(i1, j0, k0)];
        uint32_t t010 = g[SHIM_IDX(i0, j1, k0)], t110 = g[SHIM_IDX(i1, j1, k0)];
        uint32_t t001 = g[SHIM_IDX(i0, j0, k1)], t101 = g[SHIM_IDX(i1, j0, k1)];
        uint32_t t011 = g[SHIM_IDX(i0, j1, k1)], t111 = g[SHIM_IDX(i1, j1, k1)];
        uint32_t ux = (uint32_t)wx, uy = (uint32_t)wy, uz = (uint32_t)wz;
        uint32_t x00 = t000 * (256u - ux) + t100 * ux;
        uint32_t x10 = t010 * (256u - ux) + t110 * ux;
        uint32_t x01 = t001 * (256u - ux) + t101 * ux;
        uint32_t x11 = t011 * (256u - ux) + t111 * ux;
        uint32_t y0  = x00 * (256u - uy) + x10 * uy;
        uint32_t y1  = x01 * (256u - uy) + x11 * uy;
        uint32_t v   = y0 * (256u - uz) + y1 * uz;
        return (float)v * SHIM_U8_TRI_SCALE;
    }
    const float* g = (const float*)a->data;
    float fx = (float)wx * (1.0f / 256.0f), fy = (float)wy * (1.0f / 256.0f), fz = (float)wz * (1.0f / 256.0f);
    float x00 = shim_lerp(g[SHIM_IDX(i0, j0, k0)], g[SHIM_IDX(i1, j0, k0)], fx);
    float x10 = shim_lerp(g[SHIM_IDX(i0, j1, k0)], g[SHIM_IDX(i1, j1, k0)], fx);
    float x01 = shim_lerp(g[SHIM_IDX(i0, j0, k1)], g[SHIM_IDX(i1, j0, k1)], fx);
    float x11 = shim_lerp(g[SHIM_IDX(i0, j1, k1)], g[SHIM_IDX(i1, j1, k1)], fx);
    float y0  = shim_lerp(x00, x10, fy);
    float y1  = shim_lerp(x01, x11, fy);
    return shim_lerp(y0, y1, fz);
}

/* two channels, point-sampled (the bound table): uchar2 read as normalised float, or float2 */
template <>
inline float2 tex3D<float2>(cudaTextureObject_t t, float x, float y, float z)
{
    const shim_texobj* o = (const shim_texobj*)(uintptr_t)t;
    const cudaArray*   a = o->array;
    int nx = (int)a->w, ny = (int)a->h, nz = (int)a->d;
    if (o->desc.filterMode != cudaFilterModePoint)
    {
        fprintf(stderr, "refshim: two-channel textures are point-sampled only\n");
        abort();
    }
    size_t idx = SHIM_IDX(shim_axis_point(x, nx, 1), shim_axis_point(y, ny, 1), shim_axis_point(z, nz, 1));
    if (a->desc.f == cudaChannelFormatKindUnsigned)
        return make_float2((float)a->data[2 * idx] * SHIM_U8_SCALE, (float)a->data[2 * idx + 1] * SHIM_U8_SCALE);
    const float* g = (const float*)a->data;
    return make_float2(g[2 * idx], g[2 * idx + 1]);
}
#undef SHIM_IDX

/* surfaces: x is a byte offset, as documented */
template <typename T>
static inline T surf3Dread(cudaSurfaceObject_t s, int xbytes, int y, int z)
{
    const cudaArray* a = (const cudaArray*)(uintptr_t)s;
    T v;
    memcpy(&v, a->data + ((size_t)y + a->h * (size_t)z) * a->w * a->elem + (size_t)xbytes, sizeof(T));
    return v;
}
template <typename T>
static inline void surf3Dwrite(T v, cudaSurfaceObject_t s, int xbytes, int y, int z)
{
    cudaArray* a = (cudaArray*)(uintptr_t)s;
    memcpy(a->data + ((size_t)y + a->h * (size_t)z) * a->w * a->elem + (size_t)xbytes, &v, sizeof(T));
}

/* --------------------------------------------------- legacy texture references -- */
struct textureReference
{
    int                    normalized;
    cudaTextureFilterMode  filterMode;
    cudaTextureAddressMode addressMode[3];
    cudaChannelFormatDesc  channelDesc;
    cudaArray_const_t      shim_array;
};
template <typename T, int Dim = 1, int Mode = cudaReadModeElementType>
struct texture : public textureReference
{
    /* CUDA's constructor: unnormalised coordinates, point filter, clamp addressing */
    texture(int norm = 0, cudaTextureFilterMode f = cudaFilterModePoint, cudaTextureAddressMode m = cudaAddressModeClamp)
    {
        normalized = norm;
        filterMode = f;
        addressMode[0] = addressMode[1] = addressMode[2] = m;
        channelDesc = cudaCreateChannelDesc<T>();
        shim_array = nullptr;
    }
};
template <typename T, int Dim, int Mode>
static inline cudaError_t cudaBindTextureToArray(const texture<T, Dim, Mode>* tex, cudaArray_const_t a, const cudaChannelFormatDesc*)
{
    const_cast<texture<T, Dim, Mode>*>(tex)->shim_array = a;
    return cudaSuccess;
}
template <typename T, int Dim, int Mode>
static inline cudaError_t cudaUnbindTexture(const texture<T, Dim, Mode>* tex)
{
    const_cast<texture<T, Dim, Mode>*>(tex)->shim_array = nullptr;
    return cudaSuccess;
}

static inline void shim_ref_check(const textureReference& t)
{
    if (t.filterMode != cudaFilterModePoint || t.addressMode[0] != cudaAddressModeClamp || t.addressMode[1] != cudaAddressModeClamp)
    {
        fprintf(stderr, "refshim: texture references are point-sampled with clamp addressing only\n");
        abort();
    }
}
struct shim_element_type; /* "return the texture's own element type" */
template <typename R, typename T> struct shim_ret { typedef R type; };
template <typename T> struct shim_ret<shim_element_type, T> { typedef T type; };

/* tex1D(t, x) and tex1D<T>(t, x) */
template <typename R = shim_element_type, typename T, int Mode>
static inline typename shim_ret<R, T>::type tex1D(const texture<T, 1, Mode>& t, float x)
{
    shim_ref_check(t);
    const cudaArray* a = t.shim_array;
    return ((const T*)a->data)[shim_axis_point(x, (int)a->w, t.normalized)];
}
/* tex2D(t, x, y) and tex2D<T>(t, x, y): one template, the return type defaulted (two overloads would be ambiguous) */
template <typename R = shim_element_type, typename T, int Mode>
static inline typename shim_ret<R, T>::type tex2D(const texture<T, 2, Mode>& t, float x, float y)
{
    shim_ref_check(t);
    const cudaArray* a = t.shim_array;
    int i = shim_axis_point(x, (int)a->w, t.normalized);
    int j = shim_axis_point(y, (int)a->h, t.normalized);
    return ((const T*)a->data)[(size_t)i + a->w * (size_t)j];
}

/* ------------------------------------------------------------------------ launches -- */
/* kernel<<<grid, block>>>(args) is rewritten by oracle/Makefile into SHIM_LAUNCH(kernel, grid, block)(args): every thread of
 * every block in turn, serially. */
template <typename F>
struct shim_launcher
{
    dim3 grid, block;
    F    f;
    template <typename... A>
    void operator()(A&&... args)
    {
        gridDim  = grid;
        blockDim = block;
        for (unsigned bz = 0; bz < grid.z; bz++)
            for (unsigned by = 0; by < grid.y; by++)
                for (unsigned bx = 0; bx < grid.x; bx++)
                    for (unsigned tz = 0; tz < block.z; tz++)
                        for (unsigned ty = 0; ty < block.y; ty++)
                            for (unsigned tx = 0; tx < block.x; tx++)
                            {
                                blockIdx  = make_uint3(bx, by, bz);
                                threadIdx = make_uint3(tx, ty, tz);
                                f(args...);
                            }
    }
};
template <typename F>
static inline shim_launcher<F> shim_make_launcher(dim3 grid, dim3 block, F f)
{
    shim_launcher<F> l = {grid, block, f};
    return l;
}
#define SHIM_LAUNCH(kernel, ...) shim_make_launcher(__VA_ARGS__, [](auto&&... shim_a) { kernel(shim_a...); })

#endif
