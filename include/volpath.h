/* volpath.h -- C ABI of libvolpath_hip.so: the MI355X-native replacement for the device
 * translation unit of RNG65536/CUDA-volpath (src/volumeRender_kernel.cu).
 *
 * Part 1 re-exports, under their original names, the 14 extern "C" entry points the reference
 * host binds (src/volumeRender.cpp:117-128 and :347-356); a maintainer swaps the CUDA TU for this
 * library and relinks.  Part 2 is additive: batched rendering, estimator / RNG
 * selection, pixel-tile sharding for multi-GPU, counters, and raw device-memory helpers so that a
 * C / ctypes caller needs no other GPU runtime binding.
 *
 * Only plain C types cross the boundary.  The CUDA vector types of the reference map onto the
 * layout-identical PODs below (float3 = 3 floats, float4 = 4 floats 16-byte aligned,
 * dim3 = 3 x uint32, cudaExtent = 3 x size_t).
 *
 * Error behaviour: Part 1 functions return void and, exactly like the reference
 * (checkCudaErrors -> exit(EXIT_FAILURE), src/cuda/helper_cuda.h:566-579; null volume -> exit(1),
 * kernel.cu:360-364), print a diagnostic and exit the process on failure.  Part 2 functions
 * return 0 on success or a negative VP_E* code and leave a message in vp_last_error().
 * There is NO CPU fallback anywhere: without a usable gfx950 device every entry point fails.
 */
#ifndef VOLPATH_H
#define VOLPATH_H

#include <stddef.h>
#include <stdint.h>
#ifndef __cplusplus
#include <stdbool.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef struct { float x, y, z; } vp_float3;
typedef struct { float x, y, z, w; } vp_float4;
typedef struct { uint32_t x, y, z; } vp_dim3;
typedef struct { size_t width, height, depth; } vp_extent;

/* src/param.h:4-12 -- 44 bytes, passed by value to the reference kernels */
#ifndef VOLPATH_PARAM_DEFINED
#define VOLPATH_PARAM_DEFINED
typedef struct Param
{
    unsigned int width, height;
    float        density, brightness;
    vp_float3    albedo;
    float        g;
    vp_float3    sigma_t;
} Param;
#endif

/* ------------------------------------------------------------------------------------------
 * Part 1: the reference's kernel-TU interface
 * ------------------------------------------------------------------------------------------ */

/* kernel.cu:354-420 (declared host.cpp:349-353).  Uploads the density volume (uchar if
 * `quantized`, else float; x fastest), builds the local (max,min) bound table (replaces the
 * call-back into host.cpp:1269-1280) and publishes the descriptors.  boxmin/boxmax may be NULL
 * (box = +-(1, Ny/Nx, Nz/Nx)).  Caller keeps ownership of h_volume.  NULL volume -> exit(1). */
void init_cuda(void* h_volume, vp_extent volumeSize, bool quantized, const vp_float3* boxmin,
               const vp_float3* boxmax);
/* kernel.cu:422-439 (host.cpp:354): point / trilinear density sampling */
void set_texture_filter_mode(bool bLinearFilter);
/* kernel.cu:441-451 (host.cpp:355) */
void free_cuda_buffers(void);
/* kernel.cu:526-553 (host.cpp:128): optical depth toward light_dir[3], dt = 0.001 */
void precompute_opacity(const float* light_dir);
/* kernel.cu:1072-1229 (host.cpp:125): row-major float4 lat-long map, row 0 = zenith; copied */
void init_envmap(const vp_float4* HDRmap, int width, int height);
/* kernel.cu:1231-1250 (host.cpp:126) */
void free_envmap(void);
/* kernel.cu:1269-1283 (host.cpp:127): dir[3], disc radiance power[3] */
void set_sun(float* sun_dir, float* sun_power);
/* kernel.cu:2320-2328 (host.cpp:119-120): row-major 3x4, sizeofMatrix = 48 */
void copy_inv_view_matrix(float* invViewMatrix, size_t sizeofMatrix);
void copy_inv_model_matrix(float* invModelMatrix, size_t sizeofMatrix);
/* kernel.cu:2330-2331 (host.cpp:121-122): no-ops in the reference, no-ops here */
void init_rng(vp_dim3 gridSize, vp_dim3 blockSize, int width, int height);
void free_rng(void);
/* kernel.cu:2364-2370 (host.cpp:117-118): adds ONE sample per pixel of frame `spp` into the
 * caller-owned device buffer d_output[width*height]; asynchronous on the library stream.
 * gridSize/blockSize are accepted for signature compatibility and ignored (the launch shape is
 * the library's business).  In C++ the last parameter is `const Param&`, same ABI. */
#ifdef __cplusplus
void render_kernel(vp_dim3 gridSize, vp_dim3 blockSize, vp_float4* d_output, int spp, const Param& p);
#else
void render_kernel(vp_dim3 gridSize, vp_dim3 blockSize, vp_float4* d_output, int spp, const Param* p);
#endif
/* kernel.cu:2333-2346 / :2348-2362 (host.cpp:123-124): device pointers, in place allowed */
void scale(vp_float4* dst, vp_float4* src, int size, float scale);
void gamma_correct(vp_float4* dst, vp_float4* src, int size, float scale, float gamma);

/* ------------------------------------------------------------------------------------------
 * Part 2: additive interface
 * ------------------------------------------------------------------------------------------ */
enum
{
    VP_OK          = 0,
    VP_E_NODEVICE  = -1, /* no gfx950 device / HIP runtime error */
    VP_E_STATE     = -2, /* call order (e.g. render before init_cuda / init_envmap) */
    VP_E_ARG       = -3,
    VP_E_NOOPACITY = -4, /* frame > 10 with the decomposition estimator needs precompute_opacity */
    VP_E_NOMEM     = -5  /* device memory exhausted (hipErrorOutOfMemory) */
};

enum { VP_EST_GLOBAL = 0, /* __d_render, kernel.cu:1285-1591: global majorant (BASELINE config 2) */
       VP_EST_DECOMP = 1, /* __d_render_bounded_decomp, kernel.cu:1958-2318: the reference's live kernel */
       VP_EST_BOUNDED = 2 /* __d_render_bounded, kernel.cu:1667-1952: local majorant, no control component,
                             800 tracked segments at most, heat = segments * 0.001, never reads the opacity volume */ };
enum { VP_RNG_SAMPLERH = 0, /* src/sampler.h bit-compatible streams: THE PARITY MODE -- the reference's generator, seeding and order of
                               draws (sampler.h:3-46; Tr_spectral draws from the path's own sequential stream), i.e. what a run of the
                               reference computes sample for sample up to the arithmetic contract of DESIGN.md section 2 */
       VP_RNG_PHILOX   = 1, /* Philox2x32-10, counter = (draw/2, x<<16|y), key = (frame ^ key0) + key1.  SAME ESTIMATOR, BUILD-DEFINED
                               STREAM (north_star: a counter-based generator replaces sampler.h): same free flights, collision tests and
                               transmittance flags, but shadow rays draw from sub-streams -- counter word 0 = 0x80000000 +
                               ((2 * depth + ray) << 20) + step, 2^20 pairs each: a shadow ray of more steps (a majorant above 3e5 per
                               unit length; the default medium has 800) would run into the next sub-stream -- and the phase function is
                               sampled before the shadow ray.  Defined by oracle/vp_oracle.c; tied to the sampler.h images statistically
                               (tests/test_parity_gpu.py::test_full_size_estimators_and_builds_converge_to_one_image) */
       VP_RNG_PHILOX7  = 2  /* Philox2x32-7 (the fewest rounds Random123 documents as Crush-resistant), same counter / key / sub-streams;
                               built for the shipped configuration (spectral tracking, passive environment) */ };

const char* vp_last_error(void);
const char* vp_version(void);
int  vp_device_count(void);
int  vp_set_device(int device);       /* device of the CURRENT context; before its first GPU call; default 0 */

/* Contexts.  The reference keeps its scene in file-scope statics and __constant__ symbols: one scene, one device per process
 * (kernel.cu:148-151, :621-629; cudaSetDevice(0) src/denoiser.cpp:94-97).  Here all of that state lives in a context.  Every
 * entry point of this header -- Part 1 included -- acts on the calling thread's current context; a thread that never set one
 * uses the process-wide default context, so the reference host binds the 14 Part-1 symbols unchanged.  One context per GPU
 * gives a single-process multi-GPU host (host/main.cpp --gpus N: N contexts, pixel tiles dealt by vp_set_shard, one RCCL
 * reduce).  A context is not thread-safe; different contexts may be driven from different threads. */
typedef struct vp_ctx vp_ctx;
vp_ctx* vp_ctx_create(int device);         /* NULL on failure (vp_last_error of the current context says why) */
int     vp_ctx_destroy(vp_ctx* ctx);       /* frees its device memory; the current context becomes the default one if it was ctx */
int     vp_ctx_set_current(vp_ctx* ctx);   /* NULL = the default context */
vp_ctx* vp_ctx_get_current(void);          /* NULL while the default context is current */
int     vp_ctx_device(void);               /* device index of the current context */
/* dst[i] += src[i] for n float4 on the current context's stream (device pointers of ITS device): sums per-shard accumulators
 * where no collective is available (several contexts on one GPU) */
int     vp_accumulate(vp_float4* dst, const vp_float4* src, size_t n);
int  vp_set_stream(void* hip_stream); /* hipStream_t to launch on; NULL = library-owned stream */
void* vp_get_stream(void);            /* the hipStream_t the current context launches on (for a collective queued behind a render) */
int  vp_synchronize(void);

int vp_set_estimator(int est);                         /* default VP_EST_DECOMP */
int vp_set_rng(int mode, uint32_t key0, uint32_t key1); /* default VP_RNG_SAMPLERH */
/* Environment lighting.  VP_ENV_PASSIVE is the reference's shipped build (PASSIVE_ENVMAP 1, kernel.cu:21): escaping paths
 * look the environment up.  VP_ENV_MIS is its compiled-out alternative: luminance CDFs built in init_envmap
 * (kernel.cu:1144-1210) and one-sample MIS between phase-function and environment sampling after each collision
 * (kernel.cu:2220-2297, MULT_PDF 0, PRE_WARP 1); only unscattered paths then see the environment directly. */
/* Collision sampling.  VP_TRACK_SPECTRAL is the reference's shipped build (SPECTRAL_TRACKING 1, kernel.cu:15-34): one path
 * for the three channels with history-aware collision probabilities.  The other two are its compiled-out alternatives:
 * VP_TRACK_SCALAR = SPECTRAL_TRACKING 0 (one extinction coefficient = density, throughput *= albedo per collision, scalar
 * shadow rays), VP_TRACK_MULTI_CHANNEL = MULTI_CHANNEL 1 (the same with coefficient density * sigma_t[channel], the channel
 * drawn per sample and written times three, kernel.cu:1993-1994, :2311-2313).  Both ignore the local bound (kernel.cu:2063)
 * and exist with VP_ENV_PASSIVE only. */
enum { VP_TRACK_SPECTRAL = 0, VP_TRACK_SCALAR = 1, VP_TRACK_MULTI_CHANNEL = 2 };
int vp_set_tracking(int mode);                         /* default VP_TRACK_SPECTRAL */
/* render_kernel renders up to max_frames consecutive frames per launch when the host asks for frame f right after f-1 with
 * unchanged state, stages them, and serves the following calls from the staged frames (bit-identical to one launch per
 * frame).  The first frame of a run is rendered alone, then batches of 32, 64, ... frames, each with its
 * successor queued behind it; beyond 64 a batch is at most half of what the run has accumulated.  A setter or a camera move
 * stops the batches in flight within a fraction of a millisecond.  Default 256; 0 or 1 = one launch per call.  Env: VP_LOOKAHEAD. */
int vp_set_lookahead(int max_frames);
enum { VP_ENV_PASSIVE = 0, VP_ENV_MIS = 1 };
int vp_set_envmap_sampling(int mode);                  /* default VP_ENV_PASSIVE */
/* Arithmetic of the integrator.  VP_ARITH_EXACT, the default, is the parity contract: correctly rounded
 * binary32 divides and roots, the Cephes polynomials of vp_math.h, no contraction -- bit for bit the CPU oracle's.  VP_ARITH_FAST
 * trades the last ulps for issue slots: the integrator's logarithm, exponential, divides, reciprocals, roots, normalisations and
 * the phase function's sine and cosine become the hardware's single instructions (v_log_f32, v_exp_f32, v_rcp_f32, v_sqrt_f32,
 * v_rsq_f32, v_sin_f32, v_cos_f32), each written out in the source, nothing left to the compiler.  It is deterministic like the
 * exact mode -- two runs, render_frames against render_kernel's look-ahead, a sharded render against a whole one give the same
 * bits -- but it is no longer the oracle's, and the same estimator's result moves within the tolerance below.
 *   Built for: VP_RNG_PHILOX / VP_RNG_PHILOX7, VP_TRACK_SPECTRAL, VP_ENV_PASSIVE, VP_EST_GLOBAL / VP_EST_DECOMP, uchar and float
 *   volumes, work counters off.  Any other combination makes the render fail with VP_E_STATE (the context stays usable).
 *   Unchanged by the mode (exact in both): the per-pixel tables and certificates, the pixels whose camera ray misses the box or
 *   meets certified-empty cells only (pixel classes 1 and 2 of vp_get_pixel_table: bit-identical), scale and gamma_correct.
 *   Tolerance (mean-radiance images I of N frames, the same stream and keys in both modes): the relative L2 distance
 *   ||I_fast - I_exact||_2 / ||I_exact||_2 over the whole image is at most VP_ARITH_FAST_REL_L2 = 2e-3 at N = 1024 on BASELINE
 *   configs 2 and 3 and the chromatic c4s -- measured 4.7e-4, 3.7e-4 and 5.5e-4: the bound is 3.6 times the largest (c4f, 256
 *   frames: 1.5e-3) --, and the image mean moves by less than 2e-3 per channel (measured: below 3e-6).  The fast mode changes
 *   95-99 % of the general pixels' samples; it is unbiased (an estimator of the same image), not equal.  The hardware instructions
 *   flush denormal inputs: a sample whose collision weight comes out infinite that way (a path whose throughput fell below
 *   2^-126) is written as 0.
 *   Speed (kernel time, 1024 frames): +12 % (c3) to +20 % (c2) on the benchmark workloads (profiles/experiments/r06_arith_fast.txt).
 * vp_set_arithmetic is per context; it checks its argument before it touches the device and stops render_kernel's look-ahead
 * batches in flight (frames staged in one mode are never served in the other). */
enum { VP_ARITH_EXACT = 0, VP_ARITH_FAST = 1 };
#define VP_ARITH_FAST_REL_L2 2e-3
int vp_set_arithmetic(int mode);                       /* default VP_ARITH_EXACT */
/* Anti-aliasing: stratified sub-pixel camera rays.  A sub-pixel factor S in {1, 2, 4, 8}, m = log2 S, per
 * context, default 1 (env VP_SUBPIXEL=<s> sets the default of new contexts).  THE DEFINITION:
 *   With factor S, the sample of pixel (x, y) in frame f of a W x H image is, bit for bit, the sample that the same context with
 *   S = 1 computes for pixel (S x + i, S y + j) in frame f of the S W x S H image -- same Param otherwise, same camera, stream, keys,
 *   estimator, arithmetic mode.
 * The camera ray, the random stream and every per-pixel certificate are the fine pixel's; only the accumulator address is the coarse
 * pixel's, and samples are still added per pixel in frame order.  The fine image has the same field of view and aspect
 * (u = (2 px - W) / W, v = (2 py - H) / W), so the S^2 fine rays tile the pixel's footprint: a box-filtered pixel.  Pixel x of the
 * reference's camera is the point u = (2x - W) / W, the LEFT EDGE of the cell [x, x+1); the fine rays sample that cell at offsets
 * i / S, j / S.  Against an S = 1 render the image content therefore moves by (S - 1) / (2 S) of a pixel: the reference's own pixel
 * convention made visible, not an error.
 * (i, j) is a pure integer function of (x, y, f, S), independent of the keys (vp_subpixel_offset computes it on the host):
 *   h = wang_hash(((x << 16) | y) ^ 0x9E3779B9)     wang_hash: sampler.h:3-11
 *   k = ((uint32) f + h) mod S^2                     uint32 wrap-around arithmetic
 *   r = k with its 2m bits reversed                  bit b -> bit 2m-1-b
 *   i = bits 0, 2, 4, ... of r packed into m bits,   j = bits 1, 3, 5, ... of r
 * Any 4^t consecutive frames, t <= m, hit each of the 2^t x 2^t sub-squares of the pixel exactly once; S^2 frames cover the lattice.
 * S = 1 gives (0, 0) always: the identity, not a bit of the default behaviour changes.
 *   Built for: every estimator, stream, tracking and environment mode, both arithmetic modes, uchar and float volumes, shards,
 *   vp_render_frames and render_kernel (look-ahead, pipeline) -- with work counters off: a render with S > 1 while counters are enabled
 *   fails with VP_E_STATE (the context stays usable).
 *   Limits: the fine coordinates go into the 16-bit halves of x << 16 | y: a render with S W > 65536 or S H > 65536 fails with VP_E_ARG.
 *   The per-pixel table is the fine image's (S^2 x 32 bytes per pixel: 245 MB at 800x600, S = 4): VP_E_NOMEM where it does not fit.
 *   vp_get_pixel_table(P) keeps describing exactly the image P names; vp_get_pixel_lists returns the lists of the current factor: a pixel
 *   is general if any of its S^2 fine pixels is (or if they mix the other two classes), box-missing if all of them are, light if all are.
 * vp_set_subpixel checks its argument before it touches the device, stops look-ahead batches in flight, waits for pipelined launches
 * and drops the per-view tables and pixel lists.  vp_subpixel_offset needs no device; x, y <= 65535, frame >= 0. */
#define VP_SUBPIXEL_MAX 8
int vp_set_subpixel(int s);                            /* default 1 (VP_SUBPIXEL) */
int vp_get_subpixel(void);
int vp_subpixel_offset(unsigned x, unsigned y, int frame, int s, int* i, int* j);
/* test hook: the tables of the current environment: cdf_y[h], cdf_x[w*h] (row CDFs), HDRpdfnormAlt; any may be NULL */
int vp_get_env_tables(float* cdf_y, float* cdf_x, float* pdfnorm_alt);
/* brick edge (power of two, 1 = the reference's per-voxel table) used by the NEXT init_cuda */
int vp_set_bound_brick(int brick);

/* Volume formats.  vp_init_volume is init_cuda with the format named and an error code instead of exit():
 * VP_VOL_U8 is init_cuda(quantized = true), VP_VOL_F32 init_cuda(quantized = false), the same code path, the same bits.
 * VP_VOL_F16: h_volume holds IEEE binary16 values (x fastest).  THE DEFINITION: a binary16 volume h renders, in every mode, exactly
 * what the float volume widen(h) renders, widen = each element converted to binary32 (exact; subnormal halves are NOT flushed) --
 * images, work counters, the bound table (float (max, min) pairs of the widened values), the opacity table, pixel classes and every
 * certificate.  The filter is the float filter applied to the widened taps.  Only the stored cell differs: 8 halves in 16 bytes
 * instead of 8 floats in 32, one 16-byte load per fetch instead of two; the forms that exist for uchar volumes alone (the brick table in
 * LDS, the staged opacity march, the segment table, local-majorant exit flights) stay theirs.  Finite values are the contract.
 * VP_E_ARG before the device is touched: NULL volume, unknown format, an empty extent.  boxmin / boxmax may be NULL as in init_cuda. */
enum { VP_VOL_U8 = 0, VP_VOL_F32 = 1, VP_VOL_F16 = 2 };
int vp_init_volume(const void* h_volume, vp_extent ext, int format, const vp_float3* bmin, const vp_float3* bmax);
/* what the current volume occupies: cell_bytes per packed 2x2x2 neighbourhood cell (8, 32, 16), cells_bytes of them on the device
 * (nx ny nz cells; with VP_CELL_BRICKS=1 the 4x4x4-brick-padded count).  VP_E_STATE without a volume. */
typedef struct { int format; int nx, ny, nz; int cell_bytes; uint64_t cells_bytes; } vp_volume_info;
int vp_get_volume_info(vp_volume_info* out);
/* Pixel-tile sharding: this context renders the 8x8 pixel tiles (tx, ty) with vp_tile_owner(tx, ty, world) == rank: within
 * a tile row every world-th tile, the rows shifted against each other by a hash of the row index, so that neither columns
 * nor rows nor diagonals of the image belong to one rank whatever tiles_x % world is. */
int vp_set_shard(int rank, int world);
int vp_tile_owner(unsigned tx, unsigned ty, int world);

/* Adds frames [first_frame, first_frame + n_frames) into d_output[width*height] (device).
 * Per pixel the samples are added in frame order, so the result equals n_frames successive
 * render_kernel calls bit for bit.  Asynchronous. */
int vp_render_frames(vp_float4* d_output, int first_frame, int n_frames, const Param* p);

/* Per-pixel noise estimates and adaptive sampling.  THE DEFINITION:
 * d_stats is a caller-owned device buffer of width * height records, zeroed by the caller (vp_memset), indexed like the accumulator.
 * For every sample v (the float4 that is added to the accumulator) that a stats-carrying render adds to pixel i, record i receives
 *   y = (0.2126f * v.x + 0.7152f * v.y) + 0.0722f * v.z      in binary32, no contraction
 *   sum_y  += (double)y
 *   sum_y2 += (double)y * (double)y
 *   n      += 1
 * Per pixel the samples are added in frame order, like the accumulator, so the sums are bit-defined.
 *
 * vp_render_frames_stats: a uniform render with statistics.  d_output ends up bit-identical to what vp_render_frames writes.  It
 * never reads or sets `flags`: a record's FROZEN bit stays as the caller left it, and frozen pixels are sampled like any other.  It
 * touches only the records of the pixels the context owns (vp_set_shard).
 *
 * vp_render_adaptive: a pixel is ACTIVE while its record's FROZEN bit is clear.  The frozen set is exactly what d_stats says: there
 * is no hidden per-context state, so a second call continues a first one.  With B = round_frames, round k = 0, 1, ... covers frames
 * [first_frame + k B, first_frame + min((k + 1) B, max_frames)).  Every owned pixel that is active at the start of a round receives
 * all frames of the round, in frame order; a frozen pixel receives none.  After the round each pixel that was active in it is frozen
 * iff n >= min_frames and the criterion holds, evaluated in binary64, no contraction, operations in the order written, with
 * nd = (double)n, tol = (double)rel_tol, fl = (double)floor_y (the binary32 arguments widened):
 *   lhs = nd * sum_y2 - sum_y * sum_y
 *   m   = max(sum_y, nd * fl)                                 max(a, b) is a > b ? a : b
 *   rhs = ((tol * tol) * (nd - 1.0)) * (m * m)
 *   frozen  <=>  lhs <= rhs                                   false when either side is NaN
 * i.e. "the estimated standard error of the mean luminance is at most rel_tol * max(mean, floor_y)", cleared of divisions and
 * roots: multiplies, adds and a compare only, so a float64 restatement gives the same bits.  The call ends when no owned pixel is
 * active or the frames are used up.  Freezing is permanent.  The set of samples a pixel receives depends on nothing but this
 * definition: not on launch sizes, staging caps, pixel classes, shards or the pipeline.  `result` (may be NULL) reports the samples
 * added by the call, the rounds it ran, the owned pixels still active at its end and the frames its longest-running pixel received
 * from it (the frames of the rounds run).
 *   Refused before the device is touched, with VP_E_ARG: NULL pointers (result excepted), max_frames <= 0 or first_frame < 0,
 *   min_frames < 2, round_frames < 1, rel_tol or floor_y negative or NaN.  VP_E_STATE: work counters enabled (the context stays
 *   usable).  VP_E_NOOPACITY as vp_render_frames would give for frame first_frame + max_frames - 1.
 *   Built for: every estimator, stream, tracking and environment mode, both arithmetic modes, uchar and float volumes, shards
 *   (each context its own pixels; reducing statistics across processes is the caller's business; the records of sharded contexts on ONE
 *   device add up with vp_accumulate_stats, below) and every sub-pixel factor.
 *   Rounds are serial -- round k + 1 needs round k's decisions -- and run on the context's stream: the call stops look-ahead
 *   batches, waits for pipelined launches and reads three counts back per round (it synchronises).  The cached pixel lists of the
 *   view and vp_get_pixel_lists are never modified by it.
 * What adaptive sampling is and is not: it stops sampling a pixel when the ESTIMATE of its error is small.  The stopping rule looks
 * at the estimate it stops, so the result carries the small bias every such scheme has (a pixel whose first samples happen to agree
 * is stopped early and keeps that mean); min_frames is the guard against a pixel freezing on a lucky start.  The image of an
 * adaptive render is sum / n per pixel (vp_scale_by_count), not the sum times one factor.  The exact-parity product -- bit for bit the
 * reference's estimator, every pixel the same frames -- stays vp_render_frames.
 *
 * Output stage (the reference's `scale` assumes one count for all pixels).  vp_scale_by_count: each channel of dst[i] is
 * src[i].c * (scale / (float)n_i), the divide binary32 and correctly rounded; n_i == 0 gives 0; in place is allowed.
 * vp_stats_rel_error, the noise map: dst[i] = sqrt(max(lhs, 0) / (nd * nd * (nd - 1))) / max(sum_y / nd, fl), computed in binary64
 * and rounded to binary32; n < 2 gives 0.  A diagnostic image. */
typedef struct { double sum_y, sum_y2; uint32_t n, flags; } vp_pixel_stats;   /* 24 bytes */
#define VP_STATS_FROZEN 1u
typedef struct { float rel_tol, floor_y; int min_frames, round_frames; } vp_adaptive;
typedef struct { uint64_t samples; uint32_t rounds, active_left, frames_used; } vp_adaptive_result;
int vp_render_frames_stats(vp_float4* d_output, vp_pixel_stats* d_stats, int first_frame, int n_frames, const Param* p);
int vp_render_adaptive(vp_float4* d_output, vp_pixel_stats* d_stats, int first_frame, int max_frames, const Param* p,
                       const vp_adaptive* a, vp_adaptive_result* result);
int vp_scale_by_count(vp_float4* dst, const vp_float4* src, const vp_pixel_stats* d_stats, int size, float scale);
int vp_stats_rel_error(float* dst, const vp_pixel_stats* d_stats, int size, float floor_y);

/* vp_denoise: a variance-guided non-local-means filter for the output stage (the reference's other output stage, scaledOutput ->
 * denoise -> gamma_correct, is OptiX; this is what stands in its place: the NL-means filter with a variance-cancelled patch distance
 * of Rousselle, Knaus and Zwicker 2012, which needs exactly the per-pixel records above).  `src` is an accumulator of sums and
 * d_stats its records; dst receives a MEAN image (the division by the count is part of the call).  The pair (guide, d_guide_stats)
 * supplies the weights, `src` the colours; both NULL: the guide is src itself.  Cross-filtering two half-buffers is a
 * pipeline of existing calls: vp_render_frames_halves_stats, two filter calls with the roles swapped, vp_merge_halves (below).
 *   Everything is binary32, no contraction, operations in the order written, unless marked binary64.  min(a, b) is a < b ? a : b,
 *   max(a, b) is a > b ? a : b, clamp() clamps a coordinate pair into the image.  Per pixel a of a pair (accumulator A, records T):
 *     s_a = T.n == 0 ? 0 : 1.0f / (float)T.n          c_a = A.xyz * s_a   (the bits vp_scale_by_count(..., 1.0f) writes)
 *     y_a = (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z                                          (of the guide pair)
 *     v_a = variance of the mean luminance from the guide's records, binary64 rounded once:  nd = (double)n;
 *           lhs = nd * sum_y2 - sum_y * sum_y;  v = (float)(max(lhs, 0.0) / (nd * nd * (nd - 1.0)));  n < 2 gives 0.  `flags` is never read.
 *   Pair term for unclamped positions a, b with a' = clamp(a), b' = clamp(b), eps = 1e-20f, k2 = k * k:
 *     e(a, b) = ((y_a' - y_b') * (y_a' - y_b') - (v_a' + min(v_b', v_a'))) / (eps + k2 * (v_a' + v_b'))
 *   Patch distance of pixel p and offset o, F = patch: row sums first, for ty = -F..F
 *     row_ty = sum over tx = -F..F, left to right, starting from 0.0f, of e(p + (tx, ty), p + o + (tx, ty))
 *     D = sum over ty, top to bottom, starting from 0.0f, of row_ty;   D = max(D * (1.0f / (float)((2F+1) * (2F+1))), 0.0f)
 *     w = expf_(-D), the exact-mode exponential of the integrator whatever vp_set_arithmetic says (as for scale and gamma_correct)
 *   dst[p].xyz = (sum over o of w * c_(p+o)) / (sum over o of w): both sums start from 0.0f and run over oy = -R..R (outer) and
 *   ox = -R..R (inner), R = radius; offsets whose p + o lies outside the image are skipped; per channel num = num + w * c; one
 *   correctly rounded divide per channel.  The two sum orders are fixed so that a shared pass over a tile and a per-thread loop give
 *   the same bits (running sums would not, and are not used).
 *   Exceptions: where the guide's v_p == 0 -- a noise-free or unmeasured pixel, every per-pixel-constant class -- dst[p].xyz = c_p,
 *   unfiltered.  dst[p].w = src[p].w * s_p always: the heat channel is never filtered.
 *   Inputs are assumed finite and small enough that v_a + v_b and k2 * (v_a + v_b) stay finite: every variance of the mean at most
 *   1.7e38 / max(1, k2) -- per-sample luminances up to about 1e19 / max(1, k) are safe.  Then e is no NaN and e >= -1 / k2, the centre
 *   weight is exactly 1 and the denominator is >= 1.  In that range d * d may overflow: e = +inf and w = 0, as it should be.  Beyond
 *   it e is (x - inf) / inf; the clamp at 0 makes D = 0 of a NaN (NaN > 0 is false), so dst still holds no NaN, but such an offset is
 *   mixed in with weight 1: an answer without meaning.  The running sums stay finite while (2R+1)^2 |c| does.
 *   Refused with VP_E_ARG before the device is touched: NULL dst, src, d_stats or dp; exactly one of the two guide pointers; dst == src
 *   or dst == guide (the call reads neighbours: in place is not possible); width or height < 1; radius outside
 *   0..VP_DENOISE_MAX_RADIUS; patch outside 0..VP_DENOISE_MAX_PATCH; k not finite or not > 0.
 *   Needs no scene (it works before init_cuda, like scale); runs asynchronously on the context's stream, behind the renders queued
 *   there; never synchronises.
 * What this is and is not: the filter sees LUMINANCE variance only -- purely chromatic noise is invisible to it.  Like every such
 * filter it trades variance for bias.  Weights taken from the buffer they filter are correlated with it: the guide pair is the
 * remedy.  The variance estimates themselves are not pre-filtered (vp_denoise_var, below, takes ones that are).  The exact-parity product stays vp_render_frames plus scale.
 * vp_set_denoise_form (test hook): 0 = one workgroup per pixel tile, (y, v), the colours and the pair terms of an offset shared through
 * LDS (default); 1 = one thread per pixel from global memory.  The same bits.  vp_last_denoise_form: the form of the last call. */
typedef struct { int radius, patch; float k; } vp_denoise_params;   /* search window (2R+1)^2, patch (2F+1)^2, strength */
#define VP_DENOISE_MAX_RADIUS 10
#define VP_DENOISE_MAX_PATCH  3
int vp_denoise(vp_float4* dst, const vp_float4* src, const vp_pixel_stats* d_stats,
               const vp_float4* guide, const vp_pixel_stats* d_guide_stats,      /* both NULL: guide = src */
               int width, int height, const vp_denoise_params* dp);
int vp_set_denoise_form(int form);
int vp_last_denoise_form(void);

/* vp_denoise_guided: vp_denoise with the weight of an offset cut by a second distance, computed from noise-free feature planes
 * (Rousselle, Manzi and Zwicker 2013: the weight is the smaller of the colour weight and the feature weight).  The planes are
 * meant to be vp_render_features' (below); any vp_float4 image of the size of src serves.  DESIGN.md section 2.13.
 *   The definition is vp_denoise's, word for word, with one change to the weight of an offset.  Let p be a pixel and o an offset
 *   with q = p + o inside the image (offsets that leave the image are skipped as before: no feature is read at a clamped position),
 *   and D vp_denoise's patch distance after the scaling by 1 / (2F+1)^2 and the clamp at 0.  Binary32, one rounding per operation,
 *   no contraction, in the order written:
 *     g_j = 1.0f / ((2.0f * sigma_j) * sigma_j)        once per call, on the host; the kernel receives it as it is
 *     fa  = features[j].plane[p].channel_j             fb = features[j].plane[q].channel_j
 *     t_j = (fa == fb) ? 0.0f : ((fa - fb) * (fa - fb)) * g_j
 *     Df  = 0.0f;  Df = Df + t_j  for j = 0 .. n_features-1 in order
 *     Dg  = Df > D ? Df : D
 *     w   = expf_(-Dg), the exact-mode exponential whatever vp_set_arithmetic says
 *   fa == fb makes two equal infinities agree: a depth that "does not exist" on both sides gives 0.  An infinity against a finite
 *   value gives t = +inf, Dg = +inf and w = expf_(-inf) = 0 (the first line of expf_): such a pair is never mixed.  At the centre
 *   offset Df = 0 and D = 0, so w = 1 and the denominator stays >= 1.  Features are assumed free of NaN.
 *   Everything else is vp_denoise's: the mean colours, y, v and the pair term, the two sum orders, the v_p == 0 exception,
 *   dst.w = src.w * s_p, the role of the guide pair, the safe range of v (Df and Dg have no NaN of their own: t_j >= 0 or +inf);
 *   no scene needed, asynchronous on the context's stream, never synchronises.
 *   vp_set_denoise_form applies and vp_last_denoise_form reports it.  With n_features == 0 (features may then be NULL) the output is
 *   vp_denoise's byte for byte.  Feature planes may be src, guide or each other.
 *   Refused with VP_E_ARG before the device is touched, dst untouched: everything vp_denoise refuses; n_features outside
 *   0..VP_DENOISE_MAX_FEATURES; features == NULL with n_features > 0; a NULL plane; a plane equal to dst; a channel outside 0..3; a
 *   sigma that is not finite or not > 0; a sigma whose g_j is not finite or not > 0 (this keeps 0 * inf out of the kernel). */
typedef struct { const vp_float4* plane; int channel; float sigma; } vp_denoise_feature;   /* channel 0..3 = x, y, z, w; 16 bytes */
#define VP_DENOISE_MAX_FEATURES 4
int vp_denoise_guided(vp_float4* dst, const vp_float4* src, const vp_pixel_stats* d_stats,
                      const vp_float4* guide, const vp_pixel_stats* d_guide_stats,
                      const vp_denoise_feature* features, int n_features,
                      int width, int height, const vp_denoise_params* dp);

/* Half-buffer renders and the cross-filtered output stage: the dual buffers of Rousselle, Knaus and Zwicker
 * 2012.  One render call splits its frames between two (accumulator, records) pairs, so that each half can supply the filter
 * weights for the OTHER one -- weights that are independent of the noise they filter.
 *
 * vp_render_frames_halves_stats.  THE DEFINITION: let S be the context's sub-pixel factor and m = log2 S.  Frame f belongs to half
 *   h(f) = (f >> 2m) & 1
 * -- S = 1: even frames to h0, odd frames to h1.  S > 1: blocks of S^2 consecutive frames alternate, NOT plain parity:
 * vp_subpixel_offset bit-reverses (f + hash) mod S^2, so the frames of one parity see half of the pixel's footprint only, while any
 * aligned block of S^2 frames covers the whole S x S lattice whatever the per-pixel hash.  For h = 0, 1 the accumulator d_h and the
 * records d_h_stats end bit-identical to what vp_render_frames_stats(d_h, d_h_stats, f, 1, p), called once for each f of
 * [first_frame, first_frame + n_frames) with h(f) == h in ascending order, leaves in the same context state.  Hence:
 *   - a frame adds nothing to the other half, no +0.0f either: a -0.0f already in the other accumulator stays -0.0f;
 *   - record h gains in n exactly the number of its own frames; `flags` is neither read nor written;
 *   - a per-pixel constant of a launch is one sequential addition per frame of that half, never a product;
 *   - only owned pixels are touched (vp_set_shard);
 *   - there is no hidden state: a second call continues a first one, a job that the staging cap splits into launches of any size
 *     gives the bits of one launch, and the half is a function of the ABSOLUTE frame number, never of the index within a launch.
 *   Built for: everything vp_render_frames_stats accepts -- every estimator, stream, tracking and environment mode, both arithmetic
 *   modes, every volume format and sub-pixel factor, shards: the render launches are that call's own kernel instances, and only the
 *   reduce is new.  Like the calls with planes it stops look-ahead batches, waits for pipelined launches and runs staged on the
 *   context's stream, for one frame too; it stages ONE plane, so vp_reserve_frames serves it unchanged.  It leaves nothing behind.
 *   Refused with VP_E_ARG before the device is touched, all four buffers untouched: any NULL pointer, d_h0 == d_h1, equal record
 *   pointers, n_frames <= 0, first_frame < 0.  Other errors as vp_render_frames_stats gives them.
 *   Not built: a form without records.  Adaptive rounds on halves: vp_render_adaptive_halves, below (section 2.20).  Halves of calls
 *   with planes (layers, groups, group layers): vp_render_frames_planes_halves_stats, below (section 2.19).
 *
 * vp_merge_halves: a and b are MEAN images of the two halves -- what vp_denoise, vp_denoise_guided or vp_scale_by_count(..., 1.0f)
 * write -- and of the records only n is read.  Binary32, one rounding per operation, no contraction, in the order written:
 *   na = (float)a_stats[i].n;   nb = (float)b_stats[i].n;   nt = na + nb
 *   nt == 0:   dst[i] = (0, 0, 0, 0),  resid[i] = 0
 *   else, each channel c of x, y, z, w:   dst[i].c = (a[i].c * na + b[i].c * nb) / nt          the divide correctly rounded
 *   lum(v)   = (0.2126f * v.x + 0.7152f * v.y) + 0.0722f * v.z
 *   d = lum(a[i]) - lum(b[i]);   e = 0.5f * fabsf(d);   ym = lum(dst[i]);   den = ym > floor_y ? ym : floor_y
 *   resid[i] = (a_stats[i].n == 0 || b_stats[i].n == 0) ? 0.0f : e / den
 * resid estimates the relative standard error of the merged image from the disagreement of two independent estimates; for filtered
 * halves it therefore includes the filter's residual noise, which the records can no longer tell.  A diagnostic image like
 * vp_stats_rel_error's; a pixel that vp_denoise leaves unfiltered because it is a constant gives exactly 0.  d_resid may be NULL; dst
 * may be a or b; no scene is needed; asynchronous on the context's stream, never synchronises.  Refused with VP_E_ARG before the device
 * is touched: NULL dst, a, b or either records pointer; size < 0; with d_resid given, a floor_y that is not finite or not > 0.
 * The cross-filter is these calls in sequence (no entry point of its own: the filter takes a fraction of a millisecond):
 *   vp_render_frames_halves_stats(h0, h1, s0, s1, ...)
 *   vp_denoise_guided(A, h0, s0, h1, s1, ...)   vp_denoise_guided(B, h1, s1, h0, s0, ...)   vp_merge_halves(dst, resid, A, s0, B, s1, ...)
 *
 * vp_accumulate_stats: vp_accumulate for records.  Per record dst.sum_y = dst.sum_y + src.sum_y and dst.sum_y2 = dst.sum_y2 +
 * src.sum_y2 (binary64), dst.n += src.n, dst.flags |= src.flags.  NULL pointers: VP_E_ARG.  With vp_accumulate it turns two halves
 * into the (accumulator, records) pair of all their frames, and it merges the records of sharded contexts on one device (disjoint
 * owned pixels: every addition is against zero and exact).  The union of two halves is NOT bit-equal to vp_render_frames_stats over
 * the same frames -- the order of the additions differs; the exact-parity product stays the uniform call. */
int vp_render_frames_halves_stats(vp_float4* d_h0, vp_float4* d_h1, vp_pixel_stats* d_h0_stats, vp_pixel_stats* d_h1_stats,
                                  int first_frame, int n_frames, const Param* p);
int vp_merge_halves(vp_float4* dst, float* d_resid, const vp_float4* a, const vp_pixel_stats* a_stats,
                    const vp_float4* b, const vp_pixel_stats* b_stats, int size, float floor_y);
int vp_accumulate_stats(vp_pixel_stats* dst, const vp_pixel_stats* src, size_t n);

/* The variance stage of the cross-filter: Rousselle, Knaus and Zwicker 2012 estimate the pixel variance from
 * BOTH buffers and smooth it with a small NL-means pass before the colour pass.  Three calls; opt-in, the calls above keep their bits.
 * Everything is binary32, one rounding per operation, no contraction, operations in the order written, unless marked binary64; min,
 * max and clamp() as in vp_denoise.  All three need no scene, run asynchronously on the context's stream behind what is queued there,
 * never synchronise, and check their arguments before the device is touched.
 *
 * vp_halves_variance: the pooled PER-SAMPLE luminance variance of two halves and the noise of that estimate; only the records are read.
 *   Per record T: T.n < 2: "not measured", u(T) = 0.  Else u(T) = (float)(max(lhs, 0.0) / (nd * (nd - 1.0))) with nd and lhs as in
 *   vp_denoise, binary64 rounded once (the unbiased sample variance: vp_denoise's v is this over n).  `flags` is never read.
 *   Per pixel, ua = u(a_stats[i]), ub = u(b_stats[i]):
 *     both measured:        u = 0.5f * (ua + ub);   d = ua - ub;   q = 0.25f * (d * d)
 *     exactly one measured: u = that half's value;  q = u * u      (nothing is known about its error)
 *     neither measured:     u = 0;  q = 0
 *   q estimates the variance of u: two independent estimates differ by twice the variance of their mean.  d_q may be NULL.
 *   VP_E_ARG: NULL d_u or records, size < 0.
 *
 * vp_filter_variance: vp_denoise's filter on one scalar plane.  The definition is vp_denoise's word for word with y := u, v := q and
 * the one "colour" c := u: the pair term e from (u, q), row sums, their sum, the scaling by 1 / (2F+1)^2, the clamp at 0, w = expf_(-D),
 * offsets in raster order, offsets that leave the image skipped, dst[p] = (sum of w * u_(p+o)) / (sum of w), one correctly rounded divide.
 *   Exceptions: there is no v_p == 0 exception; instead u[p] == 0.0f gives dst[p] = 0.0f -- a pixel that is a constant in both halves
 *   stays one, because vp_denoise's own early-outs hang on v_p == 0.  (Such a pixel still serves its neighbours as a value of 0.)
 *   The centre weight is exactly 1, so the denominator is >= 1; radius == 0 returns u bit for bit where u != 0.
 *   Inputs are assumed finite and small enough that d * d and q_a + q_b stay finite: u is a squared luminance and q its square, a
 *   FOURTH power of a luminance -- luminances up to about 3e9 are safe.
 *   Limits VP_DENOISE_MAX_RADIUS and VP_DENOISE_MAX_PATCH.  VP_E_ARG: NULL pointers; dst == u or dst == q; width or height < 1; radius
 *   or patch outside their limits; a k that is not finite or not > 0.  vp_set_denoise_form applies (0: a workgroup per 32 x 8 tile, u and
 *   q staged in LDS once; 1: a thread per pixel from global memory; the same bits) and vp_last_denoise_form reports it.
 *
 * vp_denoise_var: vp_denoise_guided with the variance supplied by the caller.  One change to the definition: wherever it reads v_a of
 * the guide -- the pair term and the v_p == 0 exception --
 *     v_a = d_sample_var[a'] * s_a'          s the GUIDE pair's 1.0f / (float)n, 0 where n == 0; one binary32 multiply
 *   -- a per-sample variance becomes the variance of that guide's mean.  Everything else, the features among it, is unchanged, and
 *   vp_denoise's safe range holds for this v: d_sample_var[a'] * s_a' at most 1.7e38 / max(1, k2).  With
 *   d_sample_var == NULL the output is vp_denoise_guided's byte for byte.  Refused: everything vp_denoise_guided refuses, and a plane
 *   that is dst.
 * The cross-filter with the stage: vp_render_frames_halves_stats(h0, h1, s0, s1, ...);  vp_halves_variance(u, q, s0, s1, n);
 *   vp_filter_variance(uf, u, q, ...);  vp_denoise_var(A, h0, s0, h1, s1, uf, ...);  vp_denoise_var(B, h1, s1, h0, s0, uf, ...);
 *   vp_merge_halves(dst, resid, A, s0, B, s1, ...).  Both colour passes read the same filtered plane. */
int vp_halves_variance(float* d_u, float* d_q, const vp_pixel_stats* a_stats, const vp_pixel_stats* b_stats, int size);
int vp_filter_variance(float* dst, const float* u, const float* q, int width, int height, const vp_denoise_params* vp);
int vp_denoise_var(vp_float4* dst, const vp_float4* src, const vp_pixel_stats* d_stats,
                   const vp_float4* guide, const vp_pixel_stats* d_guide_stats, const float* d_sample_var,
                   const vp_denoise_feature* features, int n_features,
                   int width, int height, const vp_denoise_params* dp);

/* Per-pixel filter selection from cross-buffer error estimates: Rousselle, Manzi and Zwicker 2013 filter with
 * several candidate windows, estimate each candidate's error per pixel, smooth the error maps, take the best candidate per pixel and
 * smooth the selection.  The half-buffers supply the estimate: a half filtered with colours of its own is held against the UNFILTERED
 * mean of the other half, whose noise the records measure.  Two calls; opt-in, the calls above keep their bits.  Binary32, one rounding
 * per operation, no contraction, operations in the order written, unless marked binary64.  Both need no scene, run asynchronously on
 * the context's stream behind what is queued there, never synchronise, and check their arguments before the device is touched.
 *
 * vp_cross_error: one candidate's per-pixel error estimate.  fa and fb are MEAN images of the two halves after some filter (what
 * vp_denoise* or vp_scale_by_count(..., 1.0f) write), (h0, s0) and (h1, s1) the halves' accumulators and records.  Per pixel i:
 *     c0 = h0[i].xyz * s_0,  s = n == 0 ? 0 : 1.0f / (float)n        vp_denoise's mean colours
 *     y0 = lum(c0),  lum(x, y, z) = (0.2126f x + 0.7152f y) + 0.0722f z
 *     v0 = vp_denoise's variance of the mean luminance from s0[i]: binary64, rounded once, 0 where n < 2
 *     y1, v1 likewise from (h1, s1)
 *     da = lum(fa[i]) - y1;   ea = da * da - v1;      db = lum(fb[i]) - y0;   eb = db * db - v0
 *     err = (s0[i].n >= 2 && s1[i].n >= 2) ? 0.5f * (ea + eb) : 0.0f
 *   err is NOT clamped: E[(f - y)^2] = (f - mu)^2 + Var(y) for f independent of y, so (f - y)^2 - v is an unbiased estimate of the
 *   squared luminance error of the filtered half, and it may be negative.  Clamping before smoothing would bias it.  `flags` is never
 *   read.  Inputs are assumed finite with v0, v1 finite as binary32: variances of the mean up to 3.4e38, per-sample luminances up to
 *   about 1e19.  Then err is no NaN; it is +inf where da * da or db * db overflows (|lum(f) - y| above 1.8e19) and -inf where ea + eb
 *   does.  Nothing clamps here: a variance that rounds to +inf gives -inf, and NaN where the squared difference overflows too.
 *   VP_E_ARG: any NULL pointer, d_err equal to an input, size < 0.
 *   What the estimate is and is not: it sees LUMINANCE only, like every filter here.  It is unbiased only as far as fa is independent
 *   of h1's noise: the WEIGHTS of a cross-filtered fa come from h1, and the variance stage pools both halves -- that dependence is
 *   second order and it is not removed.  A self-guided candidate whose colours come from both halves is not a valid input.
 *
 * vp_select: smooth the errors, pick per pixel, blend the picks.  images and errors are HOST arrays of n device pointers (the kernel
 * takes them by value in its argument block).  With Rs = smooth_radius, Rb = blend_radius:
 *   Smoothed error: for ty = -Rs..Rs, top to bottom, row_ty = the sum over tx = -Rs..Rs, left to right and starting from 0.0f, of
 *     errors[c] at p + (tx, ty); positions outside the image are skipped, and a row outside the image contributes nothing.  S = the sum
 *     of the rows, top to bottom, starting from 0.0f.  E_c(p) = S / (float)count, count the number of in-image positions, one correctly
 *     rounded divide.  The sums run row first so that a horizontal pass followed by a vertical pass gives the same bits.
 *   Pick: k = 0; for c = 1..n-1: if (E_c(p) < E_k(p)) k = c.  Ties go to the lowest index: the order of the candidates is a
 *     preference.  Inputs are assumed free of NaN.
 *   Blend: W_c(p) = the number of in-image positions q in the (2 Rb + 1)^2 window of p with k(q) == c (an integer: no order matters),
 *     T = the number of in-image positions.  W_k(p) == T: dst[p] = images[k(p)][p] bit for bit in all four channels.  Otherwise, per
 *     channel of x, y, z:  num = 0.0f;  num = num + (float)W_c * images[c][p].ch for c = 0..n-1 in order;  dst[p].ch = num / (float)T.
 *     dst[p].w = images[k(p)][p].w always: the heat or coverage channel is never blended, as it is never filtered.
 *   Consequences: n = 1 is a copy.  Equal error planes give images[0].  A region where one candidate wins throughout carries that
 *   candidate's bits.  A pixel that every candidate left unfiltered (a constant) keeps its value wherever all candidates agree on it
 *   bit for bit and (n W c) / T rounds back to c -- always where one candidate holds the whole window.
 *   d_index (may be NULL) receives k(p).  dst may be one of images: the call reads images at p only.
 *   VP_E_ARG: NULL dst, images, errors or sp; n outside 1..VP_SELECT_MAX_CANDIDATES; a NULL entry; an error plane or d_index equal to
 *   dst; width or height < 1; a radius outside 0..VP_SELECT_MAX_RADIUS.  vp_set_denoise_form applies (0: a workgroup per 32 x 8 tile,
 *   the error planes staged in LDS once, horizontal then vertical sums; 1: a thread per pixel from global memory; the same bits) and
 *   vp_last_denoise_form reports it.
 * The pipeline: the variance stage once; per candidate (R, F, k): vp_denoise_var(A, h0, s0, h1, s1, uf, ...); vp_denoise_var(B, h1,
 *   s1, h0, s0, uf, ...); vp_cross_error(err_c, A, B, h0, s0, h1, s1, n); vp_merge_halves(img_c, NULL, A, s0, B, s1, ...); then one
 *   vp_select(dst, index, img, err, n, ...). */
typedef struct { int smooth_radius, blend_radius; } vp_select_params;   /* 8 bytes */
#define VP_SELECT_MAX_CANDIDATES 4
#define VP_SELECT_MAX_RADIUS 3
int vp_cross_error(float* d_err, const vp_float4* fa, const vp_float4* fb,
                   const vp_float4* h0, const vp_pixel_stats* s0,
                   const vp_float4* h1, const vp_pixel_stats* s1, int size);
int vp_select(vp_float4* dst, uint8_t* d_index,
              const vp_float4* const* images, const float* const* errors, int n,
              int width, int height, const vp_select_params* sp);

/* Compositing layers: a foreground F and a per-channel transmittance T with  pixel = F + T o B  for any
 * background B -- another sky, a plate, a second render.  vp_render_frames bakes the context's own sky into every sample and keeps
 * the reference's heat value in w; these two calls are what a compositor needs instead.
 *
 * vp_render_frames_layers.  Take the sample (x, y, frame) that vp_render_frames computes: same path, same draws, same streams.  Let
 * thr be its throughput where it leaves the medium for the environment and heat its fourth channel.  The path is UNSCATTERED if it
 * gets there without a scatter event (a camera ray that misses the box, or one tracked through the box with null collisions only).
 *   unscattered:  fg sample (0, 0, 0, heat)                 trans sample (max(thr.x, 0), max(thr.y, 0), max(thr.z, 0), 1)
 *   otherwise:    fg sample = the vp_render_frames sample    trans sample (0, 0, 0, 0)
 * No brightness and no background enter a trans sample; the fg sample of a scattered path includes the sky light it sees after
 * scattering.  Both caller-owned accumulators (width * height float4 each, not the same buffer) receive their samples in frame
 * order, like vp_render_frames' accumulator.  So fg.w is bit-equal to vp_render_frames' w; trans.w / n is the fraction of unscattered
 * samples; 1 - trans.xyz / n is the per-channel alpha.  Equivalently: the trans RGB of an unscattered sample is the vp_render_frames
 * sample of the same scene with every environment texel (1, 1, 1), a sun disc of (1, 1, 1) and brightness 1 -- with the passive
 * environment none of those influences a draw.
 *   Obeys vp_set_shard, vp_set_estimator, vp_set_rng and vp_set_subpixel (every value each), every volume format and cell order.
 *   It runs kernel instances of its own, built in the exact arithmetic only; vp_render_frames' kernels carry no code for it.  The call stops look-ahead batches, waits for pipelined launches and runs staged on the
 *   context's stream, for one frame too; it leaves nothing behind: a vp_render_frames call after it renders the bits it rendered
 *   before.
 *   Refused before anything is launched and before the device is touched, with VP_E_ARG: NULL pointers, d_fg == d_trans,
 *   n_frames <= 0, first_frame < 0; with VP_E_STATE: VP_ENV_MIS (scattered paths never see the sky there: another definition),
 *   scalar and multi-channel tracking, enabled work counters, VP_ARITH_FAST.  Both buffers are then untouched.  Other errors as vp_render_frames.
 *   This call takes no statistics (vp_render_frames_layers_stats below does) and runs no adaptive rounds (vp_render_adaptive_layers
 *   below does); reducing layers across processes is not built.
 *
 * vp_composite, the output stage: for i < size, with B = plate[i].xyz where plate is non-NULL, else plate_rgb[0..2],
 *   dst[i].xyz = fg[i].xyz * scale + (trans[i].xyz * scale) * B        dst[i].w = 1 - trans[i].w * scale   (coverage)
 * in binary32: one multiply and one add per term in this order, no contraction.  scale is 1 / frames.  dst may be fg or trans.
 * Needs no scene; runs asynchronously on the context's stream.  VP_E_ARG: NULL dst, fg or trans, both plate pointers NULL, size < 0. */
int vp_render_frames_layers(vp_float4* d_fg, vp_float4* d_trans, int first_frame, int n_frames, const Param* p);
int vp_composite(vp_float4* dst, const vp_float4* fg, const vp_float4* trans, const vp_float4* plate, const float plate_rgb[3], int size, float scale);

/* Light groups: the sun's light and the sky's light of one render in separate accumulators, to be weighted
 * against each other afterwards.  The integrator is linear in its lights: the sun's power enters a sample only as a factor of each
 * shadow-ray term, the environment only once, where the path ends; with the passive environment neither influences a draw.
 *
 * vp_render_frames_groups.  Take the sample (x, y, frame) that vp_render_frames computes: same path, same draws, same streams.  Let R
 * be the radiance the path has summed from its sun shadow rays when it ends, E the term its end adds -- thr o background(dir, depth)
 * if the path leaves for the environment, otherwise nothing --, b the brightness and heat the fourth channel.  vp_render_frames
 * writes (max(b (R + E), 0), heat).  This call writes
 *   E is the sun disc's value (background at depth 0 inside the disc):
 *                 sun sample (max(b (R + E), 0), heat)        sky sample (0, 0, 0, heat)
 *   otherwise:    sun sample (max(b R, 0), heat)              sky sample (max(b E, 0), heat); a path with no E: (0, 0, 0, heat)
 * with the operations of the beauty sample in its order (the sky sample's sum starts from +0 as the path's does).  Both caller-owned
 * accumulators (width * height float4 each, not the same buffer) receive their samples per pixel in frame order, like
 * vp_render_frames' accumulator.  Equivalently, wherever the path's throughput is finite: the sun accumulator is bit for bit what
 * vp_render_frames renders on the same scene with every environment texel (0, 0, 0), the sky accumulator what it renders after
 * set_sun(dir, (0, 0, 0)).  Where a throughput is not finite (0 * inf in such a render) the in-kernel form above is the definition.
 *   Obeys vp_set_shard, vp_set_estimator, vp_set_rng and vp_set_subpixel (every value each), every volume format, cell order and LDS
 *   form of the brick table.  It runs kernel instances of its own, built in the exact arithmetic only; vp_render_frames' kernels
 *   carry no code for it.  The call stops look-ahead batches, waits for pipelined launches and runs staged on the context's stream,
 *   for one frame too, in two staging planes: a launch holds half the frames a vp_render_frames launch holds
 *   (vp_reserve_frames_groups sizes the staging for it).  It leaves nothing behind: a vp_render_frames call after it renders the
 *   bits it rendered before.
 *   Refused before anything is launched and before the device is touched, with VP_E_ARG: NULL pointers, d_sun == d_sky,
 *   n_frames <= 0, first_frame < 0; with VP_E_STATE: VP_ENV_MIS (the environment is sampled as a light there: another estimator),
 *   scalar and multi-channel tracking, enabled work counters, VP_ARITH_FAST.  Both buffers are then untouched.  Other errors as
 *   vp_render_frames.
 *   Not built: reducing groups across processes.  With layers in one call: vp_render_frames_group_layers, below.  Not part of THIS call, which writes no
 *   records: statistics, adaptive rounds or vp_denoise on groups.  vp_render_frames_groups_stats, below, is the same render with one
 *   record buffer per group, which is what vp_denoise needs; vp_render_adaptive_groups, below it, runs the adaptive rounds.
 *
 * vp_relight, the output stage: for i < size and each channel c of x, y, z, in binary32, one rounding per operation, no contraction,
 *   a = (sun[i].c * scale) * sun_gain[c]     k = (sky[i].c * scale) * sky_gain[c]     dst[i].c = a + k     dst[i].w = sun[i].w * scale
 * scale is 1 / frames.  dst may be sun or sky.  Needs no scene; runs asynchronously on the context's stream.  VP_E_ARG: NULL dst,
 * sun, sky or either gain, size < 0.
 *
 * vp_reserve_frames_groups: vp_reserve_frames for a coming vp_render_frames_groups job (two planes per frame, one-frame calls too).
 * vp_groups_frames_per_launch: the frames one staged launch of this context holds for this image now, with planes = 1
 * (vp_render_frames) or 2 (vp_render_frames_groups); negative: an error code. */
int vp_render_frames_groups(vp_float4* d_sun, vp_float4* d_sky, int first_frame, int n_frames, const Param* p);
int vp_relight(vp_float4* dst, const vp_float4* sun, const vp_float4* sky, const float sun_gain[3], const float sky_gain[3], int size, float scale);
int vp_reserve_frames_groups(const Param* p, int n_frames);
int vp_groups_frames_per_launch(const Param* p, int planes);

/* Statistics on planes: vp_render_frames_groups and vp_render_frames_layers with one buffer of per-pixel
 * records per plane, so that each plane can be filtered by vp_denoise with its own noise estimate as guide.
 *
 * vp_render_frames_groups_stats / vp_render_frames_layers_stats.  THE DEFINITION:
 *   The two accumulators end bit-identical to what vp_render_frames_groups / vp_render_frames_layers write with the same arguments
 *   and state.  Each record buffer holds width * height vp_pixel_stats, caller-owned and caller-zeroed (vp_memset), indexed like the
 *   accumulators.  For every sample v that the call adds to a PLANE's accumulator at pixel i, record i of THAT plane receives exactly
 *   what vp_render_frames_stats defines:
 *     y = (0.2126f * v.x + 0.7152f * v.y) + 0.0722f * v.z      in binary32, no contraction
 *     sum_y  += (double)y        sum_y2 += (double)y * (double)y        n += 1
 *   per pixel in frame order.  v is the sample as the underlying call's definition names it, not a staged word: for an unscattered
 *   path of a layers call the fg sample is (0, 0, 0, heat), so its y is +0, and the trans sample is (max(thr, 0), 1), whose y comes
 *   from its RGB; a scattered path gives the trans record y = 0.  w never enters a luminance.  Every owned pixel's two records gain
 *   n_frames in n -- the per-pixel-constant classes (box-missing pixels, a light class written as constants) included, and theirs are
 *   n_frames sequential additions, never a product.  `flags` is neither read nor written.  Only the records of the pixels this
 *   context owns (vp_set_shard) are touched.  There is no hidden state: a second call continues a first one, records and accumulators
 *   carry over, and a job that the staging cap splits into several launches gives the bits of one launch.
 *   Equivalently, wherever the path's throughput is finite (as for vp_render_frames_groups): the sun records are bit for bit what
 *   vp_render_frames_stats leaves on the same scene with every environment texel (0, 0, 0), the sky records what it leaves after
 *   set_sun(dir, (0, 0, 0)).
 *   Everything else is as the underlying call: it obeys vp_set_shard, vp_set_estimator, vp_set_rng and vp_set_subpixel, every volume
 *   format and LDS form; it runs staged on the context's stream, for one frame too; it stops look-ahead batches and waits for
 *   pipelined launches; it leaves no per-context state behind.  The render launches are the underlying call's own; only the reduce
 *   that adds the staged samples differs.  A groups call needs the two-plane staging: vp_reserve_frames_groups serves it unchanged.
 *   Refused before the device is touched, all four buffers untouched, with VP_E_ARG: any NULL pointer, d_sun == d_sky
 *   (d_fg == d_trans), the two record pointers equal, n_frames <= 0, first_frame < 0; with VP_E_STATE exactly where the underlying
 *   call gives it (VP_ENV_MIS, scalar and multi-channel tracking, enabled work counters, VP_ARITH_FAST).
 *   These calls run no adaptive rounds on planes: vp_render_adaptive_groups / vp_render_adaptive_layers of the next section do, and
 *   vp_render_adaptive_group_layers (section 2.11) runs the adaptive rounds on three planes.  Still not built: reducing planes or their
 *   records across processes, and these calls under VP_ARITH_FAST.
 * The pipeline these calls exist for: the _stats call, then per plane vp_denoise(dst, plane, plane's records, NULL, NULL, ...) -- a
 * MEAN image each --, then vp_relight or vp_composite of the two means with scale 1.  vp_denoise never filters w, so a layers
 * composite keeps its exact coverage. */
int vp_render_frames_groups_stats(vp_float4* d_sun, vp_float4* d_sky, vp_pixel_stats* d_sun_stats, vp_pixel_stats* d_sky_stats,
                                  int first_frame, int n_frames, const Param* p);
int vp_render_frames_layers_stats(vp_float4* d_fg, vp_float4* d_trans, vp_pixel_stats* d_fg_stats, vp_pixel_stats* d_trans_stats,
                                  int first_frame, int n_frames, const Param* p);

/* Adaptive sampling on planes: vp_render_adaptive's rounds on the two planes of a light-groups or a layers
 * render.  [0] of the parameter arrays is the first plane's (sun / fg), [1] the second's (sky / trans).
 *
 * vp_render_adaptive_groups / vp_render_adaptive_layers.  THE DEFINITION:
 *   A pixel is ACTIVE while the FROZEN bit is clear in BOTH of its records.  The frozen set is exactly what the two caller-owned
 *   record buffers say: there is no hidden state, so a second call continues a first one.  Rounds are vp_render_adaptive's: with
 *   B = round_frames, round k covers frames [first_frame + k B, first_frame + min((k + 1) B, max_frames)).  Every owned pixel that is
 *   active at the start of a round receives all frames of the round in both planes: the samples, accumulators and records are exactly
 *   those that vp_render_frames_groups_stats / vp_render_frames_layers_stats define for that pixel and those frames, added in frame
 *   order (the per-pixel-constant classes: sequential additions).  A pixel that is not active receives nothing, in either accumulator
 *   or record.  After the round each pixel that was active in it is frozen iff, for both k = 0 and k = 1, record k has
 *   n >= min_frames and vp_render_adaptive's criterion holds on it with (rel_tol[k], floor_y[k]) -- the same binary64 operations in the
 *   same order, false on NaN, each record with its own n.  Freezing sets the FROZEN bit in both records and changes no other flag
 *   bit; it is permanent.  The call ends when no owned pixel is active or the frames are used up.  `result` is as in
 *   vp_render_adaptive; `samples` counts one per pixel and frame, not per plane.  The samples a pixel receives depend on nothing but
 *   this definition: a round that the staging cap splits into several launches gives the bits of one launch.
 *   Why AND, and why per plane: the product of these calls is weighted afterwards -- vp_relight's gains, any plate in vp_composite.
 *   The weights are unknown at render time and the records hold no cross-covariance, so a criterion on the sum would be wrong for every
 *   other weighting: each plane must be converged by its own measure.  The planes live on different scales (radiance times brightness
 *   for sun, sky and fg; [0, 1] for trans), hence one tolerance and one floor per plane.  A large floor_y[k] with rel_tol[k] > 0
 *   (1e30f, say) makes plane k's criterion hold from two samples on, i.e. takes plane k out of the decision: the frozen set is then the
 *   other plane's own.
 *   What it is not, as for vp_render_adaptive: the stopping rule looks at the estimate it stops, which gives a small bias.  The image
 *   of a plane is sum / n per pixel: vp_scale_by_count with THAT plane's records, then vp_relight / vp_composite with scale 1.  The
 *   exact-parity products stay the uniform calls.
 *   Refused before the device is touched, all four buffers untouched, with VP_E_ARG: any NULL pointer (result excepted), equal
 *   accumulators or equal record buffers, max_frames <= 0 or first_frame < 0, min_frames < 2, round_frames < 1, any tolerance or floor
 *   negative or NaN; with VP_E_STATE exactly where the underlying plane call gives it (VP_ENV_MIS, scalar and multi-channel tracking,
 *   enabled work counters, VP_ARITH_FAST).  VP_E_NOOPACITY as vp_render_frames gives for frame first_frame + max_frames - 1.
 *   Everything else is as the underlying plane call: it obeys vp_set_shard, vp_set_estimator, vp_set_rng, vp_set_stream,
 *   vp_set_subpixel and every volume format; it stops look-ahead batches, waits for pipelined launches and runs on the context's
 *   stream, reading three counts back per round (it synchronises); it leaves nothing behind -- a vp_render_frames, a plain plane call or
 *   a vp_render_adaptive after it renders the bits it rendered before -- and never modifies the cached pixel lists.
 *   Adaptive rounds on three planes: vp_render_adaptive_group_layers, below (section 2.11).  Still not built: reducing planes or records
 *   across processes, these calls under VP_ARITH_FAST. */
typedef struct { float rel_tol[2], floor_y[2]; int min_frames, round_frames; } vp_adaptive_planes;   /* [0]: sun / fg, [1]: sky / trans */
int vp_render_adaptive_groups(vp_float4* d_sun, vp_float4* d_sky, vp_pixel_stats* d_sun_stats, vp_pixel_stats* d_sky_stats,
                              int first_frame, int max_frames, const Param* p, const vp_adaptive_planes* a, vp_adaptive_result* result);
int vp_render_adaptive_layers(vp_float4* d_fg, vp_float4* d_trans, vp_pixel_stats* d_fg_stats, vp_pixel_stats* d_trans_stats,
                              int first_frame, int max_frames, const Param* p, const vp_adaptive_planes* a, vp_adaptive_result* result);

/* Group layers: light groups combined with layers in one render -- the sun's light, the sky's light and the
 * per-channel transmittance of the same paths in three accumulators, for a cloud element that is relit AND put over a new background.
 * The groups planes bake the background into unscattered paths, the layers foreground has sun and sky summed: either call discards
 * what the other keeps, so the pair costs two renders of the same paths.  This call costs one.
 *
 * vp_render_frames_group_layers.  THE DEFINITION:
 *   Take the sample (x, y, frame) that vp_render_frames computes: same path, same draws, same streams.  Let R, E, b and heat be as for
 *   vp_render_frames_groups, thr and UNSCATTERED as for vp_render_frames_layers.  This call writes
 *     unscattered:  sun sample (0, 0, 0, heat)         sky sample (0, 0, 0, heat)          trans sample (max(thr.x, 0), max(thr.y, 0), max(thr.z, 0), 1)
 *     otherwise:    sun sample (max(b R, 0), heat)     sky sample (max(b E, 0), heat);     trans sample (0, 0, 0, 0)
 *                                                      a path with no E: (0, 0, 0, heat)
 *   with the operations of the beauty sample in its order; the sky sample's sum starts from +0.  A scattered path never sees the sun's
 *   disc (background at depth 0), so the disc case of vp_render_frames_groups arises in the unscattered row only -- and there the path
 *   is a transmittance sample like any other unscattered path: no background enters it.  The three caller-owned accumulators
 *   (width * height float4 each, all distinct) receive their samples per pixel in frame order; a per-pixel constant of a launch is
 *   n_frames sequential additions, never a product.
 *   Equivalently, wherever the path's throughput is finite and the path reaches the environment: trans is bit for bit the trans
 *   accumulator of vp_render_frames_layers; sun is the fg accumulator of vp_render_frames_layers on the same scene with every
 *   environment texel (0, 0, 0); sky is its fg accumulator after set_sun(dir, (0, 0, 0)); on a sample whose path scattered, sun and
 *   sky are the two samples of vp_render_frames_groups; sun.w, sky.w and the layers call's fg.w are equal bits.
 *   Built for exactly what the two plane calls are built for: it obeys vp_set_shard, vp_set_estimator, vp_set_rng, vp_set_stream and
 *   vp_set_subpixel (every value each), every volume format, cell order and LDS form of the brick table.  It runs kernel instances of
 *   its own (the existing ones carry no code for it), stops look-ahead batches, waits for pipelined launches and runs staged on the
 *   context's stream, for one frame too, in the two staging planes of a groups call -- two planes carry the three products, since an
 *   unscattered sample is marked in the first and needs no word in the second: vp_reserve_frames_groups and
 *   vp_groups_frames_per_launch(p, 2) serve it unchanged.  It leaves nothing behind: a vp_render_frames, groups or layers call after it
 *   renders the bits it rendered before.
 *   Refused before the device is touched, all buffers untouched, with VP_E_ARG: any NULL pointer, any two accumulators equal,
 *   n_frames <= 0, first_frame < 0; with VP_E_STATE exactly where the two plane calls give it (VP_ENV_MIS, scalar and multi-channel
 *   tracking, enabled work counters, VP_ARITH_FAST).  Other errors as vp_render_frames.
 *
 * vp_render_frames_group_layers_stats: the same render with one record buffer per plane.  The three accumulators end bit-identical to
 *   the plain call's.  For every sample v that the call adds to a PLANE's accumulator at pixel i, record i of THAT plane receives
 *   exactly what the section "Statistics on planes" defines (y from v's RGB in binary32; sum_y, sum_y2, n), in frame order; w never
 *   enters a luminance; constants are sequential additions; `flags` is neither read nor written; only owned pixels are touched; there
 *   is no hidden state, a second call continues a first.  Refusals as the plain call's, plus NULL records and any two record pointers
 *   equal.  Only the reduce differs from the plain call.
 *
 * vp_relight_composite, the output stage: for i < size and each channel c of x, y, z, in binary32, one rounding per operation, no
 * contraction, with B as in vp_composite,
 *   f = (sun[i].c * scale) * sun_gain[c] + (sky[i].c * scale) * sky_gain[c]
 *   dst[i].c = f + (trans[i].c * scale) * B.c          dst[i].w = 1 - trans[i].w * scale
 * Its bits are those of vp_relight(tmp, sun, sky, gains, size, scale), scale(t, trans, size, scale) and
 * vp_composite(dst, tmp, t, plate, plate_rgb, size, 1.0f) in sequence.  dst may be any of the three inputs.  Needs no scene; runs
 * asynchronously on the context's stream.  VP_E_ARG as for the two calls it fuses: NULL dst, sun, sky, trans or either gain, both
 * plate pointers NULL, size < 0.
 *   These calls run no adaptive rounds on three planes: vp_render_adaptive_group_layers, below, does.  Still not built: reducing planes
 *   or records across processes, these calls under VP_ARITH_FAST. */
int vp_render_frames_group_layers(vp_float4* d_sun, vp_float4* d_sky, vp_float4* d_trans, int first_frame, int n_frames, const Param* p);
int vp_render_frames_group_layers_stats(vp_float4* d_sun, vp_float4* d_sky, vp_float4* d_trans,
                                        vp_pixel_stats* d_sun_stats, vp_pixel_stats* d_sky_stats, vp_pixel_stats* d_trans_stats,
                                        int first_frame, int n_frames, const Param* p);
int vp_relight_composite(vp_float4* dst, const vp_float4* sun, const vp_float4* sky, const vp_float4* trans,
                         const float sun_gain[3], const float sky_gain[3], const vp_float4* plate, const float plate_rgb[3], int size, float scale);

/* Adaptive sampling on group layers: vp_render_adaptive's rounds on the three planes of a group-layers
 * render.  [0] of the parameter arrays is sun's, [1] sky's, [2] trans's.
 *
 * vp_render_adaptive_group_layers.  THE DEFINITION is that of "Adaptive sampling on planes", with three planes where it says two:
 *   A pixel is ACTIVE while the FROZEN bit is clear in ALL THREE of its records.  The frozen set is exactly what the three caller-owned
 *   record buffers say: there is no hidden state, so a second call continues a first one.  Rounds are vp_render_adaptive's: with
 *   B = round_frames, round k covers frames [first_frame + k B, first_frame + min((k + 1) B, max_frames)).  Every owned pixel that is
 *   active at the start of a round receives all frames of the round in all three planes: the samples, accumulators and records are
 *   exactly those that vp_render_frames_group_layers_stats defines for that pixel and those frames, added in frame order (the
 *   per-pixel-constant classes: sequential additions).  A pixel that is not active receives nothing, in any accumulator or record.
 *   After the round each pixel that was active in it is frozen iff, for k = 0, 1 and 2, record k has n >= min_frames and
 *   vp_render_adaptive's criterion holds on it with (rel_tol[k], floor_y[k]) -- the same binary64 operations in the same order, false
 *   on NaN, each record with its own n.  Freezing sets the FROZEN bit in all three records and changes no other flag bit; it is
 *   permanent.  The call ends when no owned pixel is active or the frames are used up.  `result` is as in vp_render_adaptive;
 *   `samples` counts one per pixel and frame, not per plane.  A round that the staging cap splits into several launches gives the bits
 *   of one launch.
 *   Why AND, and why per plane: as for two planes -- vp_relight_composite's gains and plate are unknown at render time.  A large
 *   floor_y[k] with rel_tol[k] > 0 (1e30f, say) takes plane k out of the decision; two planes out leaves the third plane's own frozen
 *   set.
 *   What it is not, as for vp_render_adaptive: the stopping rule looks at the estimate it stops, which gives a small bias.  The image
 *   of a plane is sum / n per pixel: vp_scale_by_count with THAT plane's records, then vp_relight_composite with scale 1.  The
 *   exact-parity product stays the uniform call.
 *   Refused before the device is touched, all six buffers untouched and *result zeroed, with VP_E_ARG: any NULL pointer (result
 *   excepted), any two accumulators equal or any two record buffers equal, max_frames <= 0 or first_frame < 0, min_frames < 2,
 *   round_frames < 1, any tolerance or floor negative or NaN; with VP_E_STATE exactly where vp_render_frames_group_layers gives it
 *   (VP_ENV_MIS, scalar and multi-channel tracking, enabled work counters, VP_ARITH_FAST); an argument error comes before a state
 *   error.  VP_E_NOOPACITY as vp_render_frames gives for frame first_frame + max_frames - 1.
 *   Everything else is as vp_render_frames_group_layers: it obeys vp_set_shard, vp_set_estimator, vp_set_rng, vp_set_stream,
 *   vp_set_subpixel and every volume format; vp_reserve_frames_groups serves it; it stops look-ahead batches, waits for pipelined
 *   launches and runs on the context's stream, reading three counts back per round (it synchronises); it leaves nothing behind -- a
 *   vp_render_frames, a plain plane call or another adaptive call after it renders the bits it rendered before -- and never modifies
 *   the cached pixel lists.  The render launches are the plain call's instances on shorter lists; only the reduce and the compaction
 *   have three-record forms.
 *   Still not built: reducing planes or records across processes, these calls under VP_ARITH_FAST. */
typedef struct { float rel_tol[3], floor_y[3]; int min_frames, round_frames; } vp_adaptive_planes3;   /* [0] sun, [1] sky, [2] trans; 32 bytes */
int vp_render_adaptive_group_layers(vp_float4* d_sun, vp_float4* d_sky, vp_float4* d_trans,
                                    vp_pixel_stats* d_sun_stats, vp_pixel_stats* d_sky_stats, vp_pixel_stats* d_trans_stats,
                                    int first_frame, int max_frames, const Param* p, const vp_adaptive_planes3* a, vp_adaptive_result* result);

/* Half-buffer renders of calls with planes: vp_render_frames_halves_stats for layers, light groups and group
 * layers, so that the cross-filter, the variance stage and the selection (vp_halves_variance, vp_filter_variance, vp_denoise_var,
 * vp_cross_error, vp_merge_halves, vp_select -- all take arbitrary (accumulator, records) pairs) serve each plane a compositor takes.
 * One staged call fills two independent halves of every plane.  h0 and h1 hold the planes of one half in the mode's order -- layers:
 * fg, trans; groups: sun, sky; group layers: sun, sky, trans --; entries beyond the mode's planes are ignored, garbage included.
 *
 * vp_render_frames_planes_halves_stats.  THE DEFINITION: let N be the mode's number of planes, S the context's sub-pixel factor,
 * m = log2 S and h(f) = (f >> 2m) & 1, the half rule of vp_render_frames_halves_stats.  For h = 0, 1 the N accumulators and the N
 * record buffers of half h end bit-identical to what the mode's one-frame _stats call -- vp_render_frames_layers_stats,
 * vp_render_frames_groups_stats or vp_render_frames_group_layers_stats with n_frames = 1 on the planes of half h --, called once for
 * each f of [first_frame, first_frame + n_frames) with h(f) == h in ascending order, leaves in the same context state.  Hence:
 *   - within the half that receives a frame the plane call's rule holds: a plane that the sample does not feed is ADDED +0.0f -- a
 *     -0.0f there becomes +0.0f -- and its record gains n += 1 with y = +0;
 *   - the other half's planes receive nothing for that frame: no +0.0f is added, so a -0.0f survives; no count is added; and no byte
 *     is written where a launch holds no frame of that half;
 *   - every record of half h gains in n exactly the number of its own frames; `flags` is neither read nor written;
 *   - a per-pixel constant of a launch is one sequential addition per frame of the half, never a product;
 *   - only owned pixels are touched (vp_set_shard);
 *   - there is no hidden state: the half is a function of the ABSOLUTE frame number, a second call continues a first one, and a job
 *     that the staging cap splits into launches of any size gives the bits of one launch.
 *   Built for exactly what the underlying plane call is built for: every estimator, stream and sub-pixel factor, every volume format,
 *   cell order and LDS form, shards.  It stages as the underlying call does -- one plane for layers, the two planes of a groups call
 *   for the other two modes --, so vp_reserve_frames / vp_reserve_frames_groups and vp_groups_frames_per_launch serve it unchanged.
 *   The render launches are the underlying plane call's own instances, counted under that mode's census kind; only the reduce is new.
 *   It stops look-ahead batches, waits for pipelined launches, runs on the context's stream and leaves nothing behind.
 *   Refused with VP_E_ARG before the device is touched, every buffer untouched: an unknown mode; a NULL h0, h1, p or used entry; any
 *   two of the 2N accumulators equal; any two of the 2N record buffers equal; n_frames <= 0 or first_frame < 0.  VP_E_STATE exactly
 *   where the underlying plane call gives it (VP_ENV_MIS, scalar and multi-channel tracking, enabled work counters, VP_ARITH_FAST),
 *   the message naming this entry point; an argument error comes before a state error.  Other errors are the underlying call's.
 *   The output stage per plane is the cross-filter's sequence with that plane's two halves (and that plane's floor for the residual:
 *   trans is constant over most pixels and lies in [0, 1]); per-pixel selection composes in the same way from vp_cross_error and
 *   vp_select with a plane's halves -- the volpath_render driver offers the cross-filter and the variance stage on planes, not selection.
 *   Adaptive rounds on halves: vp_render_adaptive_planes_halves, below (section 2.20).
 *   Still not built: a form without records, reduction across processes, VP_ARITH_FAST. */
enum { VP_PLANES_LAYERS = 1, VP_PLANES_GROUPS = 2, VP_PLANES_GROUP_LAYERS = 3 };
/* the planes of one half in the mode's order: fg trans | sun sky | sun sky trans; entries beyond the mode's planes are ignored */
typedef struct { vp_float4* acc[3]; vp_pixel_stats* rec[3]; } vp_plane_bufs;   /* 48 bytes */
int vp_render_frames_planes_halves_stats(int mode, const vp_plane_bufs* h0, const vp_plane_bufs* h1,
                                         int first_frame, int n_frames, const Param* p);

/* Adaptive sampling on half-buffers: vp_render_adaptive's rounds into the two halves of a half-buffer render,
 * for the beauty image and for every plane call -- Rousselle, Knaus and Zwicker 2012 sample adaptively into their two buffers, and the
 * cross-filter (vp_denoise_var, vp_merge_halves, vp_cross_error, vp_select) then reads halves whose pixels hold different sample counts.
 *
 * vp_render_adaptive_halves, vp_render_adaptive_planes_halves.  THE DEFINITION: let N be the mode's number of planes -- N = 1 for
 * vp_render_adaptive_halves, whose one plane is (d_h0, d_h0_stats) in half 0 and (d_h1, d_h1_stats) in half 1 --, S the context's
 * sub-pixel factor, m = log2 S and h(f) = (f >> 2m) & 1, the half rule of vp_render_frames_halves_stats.
 *   A pixel is ACTIVE while the FROZEN bit is clear in ALL 2N of its records.  The frozen set is exactly what the caller's 2N record
 *   buffers say: there is no hidden state, so a second call continues a first one, and a pixel that the caller froze in ONE record
 *   only is not active.  Rounds are vp_render_adaptive's: with B = round_frames, round k covers frames
 *   [first_frame + k B, first_frame + min((k + 1) B, max_frames)).  Every owned pixel that is active at the start of a round receives
 *   all frames of the round: its accumulators and records change exactly as the halves call -- vp_render_frames_halves_stats for the
 *   beauty image, vp_render_frames_planes_halves_stats for planes -- defines for that pixel and those frames.  Frame f goes to half
 *   h(f) of the ABSOLUTE frame number and to no other: the other half receives no +0.0f and no count for that frame, and a per-pixel
 *   constant is one sequential addition per frame of the half.  A pixel that is not active receives nothing in any of its 2N
 *   accumulators or records.
 *   After the round each pixel that was active in it is frozen iff the following holds for every plane k = 0 .. N - 1, with r0 and r1
 *   plane k's records in half 0 and half 1:
 *     r0.n >= 2  and  r1.n >= 2
 *     n   = r0.n + r1.n >= min_frames
 *     sy  = r0.sum_y + r1.sum_y;   sy2 = r0.sum_y2 + r1.sum_y2          binary64, one rounding each
 *     vp_render_adaptive's criterion holds on (sy, sy2, n) with (rel_tol[k], floor_y[k]): the same binary64 operations in the same
 *     order, false on NaN
 *   -- equivalently: the criterion holds on the record that vp_accumulate_stats makes of a copy of r0 and r1, and each half has at
 *   least two samples.  Freezing sets the FROZEN bit in all 2N records and changes no other flag bit; it is permanent.  The call ends
 *   when no owned pixel is active or the frames are used up.  `result` is as in vp_render_adaptive; `samples` counts one per pixel
 *   and frame, not per plane or half.  A round that the staging cap splits into several launches gives the bits of one launch.
 *   Why pooled, and why two per half: the product is vp_merge_halves of the two halves, and the pooled record measures the standard
 *   error of that merge before any filter; a filter only lowers the variance.  So the rule is conservative for noise -- and says
 *   nothing about the bias a filter adds.  Each half needs n >= 2 because vp_denoise reads a variance from each half's OWN records.
 *   The planes are AND-ed for the reason given under "Adaptive sampling on planes": the gains and the plate are unknown at render time;
 *   a large floor_y[k] (1e30f, say) takes plane k out of the decision.  With a sub-pixel factor a round_frames that is a multiple of
 *   2 S^2 feeds both halves equally in every round; the call takes any round_frames (a round that lies in one half freezes nothing
 *   while the other half has fewer than two samples).
 *   What it is not: bit-equal to vp_render_adaptive on one buffer -- the sums are added in another order, so even the frozen sets may
 *   differ --; and the stopping rule looks at the estimate it stops, the small bias of every adaptive call.  The image of a half is
 *   sum / n per pixel (vp_scale_by_count, or the filters, with THAT half's records).
 *   Refused before the device is touched, every buffer untouched and *result zeroed, with VP_E_ARG: an unknown mode; a NULL pointer
 *   (h0, h1, a used entry, p, a; result excepted); any two of the 2N accumulators equal; any two of the 2N record buffers equal;
 *   max_frames <= 0 or first_frame < 0; min_frames < 2 or round_frames < 1; a used tolerance or floor that is negative or NaN.  Entries
 *   of rel_tol[], floor_y[] and of the vp_plane_bufs beyond the mode's planes are ignored, garbage included.  VP_E_STATE exactly where
 *   the underlying call gives it -- vp_render_adaptive_halves: enabled work counters, as vp_render_adaptive; the plane modes:
 *   VP_ENV_MIS, scalar and multi-channel tracking, enabled work counters, VP_ARITH_FAST --, the message naming this entry point; an
 *   argument error comes before a state error.  VP_E_NOOPACITY as vp_render_frames gives for frame first_frame + max_frames - 1.
 *   Everything else is the underlying halves call's: shards, estimators, streams, vp_set_stream, sub-pixel factors, volume formats
 *   and vp_reserve_frames / vp_reserve_frames_groups behave as there.  It stops look-ahead batches, waits for pipelined launches and
 *   runs on the context's stream, reading three counts back per round (it synchronises); it leaves nothing behind and never modifies
 *   the cached pixel lists.  The render launches are the underlying call's instances on shorter lists, under that mode's census
 *   kind; new are one small pass per ROUND over the active pixels that takes the decision, and the compaction's 4- and 6-record forms.
 *   Still not built: rounds driven by the FILTERED error estimate (vp_cross_error) -- a host can already loop one-round calls around
 *   its own filter, because the frozen set lives in the caller's records --; reduction across processes; VP_ARITH_FAST on plane modes. */
int vp_render_adaptive_halves(vp_float4* d_h0, vp_float4* d_h1, vp_pixel_stats* d_h0_stats, vp_pixel_stats* d_h1_stats,
                              int first_frame, int max_frames, const Param* p, const vp_adaptive* a, vp_adaptive_result* result);
int vp_render_adaptive_planes_halves(int mode, const vp_plane_bufs* h0, const vp_plane_bufs* h1, int first_frame, int max_frames,
                                     const Param* p, const vp_adaptive_planes3* a, vp_adaptive_result* result);

/* ---- Feature pass: ray-marched opacity and depth planes per pixel
 * Every plane above is a Monte-Carlo estimate.  vp_render_features is deterministic: the march of precompute_opacity -- midpoint rule,
 * fixed step -- along each pixel's CAMERA ray, writing the expected per-channel opacity of the pixel and three depths (a Z pass).
 *
 * THE DEFINITION.  binary32 throughout, one rounding per operation, no contraction, in the order written; the exact arithmetic whatever
 * vp_set_arithmetic says (as scale, gamma_correct and vp_denoise).  For every pixel (x, y) the context owns (vp_set_shard), i = y * width + x:
 *   (ro, rd) = camera_ray of the pixel; hit, tn, tf = what intersect_box(ro, rd) leaves -- the seven values vp_test_camera_ray reports
 *   for the pixel in an exact-mode context.  if (tn <= 0.0f) tn = 0.0f (as precompute_opacity).
 *   sy = (0.2126f * sigma_t.x + 0.7152f * sigma_t.y) + 0.0722f * sigma_t.z, once.
 *   Not hit: alpha[i] = (0, 0, 0, 0), depth[i] = (+inf, +inf, +inf, 0).
 *   Hit: s = 0.0f, zf = zt = zb = +inf, cover = 0.0f, reached = false; then for k = 0, 1, 2, ... (k < 2^24: never reached, see step below)
 *       t = tn + ((float)k + 0.5f) * step;      stop as soon as !(t < tf)
 *       rho = sample_density01(ro + rd * t)     -- the integrator's fetch (vp_test_sample_density): current filter mode, any volume format
 *       s = s + rho
 *       if (rho > 0.0f) { if (cover == 0.0f) zf = t;  zb = t;  cover = 1.0f; }
 *       if (!reached && (((s * step) * p->density) * sy >= tau_z)) { zt = t; reached = true; }
 *     and after the loop
 *       tau = (s * step) * p->density
 *       alpha[i].c = 1.0f - expf_(-(tau * sigma_t.c)) for c = x, y, z, expf_ the exact-mode exponential of vp_test_math (which = 1)
 *       alpha[i].w = tau;   depth[i] = (zf, zt, zb, cover)
 *   alpha.xyz: the expected per-channel opacity of the pixel by the midpoint rule -- what 1 - trans.xyz / n of a layers render converges
 *   to; alpha.w: the optical depth per unit sigma_t.  zf / zb: where the ray first / last meets matter; zt: where the luminance optical
 *   depth reaches tau_z (a "surface" depth that ignores wisps; VP_FEATURE_TAU_Z_DEFAULT = ln 2: half of what lies behind is gone).
 *   Depths are distances along the unit camera ray; a depth that does not exist is +inf, the far convention of Z passes, and cover
 *   (1.0f: the ray met matter) tells the two cases apart.
 *   Obeys vp_set_shard (owned pixels only are written), every volume format, cell order, filter mode and estimator setting -- the
 *   estimator only selects which per-pixel tables exist and never changes a result.  Ignores the random stream, the environment, the
 *   sun, brightness, albedo and g; needs a volume and a camera, no environment map.  Asynchronous on the context's stream, behind what
 *   is queued there.  It builds the per-view table and the pixel lists as vp_prepare does (found cached after a render of the view),
 *   stops no look-ahead batch for anything else and leaves nothing behind: a vp_render_frames, plane or adaptive call after it renders
 *   the bits it rendered before.
 *   Performance only, same bits: the box-missing pixel class is filled with its constant, the light class (whole chord certified empty)
 *   with what the definition gives for a march of zeros, and a general pixel starts behind the certified-empty stretch of its chord
 *   (word [4] of vp_get_pixel_table: a step in there adds +0.0f to s and meets none of the three conditions).  VP_NO_FEATURE_SKIP=1
 *   (read when the context first uses its device) switches the three off: every pixel whose ray hits the box marches its whole chord.
 *   VP_E_ARG, before the device is touched and with both buffers untouched: any NULL pointer, d_alpha == d_depth, a step or a tau_z that
 *   is not finite or not > 0, width or height < 1 (or > 65535, as every render call).  VP_E_STATE likewise: no volume or no camera; a
 *   sub-pixel factor above 1 -- NOT BUILT: the box-filtered mean of depths that may be infinite is another definition.  Then, with the
 *   volume's box, VP_E_ARG for a step so small that the box diagonal (computed on the host in binary64) takes more than
 *   VP_FEATURE_MAX_STEPS steps -- no chord is longer, so (float)k stays exact. */
typedef struct { float step, tau_z; } vp_feature_params;   /* 8 bytes */
#define VP_FEATURE_TAU_Z_DEFAULT 0.6931472f            /* ln 2: half of what lies behind is gone */
#define VP_FEATURE_MAX_STEPS (1u << 20)
int vp_render_features(vp_float4* d_alpha, vp_float4* d_depth, const Param* p, const vp_feature_params* fp);

typedef struct
{
    uint64_t samples;
    uint64_t density_lookups; /* trilinear density evaluations of the estimator */
    uint64_t density_loads;   /* of those, the ones that issued a global load */
    uint64_t bound_lookups;
    uint64_t opacity_lookups;
    uint64_t env_lookups;
    uint64_t scatters;
    uint64_t rng_draws;
} vp_counters;
/* counters are collected only while enabled (a separately compiled kernel variant) */
int vp_enable_counters(int on);
int vp_read_counters(vp_counters* out, int reset); /* synchronises */

/* kernel time of the render launches since the last reset, measured with HIP events on the
 * launch stream; synchronises.  At most 64 launches are kept pending: older ones are folded into the running sum when
 * their events have completed, so a host that never asks does not accumulate events. */
int vp_render_time_ms(double* total_ms, int* launches, int reset);

/* The same per pixel class: ms[0] the general kernel (pixels whose camera ray can meet the medium), ms[1] the
 * light kernel (the whole chord is certified empty), ms[2] the fill of the pixels whose ray misses the box; HIP events around each
 * kernel on the stream it runs on (the first two run side by side, so the times overlap).  pixels[] = the pixels of each class
 * in the current lists of this context.  Either pointer may be NULL.  Synchronises. */
int vp_render_class_time_ms(double ms[3], unsigned pixels[3], int reset);

/* How the last render launch of this context took its general pixels' camera rays to the medium: 0 = the integrator walked them
 * itself (one-frame launches, counting launches, scalar / MIS builds, VP_NO_APPROACH), 1 = approach_k / approach_local_k walked the
 * certified-empty stretch ahead of it, 2 = as 1 with the walked throughput looked up by the number of steps (a global-majorant
 * medium whose null collision in empty space is not neutral).  Never changes a result. */
int vp_last_approach_mode(void);
/* 1 if that walk (decomposition estimator, launches of 64 frames and more) read the restart segments of each pixel's camera ray from
 * the per-view table (approach_segments_k) instead of setting them up per sample; VP_NO_APPROACH_TABLE=1 switches the table off. */
int vp_last_approach_table(void);
/* 1 if the last render call of this context wrote its light class (pixels whose camera ray meets empty cells only) as per-pixel
 * constants (miss_fill_k: a null collision in empty space leaves a throughput of 1 as it is in this medium), 0 if it integrated it. */
int vp_last_light_const(void);
/* How the last render launch of the decomposition estimator read its brick table: 0 from global memory, 1 as 16-bit (max,min) pairs
 * staged through LDS, 2 as 2-bit codes into a four-entry palette staged through LDS beside the cold per-path state (tables with at
 * most four distinct pairs -- binary volumes --, achromatic media, timed launches of the counter-based streams).  Performance
 * only: the three forms render the same bits (VP_NO_LDS_BOUNDS / VP_NO_LDS_COMPACT select them). */
int vp_last_lds_form(void);
/* VP_ARITH_EXACT / VP_ARITH_FAST: the arithmetic mode of the last render call of this context (its general pixels ran in that mode;
 * the other pixel classes are the same in both) */
int vp_last_arithmetic(void);
/* Staged vp_render_frames calls alternate between two render targets, each with its own staging and its own internal stream, so that
 * the start of a call runs in the tail of the one before; the write into d_output stays on the context's stream, ordered as before.
 * On by default where both targets fit (VP_NO_PIPELINE=1 switches it off for the process); never changes a result.  vp_set_pipeline
 * waits for pipelined launches in flight first.  vp_last_pipelined: 1 if the last render call of this context ran on such a target. */
int vp_set_pipeline(int on);
int vp_last_pipelined(void);
/* test hook: look-ahead batches this context has launched so far (render_kernel's staged frames), and how many of them were told to
 * stop while they were still running (a setter, a camera move); either pointer may be NULL */
int vp_lookahead_stats(unsigned* launched, unsigned* cancelled_in_flight);
/* Builds everything a render of this Param would build first -- the per-pixel tables of the current camera, the pixel lists
 * of the shard, the sun table -- and waits for it.  A host that moves the camera may call it to take that work out of its
 * first frame; bench.py times it (per_camera_setup_ms).  Not needed for correctness: render_kernel does the same on demand. */
int vp_prepare(const Param* p);
/* Sizes the per-launch sample staging for a coming vp_render_frames(…, n_frames, p) job of this context now (the reference's host
 * allocates its buffers at start-up too): the first launch of the job then finds its buffer instead of allocating up to 16 GiB
 * inside the caller's timed region.  Optional; never changes a result; does nothing for one-frame calls. */
int vp_reserve_frames(const Param* p, int n_frames);
/* test hook: the pixel lists of this context for p (after vp_prepare): dst[0 .. counts[0]) the general pixels, then counts[1]
 * light ones, then counts[2] whose camera ray misses the box, each y << 16 | x in tile order; dst may be NULL to ask for the counts */
int vp_get_pixel_lists(const Param* p, uint32_t* dst, size_t count, unsigned counts[3]);

/* the derived tables, for tests: bound table dims/brick and a device->host copy */
int vp_get_bound_table(void* dst, size_t bytes, int* bnx, int* bny, int* bnz, int* brick, int* radius);
int vp_get_opacity(float* dst, size_t count);
/* the per-pixel table of the current estimator / camera / volume for a width x height image, 8 floats per pixel:
 * [0..2] where the restart crawl in front of the volume ends (local-majorant estimators; the camera origin otherwise),
 * [3] its segment and draw counts (bits: segments | draws << 16), [4] the distance from there up to which the camera ray is
 * certified to meet only empty cells, [5] the pixel class (0 general; 1 the whole chord is certified empty: light kernel; 2 the
 * camera ray misses the box: one constant per pixel), [6..7] unused.  Test hook for the certificates. */
int vp_get_pixel_table(const Param* p, float* dst, size_t count);
/* test hook: the per-view segment table of the decomposition estimator's approach walk (approach_segments_k), built as vp_prepare
 * builds it.  *cap = the records a pixel's chain can hold.  dst (count >= n_general * 2 * *cap * 4 floats; NULL: *cap only, nothing is built)
 * receives, for slot s = 0 .. n_general - 1 -- the order the walk reads them in, which is the order of the general pixels in
 * vp_get_pixel_lists: slot s is the pixel dst[s] of that call -- 2 * *cap records of 4 floats: record n < *cap = (t_near, t_far,
 * bits: the brick's maximum byte | stop << 8, certified-empty distance left at the segment's start), record *cap + n = the origin
 * of segment n (x, y, z, 0).  A chain ends at its first record with the stop bit; the records behind it are not written.
 * VP_E_STATE where this configuration has no table: float and binary16 volumes, the other estimators, VP_NO_APPROACH_TABLE=1, or
 * no approach walk at all. */
int vp_get_segment_table(const Param* p, float* dst, size_t count, int* cap);
/* test hook: the per-view ray table of the global-majorant integrator (ray_table_k), built as vp_prepare builds it: what the set-up of
 * a fresh sample computes from its pixel alone, read by render_k instead.  dst (count >= n_general * 8 floats) receives, for slot
 * s = 0 .. n_general - 1 in the order of the general pixels of vp_get_pixel_lists, (rd.x, rd.y, rd.z, t_near, t_far, t_empty, 0, 0):
 * the camera ray's direction, the raw (unclamped) outputs of the box test for it, and word [4] of the pixel's vp_get_pixel_table
 * entry.  No hit flag: t_far > t_near && t_far >= 1e-3f.  VP_E_STATE where this configuration has no table: the other estimators, a
 * sub-pixel factor, no general pixel, VP_NO_RAY_TABLE=1.  Performance only: with and without it render_k computes the same bits.
 * vp_last_ray_table: 1 if the last render launch of this context's general class read it. */
int vp_get_ray_table(const Param* p, float* dst, size_t count);
int vp_last_ray_table(void);
/* test hook: out[6 i ..] = (rd.x, rd.y, rd.z, t_near, t_far, hit as 1.0f / 0.0f): the camera ray of pixel (pixels[i] & 0xffff,
 * pixels[i] >> 16) of a width x height image and the box test for it, computed by the device functions render_k calls, in the
 * arithmetic unit of the context's mode (vp_set_arithmetic).  VP_E_ARG for a pixel outside the image. */
int vp_test_camera_ray(unsigned width, unsigned height, const uint32_t* pixels, float* out, int n);
/* Counter-based streams (VP_RNG_PHILOX / VP_RNG_PHILOX7): a shadow ray draws from a sub-stream of its own, so the path's later
 * draws do not depend on the number of steps it takes, and a sun shadow ray ends once it has only empty cells in front of it.
 * dst[cell] (x fastest, count >= nx*ny*nz) = that distance from anywhere in the cell, in units of *step (world units), or
 * 0xffff = unknown (the ray is walked to its end).  Test hook for the certificate; VP_NO_SUN_CLIP=1 switches the table off. */
int vp_get_sun_clip_table(unsigned short* dst, size_t count, float* step);
/* Exit flights (any stream): a path in empty space that can meet empty cells only on its way out of the box, and whose null
 * collisions leave its throughput bit for bit as it is, ends with the environment whatever it draws, and is ended at once instead of
 * walking there.  The certificate for the cells: dst[A * nx*ny*nz + cell] (x fastest within a plane, count >= 3*nx*ny*nz), A = the
 * dominant axis of a direction in cell units (d * N / box extent), bit (e_A > 0) | (e_B > 0) << 1 | (e_C > 0) << 2 with (B, C) the
 * other two axes in increasing order: every cell a ray from anywhere in `cell` with a direction of that class can meet is empty and
 * has empty neighbours.  Test hook for the certificate; VP_NO_EXIT=1 switches the table off. */
int vp_get_exit_table(unsigned char* dst, size_t count);
/* 0: off (every path walks to the box exit); 1: the global-majorant estimator only, where that walk is 800 null collisions per
 * unit length; 2: the decomposition estimator as well (uchar bound tables with at most four distinct maxima), where the walk is one
 * free flight per restart segment.  Until this call is made (and without VP_EXIT_LOCAL): mode 2 on the counter-based streams
 * (+1...4 % on the decomposition workloads), mode 1 on sampler.h.  Performance only: the same bits in every mode. */
int vp_set_exit_flights(int mode);
/* dst[n] = throughput of an unscattered path of the global-majorant estimator after n null collisions in empty space, n < count
 * (spectral tracking: the weight of such a collision is 1 only up to rounding; the light kernel looks the product up by n).
 * Test hook: the sequence is three float32 operations per step and can be restated anywhere. */
int vp_get_null_collision_table(const Param* p, float* dst, size_t count);

/* building blocks exposed for parity tests (device execution, host arrays)
 * vp_test_math: out[i] = helper(in[i]) for the integrator's elementary helpers (vp_math.h): 0 logf_, 1 expf_, 2 / 3 the sine /
 * cosine of sincosf_ (radians), 4 acosf_, 5 atanf_, 6 pow15f_, 7 rcp_, 8 sqrt_, 9 rsqrt_, 10 / 11 the sine / cosine of
 * sincos_turns_ (the argument in turns: sin(2 pi t)).  vp_test_math and vp_test_hg run the helpers of the current context's
 * arithmetic mode (vp_set_arithmetic), as its renders do.  vp_test_math refuses a `which` outside 0..11 and n < 0 with VP_E_ARG
 * before it touches the device. */
int vp_test_math(int which, const float* in, float* out, int n);
/* vp_test_roots: the exact arithmetic's in-range root helpers (vp_math.h: which = 0 sqrt_inrange_, 1 rsqrt_unit_) against the general
 * forms (sqrtf(x), 1.0f / sqrtf(x)) on EVERY binary32 bit pattern in [lo_bits, hi_bits], walked on the device: *mismatches = how many
 * patterns differ, *first_bad = the lowest of them (0xffffffff: none).  VP_E_ARG for another `which`, lo_bits > hi_bits or a null
 * result, before the device is touched; VP_E_STATE in the fast arithmetic mode, which has no such helpers. */
int vp_test_roots(int which, uint32_t lo_bits, uint32_t hi_bits, uint64_t* mismatches, uint32_t* first_bad);
/* vp_test_log_forms: the logarithm of the current arithmetic (vp_math.h: which = 0 logf_, 1 logf_pos_, the form without the answer
 * for 0 that the approach walks take) against the chain as it stood before the exponent's bias was folded into its first constant
 * (kept word for word in the test kernels), bit for bit on EVERY binary32 pattern in [lo_bits, hi_bits], walked on the device.
 * logf_ holds on [0, 0x7f800000], logf_pos_ on [0x00800000, 0x7f800000].  Results and VP_E_ARG as vp_test_roots; runs in both
 * arithmetic modes (in the fast one all three are the hardware's instruction). */
int vp_test_log_forms(int which, uint32_t lo_bits, uint32_t hi_bits, uint64_t* mismatches, uint32_t* first_bad);
/* vp_test_approach_walk: the free-flight walks of the approach kernels (kind 0: approach_k's; kind 1: the inner loop of
 * approach_local_k and approach_local_tab_k) and the loops they replaced (kept word for word in the test kernels), each on n cases
 * with a SCRIPTED stream: next_a() returns the case's words in turn as draws (a word below 512 is a draw of exactly 0; behind the
 * last word every draw is 0), counted in pairs like Philox.  params[4 i ..] = (distance at the start, t_empty, t_end (kind 0) or
 * t_far (kind 1), the majorant's reciprocal), script[4 i ..] = (step cap (kind 0 only), index of the case's first word in `words`,
 * its number of words, the stream's pair index at the start).  out_new / out_ref[5 i ..] = the hand-over as built / as it stood:
 * (bits of the distance reached, steps made, the stream's two state words before the flight in hand, through (kind 1)).  The two
 * agree bit for bit wherever the reciprocal carries no minus sign and a segment needs fewer than 60 000 flights.  VP_E_ARG, before
 * the device is touched, for another kind, n < 0, a null array or a script outside the n_words given. */
int vp_test_approach_walk(int kind, int n, const float* params, const uint32_t* script, const uint32_t* words, uint32_t n_words,
                          uint32_t* out_new, uint32_t* out_ref);
/* vp_test_sun_start: the start of a sun shadow ray -- direction, length and the box test -- as the integrator's instances with the
 * sun row take it (memoised on the exact bits of its operands, decided per wave of 64 consecutive origins) and as it stood (kept
 * word for word in the test kernels), on n collision points origin_xyz[3 i ..] with one sun direction (three floats, any values) and
 * one box (bmin xyz, bmax xyz), in the current context's arithmetic mode.  out_new / out_ref[8 i ..] = (bits of the direction's x, y,
 * z, of the length, of tnear and tfar as intersectBox leaves them; hit; in out_new the branches the origin's wave took: bit 0 = the
 * length and the factor were read, bits 1..3 = the slab reciprocal of x, y, z was read; 0 in out_ref).  The first seven words agree
 * bit for bit for every input.  VP_E_ARG, before the device is touched, for n < 0 or a null array. */
int vp_test_sun_start(int n, const float* origin_xyz, const float* sun_dir, const float* box, uint32_t* out_new, uint32_t* out_ref);
/* vp_test_fetch_split: the texel-centre split of one axis of the density fetch in its two forms -- two steps, pn = s * linv then
 * fma(pn, n, -0.5), and folded, fma(s, linv * n, -0.5), which the fetch takes on an axis whose box scale linv is a power of two
 * (csrc/vp_device.h fetch_scales) -- on count offsets s = p - bmin given as binary32 bit patterns, with n texels on the axis.
 * out_two_step / out_folded[5 i ..] = (cell index and bits of the filter weight of the uchar split; cell index, bits of the weight
 * and the `low` flag of the float split).  The two agree in every word wherever vp_test_fetch_fold_axis(linv, n) is 1.  Exact
 * arithmetic only (the fetch is the same code in both units).  VP_E_ARG, before the device is touched, for count < 0, n outside
 * 1..4096 or a null array. */
int vp_test_fetch_split(float linv, int n, int count, const uint32_t* s_bits, uint32_t* out_two_step, uint32_t* out_folded);
/* vp_test_fetch_fold_axis: 1 where an axis of n texels with the box scale linv = 1 / (bmax - bmin) meets the folded form's
 * preconditions -- linv a positive normal power of two, linv * n finite, 1 <= n <= 4096 -- and 0 elsewhere.  The host's own
 * predicate; needs no device and no volume. */
int vp_test_fetch_fold_axis(float linv, int n);
/* vp_test_fetch_form: the host's fetch scales for the current volume and filter mode, as the launch arguments carry them.  *fold = 1:
 * every axis meets the folded form's preconditions; 0: not (also for point sampling and under VP_NO_FETCH_FOLD=1).  fscale[3] /
 * fmul[3]: the per-axis operands -- (linv * n, 1) on a folded axis, (n, linv) elsewhere.  These are the HOST's values, whatever the
 * volume's format: only the kernels built with the folded fetch read them -- the global-majorant integrator on uchar volumes in the
 * exact arithmetic and vp_test_sample_density on uchar volumes; every other kernel (float and binary16 volumes, the local-majorant
 * estimators, the fast arithmetic) scales in two steps from linv and n and ignores them.  VP_E_STATE without a volume, VP_E_ARG
 * for a null pointer.  Needs no device work. */
int vp_test_fetch_form(int* fold, float* fscale, float* fmul);
/* vp_test_launch_census: which render_k and approach kernels the library compiles, and how often each has been launched.  Every
 * launch names its kernel through a table (csrc/vp_dispatch.h); the library counts the launches per table entry, in host memory,
 * process-wide (all contexts and threads together).  unit: 0 the exact arithmetic's kernels, 1 the fast arithmetic's.  kind: 0
 * render_k, 1 render_k of a layers launch (vp_render_frames_layers), 2 the approach walks.  With launches == NULL and built == NULL
 * the call returns the table length: 10368 for kinds 0 and 1, 18 for kind 2.  Otherwise count must be that length, launches[i]
 * (if given) receives the launches of entry i since the last reset, built[i] (if given) 1 where the unit compiles a kernel for
 * entry i and 0 elsewhere, and reset != 0 zeroes the counters of this unit and kind after they are read.  Needs no device.
 * The index of a render_k instance is mixed radix over its template arguments, the first the most significant:
 *   i = (((((((((EST * 3 + RNG) * 2 + QUANT) * 2 + COUNT) * 3 + LDSB) * 2 + ACH) * 2 + MIS) * 3 + TRK) * 2 + LIGHT) * 2 + CANCEL) * 2 + HALF
 * with EST the VP_EST_* value, RNG the VP_RNG_* value, QUANT a uchar volume (of a LIGHT instance: a uchar bound table), COUNT work
 * counters, LDSB the brick table's LDS form (0 none, 1 byte pairs, 2 two-bit codes), ACH one-channel throughput, MIS active
 * environment sampling, TRK 0 spectral / 1 scalar / 2 multi-channel tracking, LIGHT the light pixel class, CANCEL a look-ahead batch
 * that can be stopped, HALF a binary16 volume.  An approach kernel's is (WALK * 3 + RNG) * 2 + QUANT with WALK 0 approach_k (global
 * majorant), 1 approach_local_k, 2 approach_local_tab_k (the segment table's); QUANT is 1 for walks 0 and 2.
 * VP_E_ARG for another unit or kind, or a count that is not the table length. */
int vp_test_launch_census(int unit, int kind, uint32_t* launches, uint8_t* built, size_t count, int reset);
/* vp_test_groups_census: the same for the table a vp_render_frames_groups launch goes through (the exact unit's; render_k's index and
 * length, 10368), counted apart from the kinds above.  With both arrays NULL the call returns the length; VP_E_ARG for a count that is
 * not the length.  Needs no device. */
int vp_test_groups_census(uint32_t* launches, uint8_t* built, size_t count, int reset);
/* vp_test_group_layers_census: the same for the table a vp_render_frames_group_layers launch goes through, kept apart again. */
int vp_test_group_layers_census(uint32_t* launches, uint8_t* built, size_t count, int reset);
int vp_test_rng(int mode, uint32_t x, uint32_t y, uint32_t frame, uint32_t k0, uint32_t k1, int n, float* out);
int vp_test_sample_density(const float* pos_xyz, float* out, int n);
/* component hooks for known-answer tests against float64 closed forms (no oracle involved):
 * HGPhaseFunction::sample through Frame (kernel.cu:557-598, the phase-function block :2301-2303) and ::evaluate (:600-603);
 * intersectBox (kernel.cu:654-680) against the current volume box; eval_envmap (kernel.cu:956-973, dir_to_uv :882-895) */
int vp_test_hg(const float* g, const float* r0, const float* r1, const float* normal_xyz, const float* cos_query, float* dir_xyz,
               float* eval, int n);
int vp_test_intersect_box(const float* origin_xyz, const float* dir_xyz, int* hit, float* tnear, float* tfar, int n);
int vp_test_eval_envmap(const float* dir_xyz, float* rgb, int n);

/* The procedural Julia-set volume of the reference (FractalJuliaSet, kernel.cu:84-140) voxelised at
 * texel centres over [-1,1]^3 to an n^3 uchar grid (0 / 255), x fastest; written to HOST memory so it
 * can be handed to init_cuda like any other volume. */
int vp_julia_voxelize(int n, unsigned char* host_out);
/* A FLAGGED SYNTHETIC stand-in for the WDAS cloud of BASELINE configs 4/5 (neither the data set nor OpenVDB exists in the build
 * image): five octaves of hashed-lattice value noise, thresholded, with a soft spherical edge, voxelised at texel centres over
 * [-1,1]^3 to n^3 float densities in [0,1] (not binary), x fastest, written to HOST memory -- to be dumped with dump_dense_volume
 * and read back with loadBinaryFile like a converted .vdb.  Deterministic in (n, seed); the oracle restates it bit for bit. */
int vp_cloud_voxelize(int n, uint32_t seed, float* host_out);

/* raw device memory helpers */
void* vp_malloc(size_t bytes);
int   vp_free(void* dptr);
int   vp_memset(void* dptr, int value, size_t bytes);
int   vp_upload(void* dptr, const void* src, size_t bytes);
int   vp_download(void* dst, const void* dptr, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* VOLPATH_H */
