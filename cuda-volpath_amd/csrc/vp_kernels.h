// vp_kernels.h -- launch descriptors and host-callable launchers of vp_kernels.hip
#pragma once
#include <hip/hip_runtime.h>

#include "vp_device.h"

#define VP_BLOCK 256
#ifndef VP_BLOCK_LDS
#define VP_BLOCK_LDS 512              // workgroup size of the LDS-bound-table variant
#endif
#ifndef VP_MIN_WAVES
#define VP_MIN_WAVES 1                // launch-bounds hint: waves per SIMD the register budget must allow
#endif
#define VP_LDS_BYTES_PER_CU (160 * 1024)   // gfx950 (MI355X_MICROARCH.md); the static_assert at render_k's cold state ties the occupancy budgets to it
#define VP_LDS_BOUND_ENTRIES 32768     // (max,min) byte pairs staged in LDS: 64 KiB
#ifndef VP_CHUNK
#define VP_CHUNK 128  // samples a wave takes from a queue per atomic (256 until round 5: at the bench's launch size 128 is +1 % on the
                      // Julia workloads -- finer hand-out at the end of a band --, 64 the same, 512 / 1024 -2 / -4 %: r05_knob_sweeps.txt)
#endif
// One sample queue per XCD: each hands out a contiguous band of the image (all frames of it), so the rays an XCD's
// L2 serves stay in one slab of the volume; a wave starts on the queue of its own XCD and moves on when it runs dry.
#define VP_NQUEUES 8
#define VP_QUEUE_STRIDE 16  // words between queue heads (one cache line each)
// the inner tracking loop of a wave runs until this many lanes are parked on an event, or until
// a parked lane has waited this many steps
// (28 since round 5 -- 24 before: C2 +1.3 % at the bench's launch size with a 0.15 % noise floor, the achromatic local kernels +0...0.3 %;
// the chromatic local kernels take 32: vp_render.cpp, profiles/experiments/r05_knob_sweeps.txt)
#ifndef VP_WAIT_LANES
#define VP_WAIT_LANES 28
#endif
#ifndef VP_WAIT_ITERS
#define VP_WAIT_ITERS 16
#endif
// lanes that must be waiting for a restart-segment set-up before it runs in the middle of a pass (it always runs at the first
// step of a pass)
#ifndef VP_END_LANES
#define VP_END_LANES 4
#endif
#ifndef VP_SETUP_LANES
#define VP_SETUP_LANES 8
#endif
// tracking steps per pass of the inner loop: the wave-level bookkeeping (ballots, wait policy) is paid once per pass
#ifndef VP_LIGHT_MIN_WAVES
#define VP_LIGHT_MIN_WAVES 8   // the light kernels fit 64 vector registers: two of their waves beside four of a 96-register kernel
#endif
#ifndef VP_PROFILE_BLOCKS
#define VP_PROFILE_BLOCKS 0   // 1: the counting kernels also carry cycle stamps, loop statistics and block tallies (scripts/block_profile.py)
#endif
#ifndef VP_GLOBAL_MIN_WAVES
#define VP_GLOBAL_MIN_WAVES 7  // global-majorant kernels: waves per SIMD their register budget is held to.  Seven = 72 registers, no spill, since
                               // intersect_box runs axis by axis (vp_device.h; round 5): C2 3010-3030 -> 3090.  History: six since the cold
                               // per-path state lives in LDS (round 4: 79 registers; it came out at 72 = seven by itself until the event section
                               // read its uniforms from LDS: 79 again, and held to 72 THEN it spilled six: 2743 vs 2999); with the cold state in
                               // registers six cost three spilled registers and lost to five (1190 vs 1341 Msamples/s on C2, round 3)
#endif
#ifndef VP_LIGHT_LOCAL_MIN_WAVES
#define VP_LIGHT_LOCAL_MIN_WAVES 7   // the local-majorant light kernels need 66-68 registers with the Philox2x32-10 and sampler.h streams:
                                     // eight waves cost three or four spilled registers, seven (72) none
#endif
#ifndef VP_LIGHT_STEPS_PER_PASS
#define VP_LIGHT_STEPS_PER_PASS 16
#endif
#ifndef VP_STEPS_PER_PASS
#define VP_STEPS_PER_PASS 4
#endif
// exit flights: the lane counter value from which a lane is tested
#define VP_EXIT_TRIP 64

namespace vp
{
// Pixel-tile deal (include/volpath.h vp_tile_owner): tile (tx, ty) belongs to rank (tx + tile_row_shift(ty)) % world, i.e.
// within a tile row every world-th tile, rows shifted against each other by a hash of the row index.  The host lists a rank's
// tiles (vp_tables.cpp pixel lists); the kernels read the list.
__host__ __device__ inline unsigned tile_row_shift(unsigned ty, unsigned world) { return ((ty * 0x9E3779B1u) >> 15) % world; }
// same values as the VP_EST_* / VP_RNG_* enums of include/volpath.h
constexpr int EST_GLOBAL = 0, EST_DECOMP = 1, EST_BOUNDED = 2;
constexpr int RNG_SAMPLERH = 0, RNG_PHILOX = 1, RNG_PHILOX7 = 2;

// one render launch: frames [frame0, frame0+nframes) x a list of pixels (one class of the pixels this rank owns)
struct LaunchDev
{
    ParamDev P;
    int      frame0, nframes;
    unsigned nslots;        // pixels of THIS launch (its slice of the pixel list) = samples per frame
    unsigned total_items;   // nframes * nslots
    const unsigned* pixels; // pixel of slot s: pixels[s] = y << 16 | x.  The rank's pixels (those of its 8x8 tiles, tile by tile) are
                            // listed class by class: general pixels, then "light" pixels whose camera ray meets empty cells only;
                            // a launch covers one class
    unsigned stage_stride;  // samples per frame in `stage`, all classes together
    unsigned slot_base;     // first sample slot of this launch's class within a frame of `stage`
    float4*  out;           // W*H accumulator (caller-owned)
    float4*  stage;         // [nframes][stage_stride] per-sample results, or null = accumulate directly
    const float4* crawl;    // per pixel two float4, or null: [0] = where the restart crawl in front of the volume ends and its segment /
                            // draw counts (crawl_table_k, local-majorant estimators), [1].x = certified-empty distance from there,
                            // [1].y = pixel class (0 general, 1 the whole chord is certified empty, 2 the ray misses the box)
    unsigned* queue;        // VP_NQUEUES sample-queue heads, VP_QUEUE_STRIDE words apart (zeroed before the launch)
    unsigned chunk_fshift;  // log2 of the frames a chunk spans (0: a chunk is VP_CHUNK pixels of one frame; 6: four pixels x 64 frames); nframes is a multiple
    unsigned q_start[VP_NQUEUES + 1];  // slot range [q_start[q], q_start[q+1]) of a frame that queue q hands out
    unsigned long long* counters;  // work counters, loop statistics and block tallies (vp_state.h kCounterWords) or null
    unsigned key0, key1;    // Philox key
    unsigned wait_lanes, wait_iters;  // inner-loop exit policy (VP_WAIT_LANES / VP_WAIT_ITERS)
    unsigned end_lanes;     // lanes that must ask for the path-end chain (environment, write, refill) before it runs in a visit (VP_END_LANES;
                            // it also runs every fourth visit, and whenever no lane of the wave is tracking)
    unsigned setup_lanes;   // lanes that must ask for a segment set-up before it runs mid-pass (VP_SETUP_LANES; 1 = at every step)
    // Counter-based streams: per cell of the volume, the distance (in steps of clip_ds, 0xffff = unknown) beyond which a ray from
    // anywhere in the cell toward the sun meets empty cells only (sun_clip_k); a sun shadow ray ends there.  Null = walk to the end.
    const unsigned short* sun_clip;
    float    clip_ds;
    unsigned count_clips;   // counting build: 0 = walk every shadow ray to its end (density_lookups = the estimator's count, as the oracle's),
                            // 1 = end them where the timed build does (VP_DEBUG_COUNT_CLIPS: block tallies of what the timed kernels execute)
    const float* thr_table; // light kernel of the global-majorant estimator: thr_table[n] = throughput after n null collisions in empty
    unsigned thr_n;         // space (thr_table_k: a function of n alone there), n < thr_n; beyond the table the recurrence is run
    // Counter-based streams: approach_k (global majorant) / approach_local_k (decomposition) has walked the camera ray of every sample
    // of this launch through its certified-empty stretch already and left (distance reached, draw pairs used) / (segment origin, pairs
    // used) in the sample's staging slot; the integrator takes a new sample up from there.  0 = start as the reference does.
    // The brick table of the decomposition estimator in its compact form (render_k<..., LDSB = 2>): where it holds at most four distinct
    // (max,min) byte pairs -- a binary volume: three -- 2-bit codes (sixteen per word, brick order, padded to 16 bytes) and the palette
    // (pair 0 | pair 1 << 16, pair 2 | pair 3 << 16); built with the volume (vp_context.cpp), null otherwise
    // (the fields themselves: at the END of this struct -- appended, so that the offsets the other kernels read do not move)
    uint2*   approach_aux;    // decomposition estimator: the stream's state per staging slot (the slot holds the segment origin and the distance
                              // reached in it): .x = pair index (counter-based) / sampler.h's two words
    unsigned approach;        // 1: the walk's null collisions leave the throughput at 1; 2 (global majorant): look it up by their number in thr_table
    unsigned approach_fshift; // log2 of the frames a wave of the approach kernels spans (6 where the launch has 64 frames or more)
    unsigned approach_steps;  // most free-flight steps (restart segments) the walk makes per sample (the integrator does what is left)
    // Exit flights (render_k).  A path that can meet certified-empty cells only on its way out of the box, and whose null collisions
    // there leave its throughput bit for bit as it is, ends with the environment whatever it draws: it is ended at once.
    // exit_oct: three byte planes (one per dominant axis of a direction in cell units), per cell eight bits, one per class of signs:
    // every cell of the quarter pyramid that opens from this cell in that class of directions has no non-empty cell in its 3x3x3
    // neighbourhood (exit_dir_slice_k); null = off.
    const unsigned char* exit_oct;
    int      exit_start;      // a lane counts its null collisions in empty space from here and is tested from VP_EXIT_TRIP on:
                              // VP_EXIT_TRIP - K (VP_EXIT_K); far below zero when the test is off
    unsigned exit_nbytes;     // local-majorant estimators: how many distinct bytes occur as maxima in the bound table (1..4, else off) ...
    unsigned exit_bytes;      // ... and the bytes, packed: every majorant a segment in empty cells can have
    // Look-ahead batches (render_kernel's staged frames) can be told to stop: the host writes the number of the newest batch of this
    // slot that is no longer wanted into *cancel (numbers only grow: nothing is ever re-armed); a batch whose number is not above it
    // hands out no more samples -- render_k asks at every chunk it takes, the approach kernels when they start.  Null = never cancelled.
    unsigned* cancel;
    unsigned  batch_id;
    // Samples that are per-pixel CONSTANTS of a launch (the box-missing pixels always; the light class where a null collision in empty
    // space is neutral: miss_fill_k) are staged ONCE, in the row of the launch's first frame: slots from const_from on.  reduce_stage_k
    // adds such a sample nframes times, in the order it would add nframes staged copies: the same bits, without 2 x 16 bytes of
    // traffic per sample for 88 % of BASELINE config 2's samples.  (Fields appended: the offsets render_k reads do not move.)
    unsigned      const_from;    // first slot (of the rank's pixel list) whose sample is a constant of the launch; >= nslots: none
    const float4* stage_const;   // the staging row that holds the constants (the first frame of the batch the frames come from)
    const unsigned* bound_codes;   // the compact brick table (above): 2-bit codes ...
    unsigned        bound_pal[2];  // ... and the palette
    // decomposition estimator, uchar bound table: per pixel slot of the general class the chain of restart segments of its camera
    // ray through certified-empty cells (approach_segments_k: segment_table_records() float4 per slot); null: approach_local_k sets
    // every segment up per sample
    const float4* seg_table;
    // Sub-pixel sampling (include/volpath.h vp_set_subpixel; appended like the fields above): log2 of the factor S, 0 = off.  A sample of
    // pixel (x, y) in frame f is computed for pixel (S x + i, S y + j) of the S W x S H image (vp_device.h subpixel_offset): `crawl` is
    // then that image's table, `pixels`, `out`, `stage` and P stay the W x H image's.  The host launches no approach walk, no segment
    // table and no constant rows with it (vp_render.cpp).
    unsigned sub_shift;
    // A layers launch (include/volpath.h vp_render_frames_layers; appended like the fields above): 1 = a sample that reaches the
    // environment unscattered is staged as (max(thr, 0), -heat) -- its throughput, no background, no brightness; the sign bit of w,
    // -0.0f included, marks it (the light kernel, whose every sample is one, stages heat as it is) -- and the reduce (split_sample) splits the
    // staged samples into the two accumulators.  0: the beauty sample, as ever.
    unsigned layers;
    // Global-majorant estimator, general class (appended like the fields above): per pixel slot of the class what a fresh sample's
    // set-up computes from the pixel alone (ray_table_k: two float4 per slot, sliced like `pixels`) -- [0] = (rd.x, rd.y, rd.z, t_near),
    // [1] = (t_far, t_empty, 0, 0): camera_ray()'s direction, intersect_box()'s raw outputs for it and the crawl table's [1].x.  The hit
    // flag is not stored: t_far > t_near && t_far >= 1e-3f.  Null (no memory, a sub-pixel factor, a caller's own lists, the light
    // class, VP_NO_RAY_TABLE=1): render_k computes them per sample, same bits.
    const float4* ray;
    // A light-groups launch (include/volpath.h vp_render_frames_groups; appended like the fields above): the second staging plane, laid
    // out like `stage` (frame * stage_stride + slot) and lying behind the launch's last staged frame.  render_k's GRP instances and the
    // constant writers stage the sky group's sample there and the sun group's in `stage`; the reduce adds the two planes into the
    // two accumulators.  Null: not a groups launch.
    float4* groups;
};

// render_k and the approach kernels: which instance a launch runs, and which of them a build compiles, is decided in vp_dispatch.h.
// A request for an instance that the build lacks (the API refuses every such configuration first: vp_render.cpp check_render) ends here:
[[noreturn]] void kernel_not_built();
// The planes of a render call.  A call has one to three planes; a staged sample splits into one sample per plane by the rule of the
// call's mode (split_sample, vp_kernels.hip).  The mode is two bits -- layers, groups -- and is also which of render_k's LYR / GRP
// instances the call launches (vp_dispatch.h):
//   PLANES_ONE           out                 the beauty sample, whole
//   PLANES_LAYERS        fg, trans           an unscattered path's throughput goes to trans, its heat to fg; any other sample to fg
//   PLANES_GROUPS        sun, sky            the first staging plane to sun, the second (LaunchDev::groups) to sky
//   PLANES_GROUP_LAYERS  sun, sky, trans     unscattered: as a layers call, the heat to both groups; else as a groups call
// A fifth constant is no mode of render_k (kPlaneModes stays the number of those) and names a reduce instance only: its launches are
// PLANES_ONE's, instance for instance -- the beauty kernels, their walks and constant writers, one staging plane, LaunchDev::layers 0
// and LaunchDev::groups null, census kind CENSUS_RENDER --, and only the reduce knows it:
//   PLANES_HALVES        h0, h1              the beauty sample of frame f, whole, to plane half_of_frame(f) ALONE; the other plane
//                                            receives no sample of that frame -- no +0.0f, no count (include/volpath.h
//                                            vp_render_frames_halves_stats).  Records always; no adaptive instance of the reduce.
// Halves are orthogonal to the split mode (PlaneSet::halves): "mode M, two halves" launches what mode M launches -- its render_k
// instances, staging planes and census kind -- and the reduce hands the N samples that split_sample<M> makes of frame f to the N planes of
// half half_of_frame(f) alone (include/volpath.h vp_render_frames_planes_halves_stats; reduce_plane_halves_k).  PLANES_HALVES above is
// "PLANES_ONE, two halves": the constant stays the name of that reduce instance and is no value of PlaneSet::mode.
constexpr int PLANES_ONE = 0, PLANES_LAYERS = 1, PLANES_GROUPS = 2, PLANES_GROUP_LAYERS = 3, kPlaneModes = 4, PLANES_HALVES = 4, kMaxPlanes = 3;
constexpr int plane_mode(bool layers, bool groups) { return (layers ? PLANES_LAYERS : 0) | (groups ? PLANES_GROUPS : 0); }
constexpr int planes_of(int mode) { return mode == PLANES_ONE ? 1 : mode == PLANES_GROUP_LAYERS ? 3 : 2; }
// the half a frame belongs to: blocks of S^2 = 4^sub_shift consecutive ABSOLUTE frames alternate (S = 1: even frames 0, odd frames 1)
__host__ __device__ constexpr int half_of_frame(int frame, unsigned sub_shift) { return (int)(((unsigned)frame >> (2u * sub_shift)) & 1u); }
// The launch census (test hook: include/volpath.h vp_test_launch_census).  The launchers of vp_dispatch.h call census_record() with the
// table index of the kernel they are about to name: one host increment per launch, nothing on the device.  unit: 0 the exact
// translation unit, 1 the fast arithmetic's; kind: CENSUS_* -- one table per plane mode of render_k (census_of_planes), and the
// approach walk's.  The public hook takes the first three kinds; the groups and group-layers tables have entry points of their own
// (vp_test_groups_census, vp_test_group_layers_census), views of the same store.
constexpr int CENSUS_RENDER = 0, CENSUS_LAYERS = 1, CENSUS_APPROACH = 2, CENSUS_GROUPS = 3, CENSUS_GROUP_LAYERS = 4;
constexpr int census_of_planes(int mode) { return mode < PLANES_GROUPS ? mode : mode + 1; }
void census_record(int unit, int kind, unsigned index);
// the read side: the table length of a kind (0: no such kind); launches[i] = launches since the last reset, built[i] = 1 where the
// unit compiles instance i (either array may be null; count = the table length); reset zeroes the counters after they are read
size_t census_size(int kind);
void census_read(int unit, int kind, unsigned* launches, unsigned char* built, size_t count, bool reset);
// built[i] of one unit, from the constexpr functions of vp_dispatch.h as that unit compiled them (vp_kernels.hip / vp_kernels_fast.hip)
void census_built(int kind, unsigned char* built, size_t count);
void census_built_fast(int kind, unsigned char* built, size_t count);
// lds_form: how the decomposition estimator reads its brick table -- 0 global memory, 1 the 16-bit table through LDS (512-thread
// workgroups), 2 2-bit codes into a four-entry palette through LDS (LaunchDev::bound_codes; 256-thread workgroups, plain occupancy)
// half (with quant = false): binary16 cells (SceneDev::cells_f16); everything else of such a volume is the float volume's
void launch_render(const SceneDev& S, const LaunchDev& L, int est, int rng, bool quant, bool half, bool count, int lds_form, bool mis, int trk,
                   int blocks, hipStream_t st);
// the same in the fast arithmetic mode (vp_kernels_fast.hip): counter-based streams, spectral tracking, passive environment, global
// majorant or decomposition, no counters -- the host refuses the rest before it launches
void launch_render_fast(const SceneDev& S, const LaunchDev& L, int est, int rng, bool quant, bool half, bool count, int lds_form, bool mis, int trk,
                        int blocks, hipStream_t st);
// the light pixel class (spectral tracking): pixels whose camera ray meets empty cells only
void launch_render_light(const SceneDev& S, const LaunchDev& L, int est, int rng, bool quant, bool count, int blocks, hipStream_t st);
// (with LaunchDev::sub_shift: subpixel_fill_k, one constant per fine pixel, staged for every frame)
void launch_miss_fill(const SceneDev& S, const LaunchDev& L, bool local_estimator, hipStream_t st);
// the camera rays' free flights through certified-empty cells, one thread per sample of the launch (approach_k); rng: RNG_PHILOX*
void launch_approach(const SceneDev& S, const LaunchDev& L, int est, int rng, bool quant, hipStream_t st);
void launch_approach_fast(const SceneDev& S, const LaunchDev& L, int est, int rng, bool quant, hipStream_t st);
// the per-pixel segment table of the decomposition estimator's approach walk (approach_segments_k): float4 per slot, and its builder
unsigned segment_table_records(void);
void launch_segment_table(const SceneDev& S, unsigned width, unsigned height, const float4* crawl, const unsigned* pixels, unsigned nslots, float4* seg,
                          hipStream_t st);
// the per-pixel ray table of the global-majorant integrator (ray_table_k; LaunchDev::ray): two float4 per slot of `pixels`; crawl may be null (t_empty = 0)
void launch_ray_table(const SceneDev& S, unsigned width, unsigned height, const float4* crawl, const unsigned* pixels, unsigned nslots, float4* table,
                      hipStream_t st);
// throughput of an unscattered global-majorant path after n null collisions with density +0, n = 0..count-1 (thr_table_k)
void launch_thr_table(const ParamDev& P, float* table, unsigned count, hipStream_t st);
// mask[8]: the bytes that occur as a maximum in a uchar bound table; flag[0] (preset to 1) is cleared unless a null collision in
// empty space leaves a throughput of 1 unchanged for every sigma_t' a light path can meet (light_identity_k)
void launch_bound_bytes(const unsigned char* bounds, size_t nbricks, unsigned* mask, hipStream_t st);
void launch_light_identity(const ParamDev& P, bool local, const unsigned* mask, unsigned* flag, hipStream_t st);
void launch_light_identity_fast(const ParamDev& P, bool local, const unsigned* mask, unsigned* flag, hipStream_t st);   // (vp_kernels_fast.hip)
// the rank's pixel lists, class by class, on the GPU (pixlist_*_k): d_row_start[tiles_y + 1] = first owned tile of each tile row,
// d_block_counts[3 * pixel_list_blocks(ntiles)] scratch, d_totals[3] = pixels per class (general, light, box-missing)
inline unsigned pixel_list_blocks(unsigned ntiles) { return (unsigned)(((size_t)ntiles * 64 + 1023) / 1024); }
void launch_pixel_lists(unsigned width, unsigned height, unsigned rank, unsigned world, unsigned ntiles, const unsigned* d_row_start,
                        const float4* table, const unsigned char* cls, unsigned* d_block_counts, unsigned* d_totals, unsigned* d_out, hipStream_t st);
// sub-pixel sampling: cls[width * height] = the class of each pixel of the width x height image from the table `fine` of the
// (width << shift) x (height << shift) image (subpixel_class_k); launch_pixel_lists then reads cls instead of a table
void launch_subpixel_classes(const float4* fine, unsigned width, unsigned height, unsigned shift, unsigned char* cls, hipStream_t st);
void launch_env_tables(const float4* env, int w, int h, float* lum, float* row_sum, float* cdf_x, float* cdf_y, float* pdfnorm_alt,
                       hipStream_t st);
void launch_crawl_table(const SceneDev& S, bool quant, unsigned width, unsigned height, bool control_draw, const unsigned char* danger, float4* table,
                        hipStream_t st);
// marked (may be null): a device counter that receives the number of cells marked (a non-empty cell in the 3x3x3 neighbourhood)
void launch_danger(const SceneDev& S, bool quant, bool half, unsigned char* out, unsigned long long* marked, hipStream_t st);
float sun_clip_step(const SceneDev& S);  // the table's distance unit: a quarter of the smallest cell edge
void launch_sun_clip(const SceneDev& S, const unsigned char* danger, float ds, unsigned short* out, hipStream_t st);
void launch_empty_table(const SceneDev& S, unsigned width, unsigned height, const unsigned char* danger, float4* table, hipStream_t st);
// the direction table of the exit flights from the danger volume: planes = 3 * nx*ny*nz bytes; one small kernel per slice and direction
void launch_exit_table(const unsigned char* danger, unsigned char* planes, int nx, int ny, int nz, hipStream_t st);
// the reduce of a one-plane launch without statistics (reduce_stage_k): the call the benchmark times, and the look-ahead's
void launch_reduce(const LaunchDev& L, hipStream_t st);
// Per-pixel statistics (include/volpath.h vp_pixel_stats, the same 24 bytes)
struct PixelStatsDev { double sum_y, sum_y2; unsigned n, flags; };
// What a render call accumulates into, as the host describes it (do_render; vp_adaptive.cpp): the planes of its mode in the order of
// the table above, each with an accumulator and -- all planes or none -- a record buffer; an adaptive call adds each plane's criterion.
struct PlaneSet
{
    int            mode;                // PLANES_ONE .. PLANES_GROUP_LAYERS: the split rule, and render_k's two bits
    bool           halves;              // two halves of the mode's planes: half h's plane k is entry h * n() + k; records always
    float4*        acc[2 * kMaxPlanes]; // count() accumulators of width * height pixels
    PixelStatsDev* rec[2 * kMaxPlanes]; // their records, indexed like the accumulators; rec[0] null: a call without statistics
    double         tol[kMaxPlanes], fl[kMaxPlanes];   // adaptive: each plane's tolerance and floor (the binary32 arguments widened); n() entries, halves or not
    unsigned       min_frames;          // adaptive: the samples a record needs before its criterion is asked (halves: the two halves' records of a plane together)
    bool           adaptive;            // a round of an adaptive call: its last launch freezes; false: `flags` is neither read nor written
                                        // (with halves the reduce never freezes: the round loop launches launch_freeze_halves after the round)
    int  n() const { return planes_of(mode); }
    int  count() const { return halves ? 2 * n() : n(); }   // the buffers of each kind the caller hands in
    bool layers() const { return (mode & PLANES_LAYERS) != 0; }   // (render_k's two bits, with halves or without)
    bool groups() const { return (mode & PLANES_GROUPS) != 0; }
    bool stats() const { return rec[0] != nullptr; }
};
// The reduce of a staged launch into the planes of S (reduce_planes_k<MODE, STATS, ADAPT>): per slot of L.pixels the staged frames in
// frame order, each split into one sample per plane; every plane's sample is added to its accumulator (S.acc[0] is L.out) and, with
// records, its luminance to the plane's record by the definition of vp_pixel_stats.  The slots [light_from, light_to) of the list are
// the light kernel's, whose samples are unscattered without carrying the mark (layers modes).  last: the last launch of the call --
// where S.adaptive, the one that evaluates the criterion: all records of a slot are frozen iff each has S.min_frames and meets the
// criterion with its own n, tolerance and floor (a record frozen on a part of a round would stay frozen).
void launch_reduce_planes(const LaunchDev& L, const PlaneSet& S, unsigned light_from, unsigned light_to, bool last, hipStream_t st);
// The freeze of an adaptive round on halves (freeze_halves_k<N>; include/volpath.h vp_render_adaptive_halves): one thread per slot of
// `pixels` -- the round's active list --, which sets FROZEN in all 2 n() records of a slot iff every plane has two samples in each half,
// S.min_frames in both together and meets its criterion on the pooled record; nothing else is written.  S.halves && S.adaptive.
void launch_freeze_halves(const unsigned* pixels, unsigned nslots, unsigned width, const PlaneSet& S, hipStream_t st);
// the pixels of the class-ordered list src (n[0] general, n[1] light, n[2] box-missing) that are frozen in none of S's records, in
// src's order, class by class, into d_out (room for all of src), and their three counts into d_totals; S.count() records per slot: 1, 2, 3, 4 or 6;
// d_block_counts[3 * compact_blocks(n)] scratch
inline unsigned compact_blocks(unsigned n) { return (n + 1023u) / 1024u; }
void launch_compact_active(const unsigned* src, const unsigned n[3], unsigned width, const PlaneSet& S, unsigned* d_block_counts, unsigned* d_totals,
                           unsigned* d_out, hipStream_t st);
void launch_scale_by_count(float4* dst, const float4* src, const PixelStatsDev* stats, int size, float s, hipStream_t st);
// the merge of two half-buffer MEAN images by their records' counts and the residual map of their disagreement (merge_halves_k;
// include/volpath.h vp_merge_halves): resid may be null, dst may be a or b
void launch_merge_halves(float4* dst, float* resid, const float4* a, const PixelStatsDev* a_stats, const float4* b, const PixelStatsDev* b_stats, int size,
                         float floor_y, hipStream_t st);
// dst += src for records: binary64 sums, n added, flags or-ed (accumulate_stats_k)
void launch_accumulate_stats(PixelStatsDev* dst, const PixelStatsDev* src, size_t n, hipStream_t st);
void launch_stats_rel_error(float* dst, const PixelStatsDev* stats, int size, float floor_y, hipStream_t st);
// the NL-means filter of the output stage (vp_denoise.hip; include/volpath.h vp_denoise, vp_denoise_guided, vp_denoise_var): weights from
// (guide, gstats), colours from (src, stats), k2 = k * k; form 0 tiled through LDS, 1 one thread per pixel from global memory.
//   feat.n == 0: the plain weight, denoise_lds_bytes(R, F) of LDS per workgroup in form 0.
//   feat.n >= 1: the feature term as well; chan[j] is the address of feature j's channel at pixel 0 (pixel i at chan[j][4 * i]),
//     g[j] = 1 / (2 sigma_j^2) as the host rounded it.  Form 0 stages the channels into n more LDS planes:
//     denoise_guided_lds_bytes(R, F, n) dynamic bytes per workgroup, which the caller holds against DENOISE_LDS_LIMIT before it launches.
//   svar != null: the guide's variance from the caller's per-sample plane, v = svar * s in place of the records' variance; the same
//     kernels with the plane as one more parameter, LDS as theirs.
struct DenoiseFeaturesDev { const float* chan[4]; float g[4]; int n; };
// what a workgroup may take without an attribute call, less the kernels' 256 static bytes (the vote of __syncthreads_or)
constexpr size_t DENOISE_LDS_LIMIT = 64 * 1024 - 256;
size_t denoise_lds_bytes(int R, int F);
size_t denoise_guided_lds_bytes(int R, int F, int n_features);
void launch_denoise(float4* dst, const float4* src, const PixelStatsDev* stats, const float4* guide, const PixelStatsDev* gstats, const float* svar,
                    const DenoiseFeaturesDev& feat, int W, int H, int R, int F, float k2, int form, hipStream_t st);
// the pooled per-sample luminance variance u of two halves' records and the noise q of that estimate (halves_variance_k; include/volpath.h
// vp_halves_variance): q may be null
void launch_halves_variance(float* u, float* q, const PixelStatsDev* a_stats, const PixelStatsDev* b_stats, int size, hipStream_t st);
// the filter on the scalar plane u with the noise q of its values (include/volpath.h vp_filter_variance): form 0 tiled through
// variance_lds_bytes(R, F) of LDS per workgroup (less than denoise_lds_bytes(R, F): no colour planes), 1 one thread per pixel
size_t variance_lds_bytes(int R, int F);
void launch_filter_variance(float* dst, const float* u, const float* q, int W, int H, int R, int F, float k2, int form, hipStream_t st);
// one candidate's per-pixel error estimate from the two filtered halves fa, fb against the unfiltered means of the other half
// (cross_error_k; include/volpath.h vp_cross_error)
void launch_cross_error(float* err, const float4* fa, const float4* fb, const float4* h0, const PixelStatsDev* s0, const float4* h1, const PixelStatsDev* s1,
                        int size, hipStream_t st);
// per-pixel selection among n candidates (vp_denoise.hip; include/volpath.h vp_select): the error planes box-smoothed at radius Rs, the
// smallest picked, the picks blended over radius Rb; index may be null.  Form 0 tiled through select_lds_bytes(n, Rs, Rb) of LDS per
// workgroup (at most 19248: n = 4, radii 3), 1 one thread per pixel from global memory.  The arrays travel by value in the arguments
constexpr int SELECT_MAX = 4;
struct SelectDev { const float4* img[SELECT_MAX]; const float* err[SELECT_MAX]; int n; };
size_t select_lds_bytes(int n, int Rs, int Rb);
void launch_select(float4* dst, unsigned char* index, const SelectDev& S, int W, int H, int Rs, int Rb, int form, hipStream_t st);
// bricks: cells in 4x4x4 bricks (vp_device.h cell_index); the buffer then holds ceil(n/4)^3 * 64 cells
void launch_pack_u8(const unsigned char* vol, uint2* cells, int nx, int ny, int nz, bool bricks, hipStream_t st);
void launch_pack_f32(const float* vol, float* cells, int nx, int ny, int nz, bool bricks, hipStream_t st);
void launch_pack_f16(const unsigned short* vol, uint4* cells, int nx, int ny, int nz, bool bricks, hipStream_t st);   // 8 halves per cell, the order of pack_f32
// lds: uchar volumes through opacity_lds_k (the density grid staged through LDS tile by tile), else opacity_k: the same bits
void launch_opacity(const SceneDev& S, bool quant, bool half, bool lds, const float dir[3], float* out, hipStream_t st);
void launch_build_bounds(const void* d_vol, bool quant, bool half, void* d_out, void* d_tmp_a, void* d_tmp_b, int nx, int ny, int nz, int radius, int brick,
                         hipStream_t st);
// the feature pass (include/volpath.h vp_render_features): a launch works on `n` slots of a pixel list (y << 16 | x) of a width x height
// image and writes alpha / depth at y * width + x.  table: the per-pixel table of that image (vp_get_pixel_table's; two float4 per
// pixel) where the march may skip the certified-empty stretch of a chord, or null
struct FeatureDev
{
    const unsigned* pixels;
    unsigned        n, width, height;
    const float4*   table;
    float           step, tau_z, density, sigma_t[3];
    float4 *        alpha, *depth;
};
// features_k: every slot marches (a ray that misses the box writes the miss constant)
void launch_features(const SceneDev& S, bool quant, bool half, const FeatureDev& F, hipStream_t st);
// features_fill_k: slots [0, n_light) get the result of a march of zeros, the rest the miss constant
void launch_features_fill(const FeatureDev& F, unsigned n_light, hipStream_t st);
void launch_julia(unsigned char* grid, int n, hipStream_t st);
void launch_cloud(float* grid, int n, unsigned seed, hipStream_t st);
void launch_scale(float4* dst, const float4* src, int size, float s, hipStream_t st);
// dst.c = (sun.c * s) * sun_gain[c] + (sky.c * s) * sky_gain[c], dst.w = sun.w * s (relight_k)
void launch_relight(float4* dst, const float4* sun, const float4* sky, float3 sun_gain, float3 sky_gain, int size, float s, hipStream_t st);
// dst = fg * s + (trans * s) o B, dst.w = 1 - trans.w * s; B = plate[i].xyz, or the constant (r, g, b) where plate is null (composite_k)
void launch_composite(float4* dst, const float4* fg, const float4* trans, const float4* plate, float r, float g, float b, int size, float s, hipStream_t st);
// the two in one pass: f.c = (sun.c * s) * sun_gain[c] + (sky.c * s) * sky_gain[c], dst.c = f.c + (trans.c * s) * B.c,
// dst.w = 1 - trans.w * s (relight_composite_k: the bits of relight_k, scale_k and composite_k with s = 1 in sequence)
void launch_relight_composite(float4* dst, const float4* sun, const float4* sky, const float4* trans, float3 sun_gain, float3 sky_gain, const float4* plate,
                              float r, float g, float b, int size, float s, hipStream_t st);
void launch_gamma(float4* dst, const float4* src, int size, float s, float inv_gamma, hipStream_t st);
void launch_accumulate(float4* dst, const float4* src, size_t n, hipStream_t st);
void launch_test_hg(const float* g, const float* r0, const float* r1, const float* nrm, const float* cosq, float* dir, float* ev, int n, hipStream_t st);
void launch_test_box(const SceneDev& S, const float* o, const float* d, int* hit, float* tn, float* tf, int n, hipStream_t st);
void launch_test_env(const SceneDev& S, const float* d, float* out, int n, hipStream_t st);
// vp_test_camera_ray (vp_test_kernels.h test_camera_ray_k): camera_ray() of n pixels (y << 16 | x) as each unit compiles it
void launch_test_camera_ray(const SceneDev& S, unsigned width, unsigned height, const unsigned* pixels, float* dir, int n, hipStream_t st);
void launch_test_camera_ray_fast(const SceneDev& S, unsigned width, unsigned height, const unsigned* pixels, float* dir, int n, hipStream_t st);
void launch_test_math(int which, const float* in, float* out, int n, hipStream_t st);
void launch_test_roots(int which, unsigned lo, unsigned hi, unsigned long long* mismatches, unsigned* first_bad, hipStream_t st);   // (exact arithmetic only)
// the same two hooks compiled in the fast arithmetic (vp_kernels_fast.hip)
void launch_test_hg_fast(const float* g, const float* r0, const float* r1, const float* nrm, const float* cosq, float* dir, float* ev, int n, hipStream_t st);
void launch_test_math_fast(int which, const float* in, float* out, int n, hipStream_t st);
// vp_test_log_forms / vp_test_approach_walk (vp_test_kernels.h), in the exact and in the fast arithmetic
void launch_test_log_forms(int which, unsigned lo, unsigned hi, unsigned long long* mismatches, unsigned* first_bad, hipStream_t st);
void launch_test_log_forms_fast(int which, unsigned lo, unsigned hi, unsigned long long* mismatches, unsigned* first_bad, hipStream_t st);
void launch_test_approach_walk(int kind, int n, const float* par, const unsigned* scr, const unsigned* words, unsigned* out_new, unsigned* out_ref, hipStream_t st);
void launch_test_approach_walk_fast(int kind, int n, const float* par, const unsigned* scr, const unsigned* words, unsigned* out_new, unsigned* out_ref,
                                    hipStream_t st);
// vp_test_sun_start (vp_test_kernels.h test_sun_start_k): sun_dir is a HOST array of three floats, the rest device arrays
void launch_test_sun_start(int n, const float* origin, const float* sun_dir, const float* box, unsigned* out_new, unsigned* out_ref, hipStream_t st);
void launch_test_sun_start_fast(int n, const float* origin, const float* sun_dir, const float* box, unsigned* out_new, unsigned* out_ref, hipStream_t st);
// vp_test_fetch_split (vp_test_kernels.h test_fetch_split_k): device arrays; the exact unit's (the fetch is one code in both)
void launch_test_fetch_split(float linv, int n, int count, const unsigned* s_bits, unsigned* out_two, unsigned* out_fold, hipStream_t st);
void launch_test_rng(int mode, unsigned x, unsigned y, unsigned f, unsigned k0, unsigned k1, int n, float* out, hipStream_t st);
void launch_test_density(const SceneDev& S, bool quant, bool half, const float* pos, float* out, int n, hipStream_t st);
}  // namespace vp
