// vp_render.cpp -- the launch path.  do_render: one render call as a sequence of stages -- the precondition check, the tables the launches
// read, the launch plan (lists, staging, approach walk, pipeline slot), then per launch the staging reserve, the pipeline waits, one
// function per pixel class (approach kernel and render_k, the light kernel or its constants, the box-missing constants) and the
// add-kernel; the render targets' buffers; counters, timing, vp_prepare / vp_reserve_frames
#include "vp_state.h"

namespace vph __attribute__((visibility("hidden")))
{
// The part of a launch's span [a, b] that the launches timed before it did not cover: from max(a, end) to b, where `end` is the latest
// end among them (nullptr: none); `end` moves to b when b is later.  Pipelined calls of vp_render_frames overlap (pipe_target): a launch
// is reported from where its predecessor ended, so the reported times add up to at most the wall time they span.
static float span_ms(hipEvent_t a, hipEvent_t b, hipEvent_t& end)
{
    float ms = 0.0f, since = 0.0f;
    if (hipEventElapsedTime(&ms, a, b) != hipSuccess) { (void)hipGetLastError(); return 0.0f; }
    if (end && hipEventElapsedTime(&since, end, b) == hipSuccess)
    {
        if (since <= 0.0f) return 0.0f;   // inside a span already counted
        ms = std::min(ms, since);
    }
    else (void)hipGetLastError();
    end = b;
    return std::max(ms, 0.0f);
}
// ... folded into a running sum: the pair goes back to the pool, except an event that is now the latest end
static void fold_span(hipEvent_t a, hipEvent_t b, hipEvent_t& end, double& sum)
{
    hipEvent_t e = end;
    if (hipEventQuery(b) == hipSuccess) sum += span_ms(a, b, e);
    else (void)hipGetLastError();   // a launch this old that has not completed is counted without a time rather than waited for
    put_event(a);
    if (e == b) { put_event(end); end = b; }
    else put_event(b);
}
// a pair of events around one kernel of a launch (per-class kernel time, vp_render_class_time_ms); best effort
struct ClassTimer
{
    int cls; hipStream_t st; hipEvent_t a = nullptr, b = nullptr; bool ok = false;
    ClassTimer(int c, hipStream_t s) : cls(c), st(s)
    {
        a = get_event(); b = get_event();
        ok = a && b && hipEventRecord(a, st) == hipSuccess;
        if (!ok) (void)hipGetLastError();
    }
    ~ClassTimer() { put_event(a); put_event(b); }   // a timer that was never stopped (an early return) hands its events back
    void stop()
    {
        if (ok && hipEventRecord(b, st) == hipSuccess) { G.class_events.push_back({cls, a, b}); a = b = nullptr; }
        else (void)hipGetLastError();
        put_event(a); put_event(b); a = b = nullptr;
        while (G.class_events.size() > 3 * kMaxPendingEvents)
        {
            auto ev = G.class_events.front();
            G.class_events.pop_front();
            fold_span(ev.a, ev.b, G.class_last_end[ev.cls], G.class_ms[ev.cls]);
        }
    }
};
// keep at most kMaxPendingEvents launch pairs: fold the oldest into the running sum
void trim_events()
{
    while (G.events.size() > kMaxPendingEvents)
    {
        auto ev = G.events.front();
        G.events.pop_front();
        fold_span(ev.first, ev.second, G.last_end, G.timed_ms);
    }
}

// Waits for the pipelined launches in flight, and has the next one wait for the caller's stream: called wherever what a launch reads
// may change -- la_quiesce (every table, the volume, the environment, buffer growth, the look-ahead), the setters, the counters.
int pipe_quiesce()
{
    G.pipe_fence = true;
    if (!G.pipe_busy) return VP_OK;
    for (hipStream_t st : G.pipe_stream)
        if (st) HIPCHK(hipStreamSynchronize(st));
    G.pipe_busy = false;
    return VP_OK;
}
// ---- render targets (vp_state.h RenderTarget): queue words by index, and the two buffers a launch needs on one
static int       target_index(const RenderTarget* rt) { return (int)(rt - G.target); }
static unsigned* target_queue(const RenderTarget* rt) { return G.d_queue + 2 * kQueueWords * (size_t)target_index(rt); }   // two tile classes each
static bool      is_lookahead(const RenderTarget* rt) { return rt == &G.target[1] || rt == &G.target[2]; }
static const int kPipeTarget[2] = {0, kTargets - 1};   // the render targets of the two pipeline slots
// nothing may read a buffer while it is replaced: the target's stream and, where its buffers are a pipeline slot's, the pipelined launches
static int drain_target(const Target& T)
{
    if (int rc = is_lookahead(T.rt) ? VP_OK : pipe_quiesce()) return rc;
    HIPCHK(hipStreamSynchronize(T.stream));
    return VP_OK;
}
// The staging buffer of T for a launch of `exact` bytes: grown to `want` >= exact or, failing that, to `exact`.  drained: the caller
// has waited for the readers itself.  An allocation that fails is no error here: the buffer is then smaller than `exact`, and what
// follows is the caller's (a smaller launch, no pipeline slot, VP_E_NOMEM).
static int reserve_stage(const Target& T, size_t exact, size_t want, bool drained = false)
{
    if (exact <= T.rt->stage.bytes) return VP_OK;
    if (!drained)
    {
        if (int rc = drain_target(T)) return rc;
        HIPCHK(hipStreamSynchronize(G.stream));  // add-kernels of earlier frames may still read the old buffer
    }
    if (T.rt->stage.grow(want) != hipSuccess && want > exact) (void)T.rt->stage.grow(exact);
    return VP_OK;
}
// The hand-over buffer likewise.  Needed is `exact`, allocated is `want`: a look-ahead slot asks for its largest batch at once (a slot
// that grew with every doubling of the ramp would synchronise its stream -- and the batch running beside it -- at every step), but a
// slot that already holds THIS batch is left alone.  Without the buffer there is no walk ahead of the integrator: same bits.
static int reserve_handover(const Target& T, size_t exact, size_t want, bool drained = false)
{
    if (exact <= T.rt->handover.bytes) return VP_OK;
    if (int rc = drained ? VP_OK : drain_target(T)) return rc;
    (void)T.rt->handover.grow(want);
    return VP_OK;
}
// ---- the pipeline of vp_render_frames calls (vp_state.h)
// Sizes pipeline slot s for a call of nframes frames in ONE launch: its staging buffer and, where the decomposition estimator's walk
// hands over, its approach buffer, each capped as the single target's (stage_frames_cap: VP_STAGE_MB, a quarter of the free memory).
// false: the slot cannot hold the call (the caller's stream then renders it as before, same bits).
static bool pipe_reserve(int s, size_t per_frame, int nframes, bool aux)
{
    const Target T = {&G.target[kPipeTarget[s]], G.stream};
    const size_t need  = per_frame * (size_t)nframes * sizeof(float4);
    const size_t need4 = aux ? per_frame * (size_t)nframes * sizeof(uint2) : 0;
    if (need <= T.rt->stage.bytes && need4 <= T.rt->handover.bytes) return true;
    if (need > T.rt->stage.bytes && stage_frames_cap(per_frame, T.rt->stage.bytes) < (size_t)nframes) return false;
    // (growth: nothing may still read the old buffers -- the slots' launches, the reduces and one-frame launches on the caller's stream)
    if (pipe_quiesce() || hipStreamSynchronize(G.stream) != hipSuccess) { (void)hipGetLastError(); return false; }
    (void)reserve_stage(T, need, need, true);
    if (need > T.rt->stage.bytes) return false;
    (void)reserve_handover(T, need4, need4, true);
    return need4 <= T.rt->handover.bytes;
}
static bool pipe_streams()
{
    for (int s = 0; s < 2; s++)
    {
        if (!G.pipe_stream[s] && create_internal_stream(&G.pipe_stream[s]) != hipSuccess) { (void)hipGetLastError(); G.pipe_stream[s] = nullptr; return false; }
        for (hipEvent_t* e : {&G.pipe_done[s], &G.pipe_free[s], &G.pipe_gate[s], &G.pipe_fence_ev})
            if (!*e && hipEventCreateWithFlags(e, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); *e = nullptr; return false; }
    }
    return true;
}
// The target of a pipelined call: the next slot's stream (created on first use, lowest priority: create_internal_stream) and render
// target.  false: today's single target on the caller's stream.
static bool pipe_target(size_t per_frame, int nframes, bool aux, Target* T)
{
    const int s = G.pipe_next;
    if (!pipe_streams() || !pipe_reserve(s, per_frame, nframes, aux)) return false;
    *T = {&G.target[kPipeTarget[s]], G.pipe_stream[s]};
    return true;
}
// Before a pipelined launch: the slot's stream waits for the reduce that last read its staging (two calls back), for the previous
// call's walk (pipe_gate) and, after a change, for the caller's stream
static int pipe_await_slot_free(int ps, hipStream_t st)
{
    if (G.pipe_free_set[ps]) HIPCHK(hipStreamWaitEvent(st, G.pipe_free[ps], 0));
    if (G.pipe_gate_set[ps ^ 1]) HIPCHK(hipStreamWaitEvent(st, G.pipe_gate[ps ^ 1], 0));
    G.pipe_gate_set[ps] = false;
    if (G.pipe_fence)
    {
        HIPCHK(hipEventRecord(G.pipe_fence_ev, G.stream));
        HIPCHK(hipStreamWaitEvent(st, G.pipe_fence_ev, 0));
        G.pipe_fence = false;
    }
    G.pipe_busy = true;
    return VP_OK;
}
// Before its reduce: the caller-visible write stays on the caller's stream, behind the slot's launch
static int pipe_await_launch(int ps, hipStream_t st)
{
    HIPCHK(hipEventRecord(G.pipe_done[ps], st));
    HIPCHK(hipStreamWaitEvent(G.stream, G.pipe_done[ps], 0));
    return VP_OK;
}
// ---- preconditions
int check_render(unsigned what, const Param* p, long long last_frame)
{
    if (what & CHK_STATE)
    {
        if (!G.have_volume) return fail(VP_E_STATE, "render before init_cuda");
        if (!G.have_env) return fail(VP_E_STATE, "render before init_envmap");
        if (!G.have_sun) return fail(VP_E_STATE, "render before set_sun");
        if (!G.have_cam) return fail(VP_E_STATE, "render before copy_inv_view_matrix");
    }
    if ((what & CHK_IMAGE) && (p->width == 0 || p->height == 0 || p->width > 65535 || p->height > 65535))
        return fail(VP_E_ARG, (what & CHK_IMAGE_NOTE) ? "image %ux%u out of range (sampler.h packs x<<16|y)" : "image %ux%u out of range", p->width, p->height);
    if (what & CHK_MODES)
    {
        if (G.trk && G.env_mis) return fail(VP_E_STATE, "scalar tracking builds exist with passive environment lighting only");
        if (G.trk && G.count) return fail(VP_E_STATE, "work counters are not built for the scalar tracking kernels");
        if (G.rng == VP_RNG_PHILOX7 && (G.trk || G.env_mis))
            return fail(VP_E_STATE, "VP_RNG_PHILOX7 is built for spectral tracking with passive environment lighting only");
        if (G.arith == VP_ARITH_FAST)
        {
            // the fast arithmetic is built for the counter-based streams' shipped configuration only (vp_kernels_fast.hip)
            if (G.rng == VP_RNG_SAMPLERH) return fail(VP_E_STATE, "VP_ARITH_FAST is not built for VP_RNG_SAMPLERH (the parity mode is exact by definition)");
            if (G.est == VP_EST_BOUNDED) return fail(VP_E_STATE, "VP_ARITH_FAST is not built for VP_EST_BOUNDED");
            if (G.env_mis) return fail(VP_E_STATE, "VP_ARITH_FAST is built for passive environment lighting only");
            if (G.trk) return fail(VP_E_STATE, "VP_ARITH_FAST is built for spectral tracking only");
            if (G.count) return fail(VP_E_STATE, "work counters are not built for VP_ARITH_FAST");
        }
        if (int rc = subpixel_check(p)) return rc;
    }
    if ((what & CHK_OPACITY) && G.est == VP_EST_DECOMP && last_frame > 10 && !G.S.opacity)
        return fail(VP_E_NOOPACITY, "frames beyond 10 need precompute_opacity (kernel.cu:2183, host.cpp:336-343)");
    return VP_OK;
}
// the camera rays' walk ahead of the integrator is built for this estimator and configuration (whatever the lists: vp_reserve_frames)
static bool approach_built()
{
    const bool dense_volume = G.marked_fraction > G.dense_fraction;   // (vp_state.h: little empty space for the walk to cross)
    // (a sub-pixel factor: the integrator walks the camera ray itself -- the approach kernels and the segment table are statements about
    // ONE camera ray per pixel, and with S^2 of them a wave of one pixel x 64 frames no longer shares a ray: DESIGN.md section 2.2)
    return G.use_approach && !G.sub_shift && (G.est == VP_EST_GLOBAL || (G.est == VP_EST_DECOMP && G.use_approach_local && !dense_volume)) && !G.trk && !G.env_mis;
}
// ... and has a table and pixels to walk for (do_render; counting launches aside)
static bool approach_possible(const float4* crawl, unsigned n_general) { return approach_built() && crawl && n_general; }
// ---- the plan of a call: what every launch of it has in common
struct LaunchPlan
{
    Target     T;                 // where its launches run: the caller's stream, the look-ahead slot handed in, or a pipeline slot
    bool       lookahead;         // ... a look-ahead batch (cancellable, never one of the caller's timed launches)
    bool       stage_only;        // ... which is staged whole and not reduced
    PlaneSet   PS;                // what the call accumulates into (vp_kernels.h): its mode, accumulators, records and criterion; PS.acc[0] is d_out
    size_t stage_planes() const { return PS.groups() ? 2u : 1u; }   // staging planes per frame: a groups mode stages the sky's samples in a second
                                                                    // (NOT the call's planes: halves double the accumulators and stage what the mode stages)
    bool plain() const { return PS.mode == PLANES_ONE && !PS.stats(); }   // vp_render_frames' own call: one plane, no records (a halves call
                                                                          // is not: staged for one frame too, never pipelined)
    // the slots of the list, general pixels first: where the class a kernel integrates ends (the general class and a light class that
    // is not written as constants), i.e. where the per-pixel constants of a launch begin -- const_from and the layers reduce's range
    unsigned integrated_end() const { return PL.n_general + ((PL.n_light && !light_const) ? PL.n_light : 0u); }
    PixelLists PL;                // the lists in use: the context's cached ones, or the caller's
    const float4* ray;            // the ray table of the general class (global majorant, the cached lists), or null
    size_t     per_frame;         // ... and their pixels = samples per frame
    bool       staged;            // samples go through the staging buffer and a reduce (false: render_k accumulates one frame directly)
    bool       light_const;       // the light class is written by miss_fill_k
    bool       approach, approach_thr, appr_aux_needed;   // a walk ahead of the integrator; with the throughput table; with a hand-over buffer
    bool       piped; int slot;   // on pipeline slot `slot`
    size_t     max_f;             // frames per launch
    bool both() const { return PL.n_light && PL.n_general && !light_const; }   // the general and the light KERNEL have work
    // frames to size a buffer for when a launch of f needs it: a look-ahead slot's for the largest batch at once (reserve_handover)
    size_t sized_frames(int f) const { return std::min<size_t>(stage_only ? std::max<size_t>((size_t)f, (size_t)std::max(G.la_max, 1)) : (size_t)f, max_f); }
};
// The tables the launches read, into L, and what they decide, into A: in this order (some synchronise or quiesce).  A.per_frame == 0: nothing to render
static int prepare_tables(const Param* p, const Shard& sh, int nframes, const PixelLists* lists, LaunchDev& L, LaunchPlan& A)
{
    int rc = VP_OK;
    // (a sub-pixel factor: the per-pixel table of the image the samples are computed on; lists, staging and output stay this image's)
    L.sub_shift = (unsigned)G.sub_shift;
    const Param fine = subpixel_param(p);
    if ((rc = ensure_crawl_table(&fine, &L.crawl))) return rc;
    if ((rc = ensure_pixel_lists(p, L.crawl, sh))) return rc;
    // the lists this call launches on: the context's cached ones, or the caller's (vp_adaptive.cpp: the active pixels of a round --
    // a class-ordered subset of the cached lists; staging rows, sample queues and the reduce are then that subset's)
    const PixelLists& PL = A.PL = lists ? *lists : PixelLists{G.d_tiles, G.n_general, G.n_light, G.n_miss};
    A.per_frame = (size_t)PL.n_general + PL.n_light + PL.n_miss;
    if (A.per_frame == 0) return VP_OK;
    // (global majorant: the general pixels' camera rays and box tests, tabulated per view in the order of the cached lists -- a caller's
    // own lists are a subset of them in another order and go without)
    A.ray = nullptr;
    if (!lists && (rc = ensure_ray_table(p, L.crawl, &A.ray))) return rc;
    G.last_ray_table = 0;
    if ((rc = ensure_sun_clip(&L.sun_clip, &L.clip_ds))) return rc;
    L.count_clips = getenv("VP_DEBUG_COUNT_CLIPS") ? 1u : 0u;
    if ((rc = exit_flights(L))) return rc;
    A.light_const = false;
    if (PL.n_light && (rc = ensure_light_const(p, &A.light_const))) return rc;
    G.last_light_const = A.light_const ? 1 : 0;
    if (G.est == VP_EST_GLOBAL && PL.n_light && !A.light_const)
    {
        if ((rc = ensure_thr_table(p, &L.thr_table))) return rc;
        L.thr_n = G.thr_entries;
    }
    // the camera rays' free flights through certified-empty cells in kernels of their own, ahead of the integrator (approach_k: global
    // majorant; approach_local_k: decomposition estimator; spectral tracking, passive environment, staged launches)
    A.approach = A.approach_thr = false;
    if (approach_possible(L.crawl, PL.n_general) && (!G.count || getenv("VP_COUNT_APPROACH")))   // counting launches: the integrator makes every step itself unless asked (block tallies)
    {
        // global majorant: one majorant for the whole walk, checked here; decomposition: approach_local_k checks each segment's own
        bool identity = true;
        if (G.est == VP_EST_GLOBAL) rc = G.arith == VP_ARITH_FAST ? ensure_fast_identity(p, &identity) : ensure_light_identity(p, &identity);
        if (rc) return rc;
        // (fast arithmetic: only where its own null collision in empty space is neutral -- else render_k walks, as in a one-frame launch)
        A.approach = identity || G.arith != VP_ARITH_FAST;
        if (!identity && A.approach)
        {
            // the walk's null collisions change the throughput: render_k looks it up by their number (the light kernel's table)
            if ((rc = ensure_thr_table(p, &L.thr_table))) return rc;
            L.thr_n  = G.thr_entries;
            A.approach_thr = true;
        }
    }
    // (decomposition estimator: the restart segments of every general pixel's camera ray, tabulated once per view -- built with the
    // crawl table and the pixel lists whatever the frame count, so that no later launch rebuilds it and waits for those in flight;
    // read by waves of one pixel x 64 frames)
    L.seg_table = nullptr;
    if (A.approach && G.est == VP_EST_DECOMP && G.approach_fshift_max >= 6 && !lists)
    {
        const float4* seg = nullptr;
        if ((rc = ensure_segment_table(p, L.crawl, &seg))) return rc;
        if (nframes >= 64) L.seg_table = seg;
    }
    return VP_OK;
}
// Where the call runs and how it is cut into launches: staging, the hand-over buffer, the pipeline slot
static int plan_target(int nframes, const Target* tgt, const PixelLists* lists, LaunchPlan& A)
{
    // a call with statistics is staged whatever its length (render_k's direct accumulation has none) and stays on the caller's stream
    // (a layers call too: the direct accumulation has no second target)
    A.staged = nframes > 1 || A.stage_only || !A.plain();
    A.T      = tgt ? *tgt : Target{&G.target[0], G.stream};   // (a pipelined call: a slot's, below)
    A.max_f  = A.staged ? stage_frames_cap(A.per_frame, A.T.rt->stage.bytes, A.stage_planes()) : 1;
    // The staging slot of the decomposition estimator's hand-over holds the segment origin and the distance reached in it: the stream's
    // state (a pair index, or sampler.h's two words) goes beside it.  Sized ONCE, before the launch loop (no synchronisation, no early
    // return between a launch's events).
    A.appr_aux_needed = A.approach && G.est == VP_EST_DECOMP && A.staged;
    // A staged call of vp_render_frames goes to the next pipeline slot when the slot holds it in one launch (counting launches stay on the
    // caller's stream).  Otherwise -- VP_NO_PIPELINE, no memory for the slot -- the caller's stream, as before: same bits either way.
    A.slot  = G.pipe_next;
    A.piped = !tgt && !A.stage_only && !lists && A.plain() && nframes > 1 && G.pipeline && !G.count && pipe_target(A.per_frame, nframes, A.appr_aux_needed, &A.T);
    if (A.piped) A.max_f = (size_t)nframes;
    else if (!tgt) G.pipe_fence = true;   // (the caller's stream uses slot 0's buffers: the next pipelined launch waits for it)
    G.last_pipelined = A.piped ? 1 : 0;
    if (!A.appr_aux_needed) return VP_OK;
    const size_t one = A.per_frame * sizeof(uint2);
    return reserve_handover(A.T, one * std::min<size_t>((size_t)nframes, A.max_f), one * A.sized_frames(nframes));
}
// The staging of a launch of f frames.  *smaller: another allocator took the memory since it was measured -- A.max_f is halved, and a
// smaller batch renders the same bits
static int reserve_launch_stage(LaunchPlan& A, int f, bool* smaller)
{
    *smaller = false;
    const size_t exact = A.per_frame * (size_t)f * sizeof(float4) * A.stage_planes();
    const int rc = reserve_stage(A.T, exact, A.per_frame * A.sized_frames(f) * sizeof(float4) * A.stage_planes());
    if (rc || exact <= A.T.rt->stage.bytes) return rc;
    if (A.stage_only) return fail(VP_E_NOMEM, "no memory for a look-ahead batch of %d frames", f);
    if (f <= 1) return fail(VP_E_NOMEM, "no memory for one staged frame (%zu bytes)", exact);
    A.max_f = (size_t)std::max(f / 2, 1);
    *smaller = true;
    return VP_OK;
}

// ---- one launch
// The form the brick table takes in the general class's kernel: 0 global memory, 1 16-bit pairs through LDS, 2 2-bit codes through LDS
static int brick_table_form(const LaunchPlan& A, const Param* p, const SceneDev& S)
{
    // the brick table goes through LDS when it fits (decomposition estimator, byte table <= 64 KiB)
    const bool lds_bounds = G.use_lds_bounds && G.est == VP_EST_DECOMP && G.quant && !G.env_mis && !G.trk &&
                            (size_t)S.bnx * S.bny * S.bnz <= (size_t)VP_LDS_BOUND_ENTRIES;
    // ... as 2-bit codes where it has at most four distinct pairs (round 5): the plain kernel's registers and occupancy with the table
    // in LDS.  Timed launches of the counter-based streams; counting launches and look-ahead batches keep the 16-bit form.
    // Chromatic media too, since their kernel fits six waves per SIMD (79 registers: intersect_box axis by axis, vp_device.h): c4s
    // 1935 with the 16-bit table and its helper, 2001 from global memory, 2024 with the codes (profiles/experiments/r05_box_sequence.txt;
    // before that change 1.7 % behind the 16-bit table: r05_lds_compact_table.txt).  VP_LDS_COMPACT_CHROMATIC=0: not.
    // A table that cannot go as codes: for those launches from GLOBAL memory (six / five waves) rather than as 16-bit pairs through LDS
    // (four waves and a helper workgroup) -- c4f +1.6 %; C3 was level already (round 5).  VP_LDS_PAIRS=1: the pairs.
    const bool ach_lds = p->sigma_t.x == p->sigma_t.y && p->sigma_t.y == p->sigma_t.z && p->albedo.x == p->albedo.y && p->albedo.y == p->albedo.z;
    // (the sequential sampler.h stream has no codes kernel; its timed launches, too, are ahead without the pairs: c3 +2.2 %, c4s +4.3 %)
    const bool timed_l  = !G.count && !A.lookahead;                // a timed launch (not a counting one, not a look-ahead batch)
    const bool timed_cb = timed_l && G.rng != VP_RNG_SAMPLERH;    // ... of a counter-based stream
    return !lds_bounds ? 0 : (G.bound_codes_ok && G.d_bound_codes && timed_cb && (ach_lds || G.lds_compact_chromatic)) ? 2
                             : (timed_l && !G.lds_pairs) ? 0 : 1;
}
// ... and whether the 16-bit form gets its helper workgroups (launch_general_class) on the auxiliary stream
// (not for look-ahead batches: two of them overlap -- the next one's approach walk and first workgroups run beside the current
// one's body and tail -- only if the current one leaves registers free: four LDS-table waves per SIMD do, the helper's fifth does
// not.  C3 host loop 1301 -> 1510 Msamples/s without it, profiles/r03_render_kernel_lookahead.txt)
// COUPLING (two tuning decisions that depend on each other): approach_local_k needs 47 vector registers (kernel_resources.py);
// beside four 97-102-register LDS-table waves AND the helper's fifth 96-register wave a SIMD has 27 left, beside the four
// alone 124.  If approach_local_k's register count or the helper's occupancy changes, re-measure the `!A.lookahead` below.
static bool brick_table_helper(const LaunchPlan& A, int lds_form) { return lds_form == 1 && G.lds_helper && A.PL.n_general && !(A.PL.n_light && !A.light_const) && !A.lookahead; }
// The grid of a class's kernel (cls 0 the general, 1 the light one) over total_items samples: workgroups, the most that are resident,
// and how long a wave stays in the tracking loop
struct ClassGrid { bool ldsb; unsigned blocks, cap, wait_iters; };
static ClassGrid class_grid(const LaunchPlan& A, int cls, int lds_form, unsigned total_items)
{
    ClassGrid g;
    g.ldsb = lds_form == 1 && !cls;   // (the 16-bit table: 512-thread workgroups, two per CU)
    const unsigned bsz  = g.ldsb ? VP_BLOCK_LDS : VP_BLOCK;
    unsigned waves  = (total_items + 63) / 64;
    g.blocks = (waves + (bsz / 64) - 1) / (bsz / 64);
    const bool     both = A.both();
    unsigned       bpc  = G.blocks_per_cu;
    // what fits a SIMD's 512 vector registers side by side: global majorant 4 x 96 + 2 x 64,
    // local majorant 5 x 96 + ... the light kernel's blocks take what is left as general blocks retire
    // (local majorant, five 96-register general waves per SIMD: the light kernel's workgroups find room as general ones retire,
    // i.e. mostly at the end -- then as many of them as fit)
    if (both && cls) bpc = G.light_blocks_per_cu ? G.light_blocks_per_cu : (G.est == VP_EST_GLOBAL ? 2u : 6u);
    if (!both && cls) bpc = 8u;   // the light kernel alone: 64 registers
    if (both && !cls) bpc = G.general_blocks_per_cu ? G.general_blocks_per_cu : (G.est == VP_EST_GLOBAL ? 4u : 5u);
    // look-ahead batches overlap in pairs: the next batch's approach walk (23 / 47 registers) must find room beside the current
    // batch's integrator -- six of its 72-register workgroups leave 80 registers per SIMD lane, five 80-register ones 112
    if (A.lookahead && !cls && !both) bpc = std::min(bpc, G.est == VP_EST_GLOBAL ? 6u : 5u);
    g.cap = (unsigned)G.num_cu * (g.ldsb ? 2u : bpc);
    if (g.blocks > g.cap) g.blocks = g.cap;
    // the light kernel's paths are long and end rarely: its waves leave the tracking loop for the (refill / environment /
    // write) pass less often than the general kernel's do for their collisions
    g.wait_iters = cls ? (G.light_wait_iters ? G.light_wait_iters : (G.est == VP_EST_GLOBAL ? 128u : 64u)) : G.wait_iters;
    return g;
}
// A target's auxiliary stream beside its own for one kernel of a launch -- the light kernel beside the general one, or the helper
// workgroups of the LDS-table kernel: forked from everything queued on the target's stream so far, joined before the stream goes on.
// Stream and events are created on first use.  Best effort: whatever fails, the work goes to the target's stream or is left out.
struct AuxBranch
{
    RenderTarget& rt; hipStream_t main; bool forked = false;
    static bool make(hipEvent_t& e) { if (!e && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); e = nullptr; } return e != nullptr; }
    // the fork point: the auxiliary stream will start behind what is on the target's stream now
    void fork() { if (!(forked = make(rt.aux_ev[0]) && hipEventRecord(rt.aux_ev[0], main) == hipSuccess)) (void)hipGetLastError(); }
    // the auxiliary stream, waiting at the fork point; null: not this time (it is used only if both the record and the wait succeeded:
    // waiting on an unrecorded event returns at once)
    hipStream_t begin()
    {
        if (!rt.aux_stream && create_internal_stream(&rt.aux_stream) != hipSuccess) { (void)hipGetLastError(); rt.aux_stream = nullptr; }
        if (!make(rt.aux_ev[1]) || !rt.aux_stream || !forked) return nullptr;
        if (hipStreamWaitEvent(rt.aux_stream, rt.aux_ev[0], 0) == hipSuccess) return rt.aux_stream;
        (void)hipGetLastError();
        return nullptr;
    }
    // the target's stream goes on (end-of-launch event, add-kernel) only when the auxiliary stream's kernel is done too
    hipError_t join() { return hipEventRecord(rt.aux_ev[1], rt.aux_stream) != hipSuccess || hipStreamWaitEvent(main, rt.aux_ev[1], 0) != hipSuccess ? hipGetLastError() : hipSuccess; }
};
// the integrator and the walk ahead of it in the call's arithmetic: chosen once (vp_kernels_fast.hip)
struct Kernels { decltype(&launch_render) render; decltype(&launch_approach) approach; };
// what the class functions of a launch share
struct Launch { const LaunchPlan& A; const SceneDev& S; LaunchDev& L; int f; int lds_form; bool lds_helper; Kernels k; AuxBranch aux; };
// the part of L that names a class's pixels, slots and sample queues
static void select_class(const LaunchPlan& A, LaunchDev& L, int cls, int f)
{
    const unsigned nt = cls ? A.PL.n_light : A.PL.n_general;
    L.pixels      = A.PL.pixels + (cls ? A.PL.n_general : 0);
    L.ray         = cls ? nullptr : A.ray;   // (sliced like `pixels`: the table holds the general class, which comes first)
    L.nslots      = nt;
    L.slot_base   = cls ? A.PL.n_general : 0u;
    L.total_items = (unsigned)((size_t)nt * (size_t)f);
    L.queue       = target_queue(A.T.rt) + (cls ? kQueueWords : 0);
    // chunks of pixels x frames (general class): only when the frame count is a multiple of the frame block
    L.chunk_fshift = (!cls && G.chunk_fshift && f % (1 << G.chunk_fshift) == 0) ? G.chunk_fshift : 0u;
    // the pixels of the class split into VP_NQUEUES bands (whole 64-pixel groups, the last band takes the rest)
    for (unsigned q = 0; q <= VP_NQUEUES; q++) L.q_start[q] = q == VP_NQUEUES ? nt : (unsigned)((unsigned long long)(nt / 64u) * q / VP_NQUEUES) * 64u;
}
// The general class: the approach walk, the mark the next pipelined call starts behind, the integrator, the LDS-table kernel's helper
static hipError_t launch_general_class(Launch& X, const ClassGrid& g)
{
    const LaunchPlan& A = X.A; LaunchDev& L = X.L; const Target& T = A.T;
    hipError_t le = hipSuccess;
    ClassTimer ct(0, T.stream);
    L.approach = 0;
    G.last_approach = 0;
    G.last_approach_table = 0;
    const bool aux_ok = !A.appr_aux_needed || T.rt->handover.p != nullptr;
    if (A.appr_aux_needed) L.approach_aux = T.rt->handover;
    if (A.approach && aux_ok && L.stage && X.f <= 65535)
    {
        L.approach       = A.approach_thr ? 2u : 1u;
        L.approach_steps = G.approach_steps;
        L.approach_fshift = 0;
        while (L.approach_fshift < G.approach_fshift_max && (2u << L.approach_fshift) <= (unsigned)X.f) L.approach_fshift++;
        X.k.approach(X.S, L, G.est, G.rng, G.quant, T.stream);
        le = hipGetLastError();
        G.last_approach = (int)L.approach;
        G.last_approach_table = (G.est == VP_EST_DECOMP && G.quant && L.seg_table && L.approach_fshift == 6u) ? 1 : 0;
        // the helper workgroups of the LDS-table kernel (auxiliary stream, below) read the staging slots as well: their
        // fork point moves behind the walk
        if (X.lds_helper && X.aux.forked && le == hipSuccess) X.aux.fork();
    }
    // (a pipelined call: the next one starts from here -- its approach walk finds room only as this render_k's waves retire,
    // i.e. in its tail; without the mark it started beside this call's own walk and the two integrators shared the chip)
    if (A.piped && le == hipSuccess)
    {
        if (hipEventRecord(G.pipe_gate[A.slot], T.stream) == hipSuccess) G.pipe_gate_set[A.slot] = true;
        else le = hipGetLastError();
    }
    if (le == hipSuccess)
    {
        X.k.render(X.S, L, G.est, G.rng, G.quant, G.half(), G.count, X.lds_form, G.env_mis, G.trk, (int)g.blocks, T.stream);
        le = hipGetLastError();
        G.last_ray_table = L.ray ? 1 : 0;
    }
    // The LDS-table kernel holds 2 x 64 KiB of a CU's LDS with 2 x 512 threads: four waves per SIMD, where the
    // registers would allow five.  The fifth comes from the SAME kernel without the LDS stage (the brick table read
    // from global memory), one 256-thread workgroup per CU beside it on the auxiliary stream, drawing from the same
    // sample queues: a sample is computed by whichever wave takes its chunk, with the same bits.
    if (X.lds_helper && g.ldsb && le == hipSuccess && X.aux.forked && g.blocks >= g.cap)
        if (hipStream_t hs = X.aux.begin())
        {
            X.k.render(X.S, L, G.est, G.rng, G.quant, G.half(), G.count, 0, G.env_mis, G.trk, G.num_cu, hs);
            le = hipGetLastError();
            if (le == hipSuccess) le = X.aux.join();
        }
    ct.stop();
    return le;
}
// The light class: one constant per pixel where its samples do not depend on the draws in this medium (written for every frame: the
// environment along the camera ray, as for the box-missing pixels), else the light kernel -- beside the general one on the target's
// auxiliary stream when both classes have work
static hipError_t launch_light_class(Launch& X, const ClassGrid& g)
{
    const LaunchPlan& A = X.A; const Target& T = A.T;
    hipStream_t ls = nullptr;
    if (!A.light_const && A.both() && G.light_overlap) ls = X.aux.begin();   // (behind the fork point: queue heads zeroed, the previous launch's reduce, uploads)
    ClassTimer ct(1, ls ? ls : T.stream);
    if (A.light_const) launch_miss_fill(X.S, X.L, false, T.stream);
    else launch_render_light(X.S, X.L, G.est, G.rng, G.quant, G.count, (int)g.blocks, ls ? ls : T.stream);
    hipError_t le = hipGetLastError();
    ct.stop();
    if (ls && le == hipSuccess) le = X.aux.join();
    return le;
}
// the pixels whose camera ray misses the box: one constant per pixel, written for every frame (miss_fill_k)
static hipError_t launch_miss_class(Launch& X)
{
    const PixelLists& PL = X.A.PL;
    X.L.pixels      = PL.pixels + PL.n_general + PL.n_light;
    X.L.nslots      = PL.n_miss;
    X.L.slot_base   = PL.n_general + PL.n_light;
    X.L.total_items = 0;
    ClassTimer ct(2, X.A.T.stream);
    launch_miss_fill(X.S, X.L, G.est != VP_EST_GLOBAL, X.A.T.stream);
    const hipError_t le = hipGetLastError();
    ct.stop();
    return le;
}
// One launch of f frames on the plan's target, between the two events of its time: queue heads, one kernel per pixel class
static int launch_classes(const LaunchPlan& A, const SceneDev& S, LaunchDev& L, const Param* p, int f)
{
    const Target& T = A.T;
    HIPCHK(hipMemsetAsync(target_queue(T.rt), 0, 2 * kQueueWords * sizeof(unsigned), T.stream));
    const int lds_form = brick_table_form(A, p, S);
    G.last_lds_form = lds_form;
    L.bound_codes = lds_form == 2 ? G.d_bound_codes : nullptr;
    L.bound_pal[0] = G.bound_pal[0]; L.bound_pal[1] = G.bound_pal[1];
    hipEvent_t e0 = get_event(), e1 = get_event();
    bool timed = e0 && e1 && hipEventRecord(e0, T.stream) == hipSuccess;
    hipError_t le = hipSuccess;
    Launch X = {A, S, L, f, lds_form, brick_table_helper(A, lds_form),
                G.arith == VP_ARITH_FAST ? Kernels{launch_render_fast, launch_approach_fast} : Kernels{launch_render, launch_approach},
                AuxBranch{*T.rt, T.stream}};
    // the fork point of the light kernel's auxiliary stream: BEFORE the general kernel is queued (the two run side by side),
    // after the queue heads are zeroed
    // (the same fork serves the helper workgroups of the LDS-table kernel when no light kernel needs the stream)
    if ((A.both() && G.light_overlap) || X.lds_helper) X.aux.fork();
    // one launch per pixel class: the general pixels, then the light ones (their own kernel, their own sample queues)
    for (int cls = 0; cls < 2 && le == hipSuccess; cls++)
    {
        if (!(cls ? A.PL.n_light : A.PL.n_general)) continue;
        if (G.debug_only_class >= 0 && G.debug_only_class != cls) continue;  // VP_DEBUG_ONLY_CLASS: block tallies of one kernel
        select_class(A, L, cls, f);
        const ClassGrid g = class_grid(A, cls, lds_form, L.total_items);
        L.wait_iters = g.wait_iters;
        le = cls ? launch_light_class(X, g) : launch_general_class(X, g);
    }
    if (A.PL.n_miss && le == hipSuccess) le = launch_miss_class(X);
    timed = timed && le == hipSuccess && hipEventRecord(e1, T.stream) == hipSuccess;
    G.timed_n++;
    if (timed) { G.events.emplace_back(e0, e1); trim_events(); }
    else { put_event(e0); put_event(e1); }
    if (le != hipSuccess) return fail(VP_E_NODEVICE, "render launch -> %s", hipGetErrorString(le));
    return VP_OK;
}
// The reduce of a staged launch into the caller's image, on the caller's stream (last: the call's last launch)
static int reduce_launch(const LaunchPlan& A, LaunchDev& L, bool last)
{
    // for the add-kernel: all tiles of the rank
    L.pixels = A.PL.pixels; L.nslots = (unsigned)A.per_frame; L.slot_base = 0;
    if (!L.stage || A.stage_only) return VP_OK;
    if (A.piped)
        if (int rc = pipe_await_launch(A.slot, A.T.stream)) return rc;
    // (an adaptive round that the staging cap splits into several launches: the criterion is the ROUND's, evaluated in its last launch;
    // the unmarked range of a layers mode is the light KERNEL's slots of the list in use, the caller's included)
    launch_reduce_planes(L, A.PS, A.PL.n_general, A.integrated_end(), last, G.stream);
    HIPCHK(hipGetLastError());
    if (A.piped)
    {
        HIPCHK(hipEventRecord(G.pipe_free[A.slot], G.stream));   // (the slot is free again once this reduce has read its staging)
        G.pipe_free_set[A.slot] = true;
    }
    return VP_OK;
}

// One render call: check, prepare the tables, plan, then launch by launch -- reserve the staging, wire the pipeline, launch the
// classes (timed), reduce
int do_render(vp_float4* d_out, int first, int nframes, const Param* p, bool stage_only, const Target* tgt, const PixelLists* lists, const PlaneSet* planes)
{
    int rc = ensure_device();
    if (rc) return rc;
    if ((rc = check_render(CHK_STATE, p))) return rc;
    if (!d_out || !p || nframes <= 0 || first < 0) return fail(VP_E_ARG, "bad render arguments");
    if ((rc = check_render(CHK_IMAGE | CHK_IMAGE_NOTE | CHK_MODES, p))) return rc;
    G.last_arith = G.arith;   // (vp_last_arithmetic: the mode of the last render call, whatever classes its pixels fall in)
    if ((rc = check_render(CHK_OPACITY, p, (long long)first + nframes - 1))) return rc;
    LaunchDev L = {};
    static_assert(sizeof(ParamDev) == sizeof(Param) && sizeof(Param) == 44, "Param layout (param.h:4-12)");
    memcpy(&L.P, p, sizeof(Param));
    const Shard sh = shard_of(p);
    L.out = (float4*)d_out;
    L.counters = G.count ? G.d_counters : nullptr;
    L.key0 = G.key0; L.key1 = G.key1;
    L.wait_lanes = G.wait_lanes; L.wait_iters = G.wait_iters; L.setup_lanes = G.setup_lanes; L.end_lanes = G.end_lanes;
    // (Rounds 4-5 gave the chromatic local-majorant kernels 32 parked lanes: their event pass was the most expensive.  Since the event
    // section reads its uniforms from LDS -- vp_kernels.hip kargs_lds_ -- a visit is cheap enough that the general default is the
    // better one there too: c4s +1.1 %, c4f +0.9 % at 28, profiles/experiments/r05_kargs_lds.txt.  Performance only.)
    // the sequential sampler.h stream (the parity mode): its shadow rays walk to their ends, a wave's lanes park later -- 24 lanes, the
    // default of rounds 1-4, stays 0.8 % ahead of 28 on the reference's live configuration (profiles/r05_raw/sweep_samplerh.txt)
    if (!G.wait_lanes_set && G.rng == VP_RNG_SAMPLERH && G.trk == VP_TRACK_SPECTRAL) L.wait_lanes = 24;
    if (sh.per_frame == 0) return VP_OK;
    if ((lists || planes) && (tgt || stage_only)) return fail(VP_E_ARG, "look-ahead batches render the cached lists without statistics, layers or groups");
    LaunchPlan A = {};
    A.lookahead = tgt != nullptr; A.stage_only = stage_only;
    if (planes) A.PS = *planes;
    A.PS.acc[0] = L.out;
    L.layers = A.PS.layers() ? 1u : 0u;
    if ((rc = prepare_tables(p, sh, nframes, lists, L, A)) || A.per_frame == 0) return rc;
    if (0xfffffff0u / A.per_frame < 1) return fail(VP_E_ARG, "image too large for the 32-bit sample queue");
    L.stage_stride = (unsigned)A.per_frame;
    SceneDev S = G.S;
    S.linear   = G.linear ? 1 : 0;
    if ((rc = plan_target(nframes, tgt, lists, A))) return rc;
    // look-ahead batches carry their slot's cancel word and their number (la_render_slot, la_quiesce); the caller's own launches cannot be cancelled
    L.cancel = tgt ? G.d_cancel + target_index(A.T.rt) : nullptr; L.batch_id = A.T.rt->batch_seq;
    for (int done = 0; done < nframes;)
    {
        const int f = (int)std::min<size_t>((size_t)(nframes - done), A.max_f);
        if (stage_only && f != nframes) return fail(VP_E_ARG, "look-ahead batch does not fit the staging buffer");
        bool smaller = false;
        if (A.staged && (rc = reserve_launch_stage(A, f, &smaller))) return rc;
        if (smaller) continue;
        L.frame0 = first + done;
        L.nframes = f;
        L.stage = A.staged ? A.T.rt->stage.p : nullptr;
        L.groups = A.PS.groups() ? L.stage + A.per_frame * (size_t)f : nullptr;   // (the second plane: behind the f frames of the first)
        // per-pixel constants of the launch (the box-missing pixels; the light class where it is written by miss_fill_k) are staged once,
        // in the launch's first row: the slots behind the general (and an integrated light) class
        L.const_from = 0xffffffffu; L.stage_const = nullptr;
        if (L.stage && G.use_const_rows && !G.sub_shift)   // (a sub-pixel factor: constants of the FINE pixel, staged per frame by subpixel_fill_k)
        {
            L.const_from  = A.integrated_end();
            L.stage_const = L.stage;
        }
        G.last_const_from = L.const_from;
        if (A.piped && (rc = pipe_await_slot_free(A.slot, A.T.stream))) return rc;
        if ((rc = launch_classes(A, S, L, p, f))) return rc;
        if ((rc = reduce_launch(A, L, done + f == nframes))) return rc;
        done += f;
    }
    if (A.piped) G.pipe_next = A.slot ^ 1;
    return VP_OK;
}
// what the counters and the timers read is complete: the pipelined launches, the caller's stream and, for the timers, the look-ahead batches
// still in flight (launches too) and the auxiliary streams (class timers)
static int await_launches(bool lookahead, bool aux)
{
    int rc = ensure_device();
    if (rc) return rc;
    if ((rc = pipe_quiesce())) return rc;
    HIPCHK(hipStreamSynchronize(G.stream));
    for (auto& sl : G.la)
        if (lookahead && sl.stream) HIPCHK(hipStreamSynchronize(sl.stream));
    for (RenderTarget& t : G.target)
        if (aux && t.aux_stream) HIPCHK(hipStreamSynchronize(t.aux_stream));
    return VP_OK;
}

// Calls with planes (include/volpath.h; vp_kernels.h PLANES_*): the call's samples are vp_render_frames' -- same plan, lists, tables,
// walks and kernels, render_k in the instance of the mode --, staged on the caller's stream whatever the frame count, and the reduce
// splits each staged sample into the planes' samples (launch_reduce_planes).
// Layers: LaunchDev::layers set; the reduce splits the samples into the foreground and the transmittance accumulator.
// Light groups: the environment's term of every sample is kept apart -- render_k's GRP instances and the groups forms of the constant
// writers stage it in a second plane (LaunchDev::groups).
// Group layers: both switches at once -- the constant writers of a layers call, two staging planes, three accumulators.
// Any of them with statistics (the _stats calls): the same launches, and the reduce also folds each plane's samples into that plane's records.
// What a mode is not built for is refused before anything is launched (and before the device is asked for).
static const char kLayersMis[] = "scattered paths never see the sky", kGroupsMis[] = "the environment is sampled as a light, another estimator";
// the state a plane call is built for, checked before the device is asked for; fn: the entry point the message names
int plane_state_check(const char* fn, bool groups)
{
    if (G.env_mis) return fail(VP_E_STATE, "%s is defined for passive environment lighting only (VP_ENV_MIS: %s)", fn, groups ? kGroupsMis : kLayersMis);
    if (G.trk) return fail(VP_E_STATE, "%s is built for spectral tracking only", fn);
    if (G.count) return fail(VP_E_STATE, "%s is not built for work counters", fn);
    if (G.arith == VP_ARITH_FAST) return fail(VP_E_STATE, "%s is built for the exact arithmetic only (its kernel instances are the exact unit's)", fn);
    return VP_OK;
}
// the planes a caller hands in: planes_of(mode) accumulators -- of each half, with halves --, all given and all different; with_stats: as many record buffers likewise.
// 0: so they are; 1: a null pointer among them; 2: one buffer given twice
int plane_buffers_check(const PlaneSet& S, bool with_stats)
{
    for (int k = 0; k < S.count(); k++)
        if (!S.acc[k] || (with_stats && !S.rec[k])) return 1;
    for (int k = 1; k < S.count(); k++)
        for (int j = 0; j < k; j++)
            if (S.acc[j] == S.acc[k] || (with_stats && S.rec[j] == S.rec[k])) return 2;
    return 0;
}
PlaneSet plane_set(int mode, vp_float4* d0, vp_float4* d1, vp_float4* d2, vp_pixel_stats* r0, vp_pixel_stats* r1, vp_pixel_stats* r2)
{
    PlaneSet S = {};
    S.mode = mode;
    S.acc[0] = (float4*)d0; S.acc[1] = (float4*)d1; S.acc[2] = (float4*)d2;
    S.rec[0] = (PixelStatsDev*)r0; S.rec[1] = (PixelStatsDev*)r1; S.rec[2] = (PixelStatsDev*)r2;
    return S;
}
// the vp_render_frames_* calls with planes: S as the caller handed it in, records (with_stats) or none
static int plane_call(const char* fn, const PlaneSet& S, bool with_stats, int first_frame, int n_frames, const Param* p)
{
    if (plane_buffers_check(S, with_stats) || !p || n_frames <= 0 || first_frame < 0) return fail(VP_E_ARG, "%s: bad arguments", fn);
    int rc = plane_state_check(fn, S.groups());
    if (rc) return rc;
    if ((rc = ensure_device())) return rc;
    // the call is serial and runs on the caller's stream: look-ahead batches stop, pipelined launches are waited for
    if ((rc = la_quiesce())) return rc;
    return do_render((vp_float4*)S.acc[0], first_frame, n_frames, p, false, nullptr, nullptr, &S);
}

}  // namespace vph

using namespace vph;

extern "C" {
int vp_render_frames(vp_float4* d_output, int first_frame, int n_frames, const Param* p)
{
    return do_render(d_output, first_frame, n_frames, p);
}
int vp_render_frames_layers(vp_float4* d_fg, vp_float4* d_trans, int first_frame, int n_frames, const Param* p)
{
    return plane_call("vp_render_frames_layers", plane_set(PLANES_LAYERS, d_fg, d_trans), false, first_frame, n_frames, p);
}
int vp_render_frames_groups(vp_float4* d_sun, vp_float4* d_sky, int first_frame, int n_frames, const Param* p)
{
    return plane_call("vp_render_frames_groups", plane_set(PLANES_GROUPS, d_sun, d_sky), false, first_frame, n_frames, p);
}
int vp_render_frames_layers_stats(vp_float4* d_fg, vp_float4* d_trans, vp_pixel_stats* d_fg_stats, vp_pixel_stats* d_trans_stats, int first_frame, int n_frames,
                                  const Param* p)
{
    return plane_call("vp_render_frames_layers_stats", plane_set(PLANES_LAYERS, d_fg, d_trans, nullptr, d_fg_stats, d_trans_stats), true, first_frame, n_frames, p);
}
int vp_render_frames_groups_stats(vp_float4* d_sun, vp_float4* d_sky, vp_pixel_stats* d_sun_stats, vp_pixel_stats* d_sky_stats, int first_frame, int n_frames,
                                  const Param* p)
{
    return plane_call("vp_render_frames_groups_stats", plane_set(PLANES_GROUPS, d_sun, d_sky, nullptr, d_sun_stats, d_sky_stats), true, first_frame, n_frames, p);
}
int vp_render_frames_group_layers(vp_float4* d_sun, vp_float4* d_sky, vp_float4* d_trans, int first_frame, int n_frames, const Param* p)
{
    return plane_call("vp_render_frames_group_layers", plane_set(PLANES_GROUP_LAYERS, d_sun, d_sky, d_trans), false, first_frame, n_frames, p);
}
int vp_render_frames_group_layers_stats(vp_float4* d_sun, vp_float4* d_sky, vp_float4* d_trans, vp_pixel_stats* d_sun_stats, vp_pixel_stats* d_sky_stats,
                                        vp_pixel_stats* d_trans_stats, int first_frame, int n_frames, const Param* p)
{
    return plane_call("vp_render_frames_group_layers_stats", plane_set(PLANES_GROUP_LAYERS, d_sun, d_sky, d_trans, d_sun_stats, d_sky_stats, d_trans_stats), true,
                      first_frame, n_frames, p);
}
// Half-buffer renders (include/volpath.h; vp_kernels.h PLANES_ONE with PlaneSet::halves): vp_render_frames_stats' launches -- the mode sets neither
// LaunchDev::layers nor LaunchDev::groups, so every kernel is the beauty instance and nothing a plane call refuses is refused -- into one
// staging plane, and a reduce that hands frame f to half_of_frame(f).  Serial on the caller's stream like a plane call.
int vp_render_frames_halves_stats(vp_float4* d_h0, vp_float4* d_h1, vp_pixel_stats* d_h0_stats, vp_pixel_stats* d_h1_stats, int first_frame, int n_frames,
                                  const Param* p)
{
    PlaneSet S = plane_set(PLANES_ONE, d_h0, d_h1, nullptr, d_h0_stats, d_h1_stats);
    S.halves = true;
    const int bad = plane_buffers_check(S, true);
    if (bad == 1 || !p) return fail(VP_E_ARG, "vp_render_frames_halves_stats: null pointer");
    if (bad) return fail(VP_E_ARG, "vp_render_frames_halves_stats: the two accumulators, and the two record buffers, are different buffers");
    if (n_frames <= 0 || first_frame < 0)
        return fail(VP_E_ARG, "vp_render_frames_halves_stats: frames [%d, %d + %d) out of range", first_frame, first_frame, n_frames);
    int rc = ensure_device();
    if (rc) return rc;
    if ((rc = la_quiesce())) return rc;
    return do_render(d_h0, first_frame, n_frames, p, false, nullptr, nullptr, &S);
}
// Halves of a call with planes (include/volpath.h; vp_kernels.h PlaneSet::halves): the plane call's launches, staging and state check,
// and a reduce that hands the planes' samples of frame f to the planes of half half_of_frame(f).
int vp_render_frames_planes_halves_stats(int mode, const vp_plane_bufs* h0, const vp_plane_bufs* h1, int first_frame, int n_frames, const Param* p)
{
    static const char fn[] = "vp_render_frames_planes_halves_stats";
    if (mode != VP_PLANES_LAYERS && mode != VP_PLANES_GROUPS && mode != VP_PLANES_GROUP_LAYERS) return fail(VP_E_ARG, "%s: unknown mode %d", fn, mode);
    if (!h0 || !h1 || !p) return fail(VP_E_ARG, "%s: null pointer", fn);
    static_assert(VP_PLANES_LAYERS == PLANES_LAYERS && VP_PLANES_GROUPS == PLANES_GROUPS && VP_PLANES_GROUP_LAYERS == PLANES_GROUP_LAYERS, "the public modes are the plane modes");
    PlaneSet S = {};
    S.mode = mode; S.halves = true;
    for (int h = 0; h < 2; h++)
        for (int k = 0; k < S.n(); k++)
        {
            S.acc[h * S.n() + k] = (float4*)(h ? h1 : h0)->acc[k];
            S.rec[h * S.n() + k] = (PixelStatsDev*)(h ? h1 : h0)->rec[k];
        }
    const int bad = plane_buffers_check(S, true);
    if (bad == 1) return fail(VP_E_ARG, "%s: null pointer among the planes of a half", fn);
    if (bad) return fail(VP_E_ARG, "%s: the accumulators of the two halves, and their record buffers, are all different buffers", fn);
    if (n_frames <= 0 || first_frame < 0) return fail(VP_E_ARG, "%s: frames [%d, %d + %d) out of range", fn, first_frame, first_frame, n_frames);
    int rc = plane_state_check(fn, S.groups());
    if (rc) return rc;
    if ((rc = ensure_device())) return rc;
    if ((rc = la_quiesce())) return rc;
    return do_render((vp_float4*)S.acc[0], first_frame, n_frames, p, false, nullptr, nullptr, &S);
}
int vp_relight_composite(vp_float4* dst, const vp_float4* sun, const vp_float4* sky, const vp_float4* trans, const float sun_gain[3], const float sky_gain[3],
                         const vp_float4* plate, const float plate_rgb[3], int size, float scale)
{
    if (!dst || !sun || !sky || !trans || !sun_gain || !sky_gain || size < 0 || (!plate && !plate_rgb)) return fail(VP_E_ARG, "vp_relight_composite: bad arguments");
    int rc = ensure_device();
    if (rc) return rc;
    if (size)
        launch_relight_composite((float4*)dst, (const float4*)sun, (const float4*)sky, (const float4*)trans, make_float3(sun_gain[0], sun_gain[1], sun_gain[2]),
                                 make_float3(sky_gain[0], sky_gain[1], sky_gain[2]), (const float4*)plate, plate ? 0.0f : plate_rgb[0], plate ? 0.0f : plate_rgb[1],
                                 plate ? 0.0f : plate_rgb[2], size, scale, G.stream);
    HIPCHK(hipGetLastError());
    return VP_OK;
}
int vp_relight(vp_float4* dst, const vp_float4* sun, const vp_float4* sky, const float sun_gain[3], const float sky_gain[3], int size, float scale)
{
    if (!dst || !sun || !sky || !sun_gain || !sky_gain || size < 0) return fail(VP_E_ARG, "vp_relight: bad arguments");
    int rc = ensure_device();
    if (rc) return rc;
    if (size)
        launch_relight((float4*)dst, (const float4*)sun, (const float4*)sky, make_float3(sun_gain[0], sun_gain[1], sun_gain[2]),
                       make_float3(sky_gain[0], sky_gain[1], sky_gain[2]), size, scale, G.stream);
    HIPCHK(hipGetLastError());
    return VP_OK;
}
int vp_composite(vp_float4* dst, const vp_float4* fg, const vp_float4* trans, const vp_float4* plate, const float plate_rgb[3], int size, float scale)
{
    if (!dst || !fg || !trans || size < 0 || (!plate && !plate_rgb)) return fail(VP_E_ARG, "vp_composite: bad arguments");
    int rc = ensure_device();
    if (rc) return rc;
    if (size)
        launch_composite((float4*)dst, (const float4*)fg, (const float4*)trans, (const float4*)plate, plate ? 0.0f : plate_rgb[0], plate ? 0.0f : plate_rgb[1],
                         plate ? 0.0f : plate_rgb[2], size, scale, G.stream);
    HIPCHK(hipGetLastError());
    return VP_OK;
}
int vp_enable_counters(int on)
{
    int rc = pipe_quiesce();
    if (rc) return rc;
    G.count = on != 0;
    return VP_OK;
}
int vp_read_counters(vp_counters* out, int reset)
{
    if (int rc = await_launches(false, false)) return rc;
    unsigned long long h[kCounterWords];
    HIPCHK(hipMemcpy(h, G.d_counters, sizeof h, hipMemcpyDeviceToHost));
    if (out)
    {
        memset(out, 0, sizeof *out);
        out->samples = h[0]; out->density_lookups = h[1]; out->density_loads = h[12]; out->bound_lookups = h[2];
        out->opacity_lookups = h[3]; out->env_lookups = h[4]; out->scatters = h[5];
        if (getenv("VP_DEBUG_COUNTERS") && h[6])
            fprintf(stderr, "[vp] wave-iterations %llu, active lane-steps %llu (%.1f per iteration), slow-path visits %llu (every %.1f iterations), "
                    "shadow lane-steps %llu; wave cycles: slow path %llu, fast loop %llu (%.1f%% slow, %.0f cycles per visit, %.0f per step)\n",
                    h[6], h[7], h[6] ? (double)h[7] / h[6] : 0.0, h[8], h[8] ? (double)h[6] / h[8] : 0.0, h[9], h[10], h[11],
                    100.0 * h[10] / (double)(h[10] + h[11] + 1), h[8] ? (double)h[10] / h[8] : 0.0, h[6] ? (double)h[11] / h[6] : 0.0);
    }
    if (getenv("VP_DEBUG_COUNTERS"))
    {
        static const char* names[15] = {"setup", "half-step", "lookup+collision", "segment/ray end", "scatter", "nee", "phase", "background", "write", "refill", "global set-up", "fetch", "zero fetch (path)", "zero fetch (shadow)", "exit test"};
        fprintf(stderr, "[vp] exit flights: %llu tests, %llu paths ended; %llu null collisions in empty space on flights that WALKED out of the box (global majorant)\n", h[13], h[15], h[14]);
        fprintf(stderr, "[vp] block: wave executions, lanes per execution (of 64)\n");
        for (int b = 0; b < 15; b++)
            if (h[16 + 2 * b]) fprintf(stderr, "[vp]   %-18s %14llu  %5.1f\n", names[b], h[16 + 2 * b], (double)h[17 + 2 * b] / (double)h[16 + 2 * b]);
        if (h[72]) fprintf(stderr, "[vp]   %-18s %14llu  %5.1f\n", "control component", h[72], (double)h[73] / (double)h[72]);
        static const char* hn[3] = {"scatter", "segment/ray end", "setup"};
        for (int q = 0; q < 3; q++)
        {
            unsigned long long tot = 0;
            for (int k = 0; k < 8; k++) tot += h[48 + 8 * q + k];
            if (!tot) continue;
            fprintf(stderr, "[vp]   executions of %-16s by lanes 1-8 .. 57-64 (%%):", hn[q]);
            for (int k = 0; k < 8; k++) fprintf(stderr, " %5.1f", 100.0 * (double)h[48 + 8 * q + k] / (double)tot);
            fprintf(stderr, "\n");
        }
    }
    if (reset) HIPCHK(hipMemset(G.d_counters, 0, sizeof h));
    return VP_OK;
}
int vp_render_time_ms(double* total_ms, int* launches, int reset)
{
    if (int rc = await_launches(true, false)) return rc;
    // (each launch from where the launches before it ended: span_ms)
    double     tot = G.timed_ms;
    hipEvent_t end = G.last_end;
    for (auto& ev : G.events) tot += span_ms(ev.first, ev.second, end);
    if (total_ms) *total_ms = tot;
    if (launches) *launches = G.timed_n;
    if (reset)
    {
        // (the latest end is kept: a launch after the reset is still reported from where the ones before it ended)
        for (auto& ev : G.events) { put_event(ev.first); if (ev.second != end) put_event(ev.second); }
        if (end != G.last_end) { put_event(G.last_end); G.last_end = end; }
        G.events.clear();
        G.timed_ms = 0.0; G.timed_n = 0;
    }
    return VP_OK;
}
int vp_last_approach_mode(void) { return G.last_approach; }
int vp_last_approach_table(void) { return G.last_approach_table; }
int vp_last_light_const(void) { return G.last_light_const; }
int vp_last_lds_form(void) { return G.last_lds_form; }
int vp_last_arithmetic(void) { return G.last_arith; }
int vp_last_pipelined(void) { return G.last_pipelined; }
int vp_set_pipeline(int on)
{
    int rc = pipe_quiesce();
    if (rc) return rc;
    G.pipeline = on != 0;
    return VP_OK;
}
int vp_lookahead_stats(unsigned* launched, unsigned* cancelled_in_flight)
{
    if (launched) *launched = G.la_launched;
    if (cancelled_in_flight) *cancelled_in_flight = G.la_cancelled;
    return VP_OK;
}
int vp_render_class_time_ms(double ms[3], unsigned pixels[3], int reset)
{
    if (int rc = await_launches(true, true)) return rc;
    // (each class's kernel from where its predecessor of the class ended: span_ms)
    double     tot[3] = {G.class_ms[0], G.class_ms[1], G.class_ms[2]};
    hipEvent_t end[3] = {G.class_last_end[0], G.class_last_end[1], G.class_last_end[2]};
    for (auto& ev : G.class_events) tot[ev.cls] += span_ms(ev.a, ev.b, end[ev.cls]);
    if (ms) for (int i = 0; i < 3; i++) ms[i] = tot[i];
    if (pixels) { pixels[0] = G.n_general; pixels[1] = G.n_light; pixels[2] = G.n_miss; }
    if (reset)
    {
        for (auto& ev : G.class_events) { put_event(ev.a); if (ev.b != end[ev.cls]) put_event(ev.b); }
        for (int i = 0; i < 3; i++)
            if (end[i] != G.class_last_end[i]) { put_event(G.class_last_end[i]); G.class_last_end[i] = end[i]; }
        G.class_events.clear();
        G.class_ms[0] = G.class_ms[1] = G.class_ms[2] = 0.0;
    }
    return VP_OK;
}
// the decomposition walk's segment table where this configuration has one (do_render asks the same): vp_prepare and vp_get_segment_table
static int prepare_segment_table(const Param* p, const float4* table, const float4** seg)
{
    *seg = nullptr;
    if (G.est == VP_EST_DECOMP && G.approach_fshift_max >= 6 && approach_possible(table, G.n_general)) return ensure_segment_table(p, table, seg);
    return VP_OK;
}
int vp_get_pixel_lists(const Param* p, uint32_t* dst, size_t count, unsigned counts[3])
{
    int rc = vp_prepare(p);
    if (rc) return rc;
    const size_t n = (size_t)G.n_general + G.n_light + G.n_miss;
    if (counts) { counts[0] = G.n_general; counts[1] = G.n_light; counts[2] = G.n_miss; }
    if (dst)
    {
        if (count < n) return fail(VP_E_ARG, "pixel lists hold %zu entries", n);
        if (n) HIPCHK(hipMemcpy(dst, G.d_tiles, n * sizeof(unsigned), hipMemcpyDeviceToHost));
    }
    return VP_OK;
}
int vp_prepare(const Param* p)
{
    int rc = ensure_device();
    if (rc) return rc;
    if (!p) return fail(VP_E_ARG, "vp_prepare: null Param");
    if (!G.have_volume || !G.have_cam) return fail(VP_E_STATE, "vp_prepare needs a volume and a camera");
    if ((rc = check_render(CHK_IMAGE, p))) return rc;
    const Shard sh = shard_of(p);
    if (sh.per_frame == 0)
    {
        // a shard without a tile (more ranks than tiles): empty lists
        G.n_general = G.n_light = G.n_miss = 0; G.tiles_key.clear();
        return VP_OK;
    }
    if ((rc = subpixel_check(p))) return rc;
    const float4 *table = nullptr, *seg = nullptr;
    const unsigned short* sc = nullptr; float ds = 0.0f;
    const float* thr = nullptr;
    const Param fine = subpixel_param(p);
    if ((rc = ensure_crawl_table(&fine, &table))) return rc;
    if ((rc = ensure_pixel_lists(p, table, sh))) return rc;
    const float4* ray = nullptr;
    if ((rc = ensure_ray_table(p, table, &ray))) return rc;
    if (G.have_sun && (rc = ensure_sun_clip(&sc, &ds))) return rc;
    if (G.est == VP_EST_GLOBAL && G.n_light && (rc = ensure_thr_table(p, &thr))) return rc;
    if ((rc = prepare_segment_table(p, table, &seg))) return rc;
    HIPCHK(hipStreamSynchronize(G.stream));
    return VP_OK;
}
int vp_get_segment_table(const Param* p, float* dst, size_t count, int* cap)
{
    if (cap) *cap = (int)(segment_table_records() / 2u);
    if (!dst) return VP_OK;
    int rc = vp_prepare(p);
    if (rc) return rc;
    // what vp_prepare has just built, if this configuration has a table at all (both tables are found cached)
    const float4 *table = nullptr, *seg = nullptr;
    const Param fine = subpixel_param(p);
    if ((rc = ensure_crawl_table(&fine, &table))) return rc;
    if ((rc = prepare_segment_table(p, table, &seg))) return rc;
    if (!seg) return fail(VP_E_STATE, "no segment table in this configuration (decomposition estimator on a uchar volume, approach walk and table switched on)");
    const size_t need = (size_t)G.n_general * segment_table_records() * 4;
    if (count < need) return fail(VP_E_ARG, "segment table needs %zu floats", need);
    HIPCHK(hipMemcpy(dst, seg, need * sizeof(float), hipMemcpyDeviceToHost));
    return VP_OK;
}
int vp_get_ray_table(const Param* p, float* dst, size_t count)
{
    if (!p || !dst) return fail(VP_E_ARG, "vp_get_ray_table: null argument");
    int rc = vp_prepare(p);
    if (rc) return rc;
    // what vp_prepare has just built, if this configuration has a table at all (both tables are found cached)
    const float4 *table = nullptr, *ray = nullptr;
    const Param fine = subpixel_param(p);
    if ((rc = ensure_crawl_table(&fine, &table))) return rc;
    if ((rc = ensure_ray_table(p, table, &ray))) return rc;
    if (!ray) return fail(VP_E_STATE, "no ray table in this configuration (global-majorant estimator, no sub-pixel factor, general pixels, the table switched on)");
    const size_t need = (size_t)G.n_general * 8;
    if (count < need) return fail(VP_E_ARG, "ray table needs %zu floats", need);
    HIPCHK(hipMemcpy(dst, ray, need * sizeof(float), hipMemcpyDeviceToHost));
    return VP_OK;
}
int vp_last_ray_table(void) { return G.last_ray_table; }
// planes: 1 for vp_render_frames, 2 for vp_render_frames_groups (whose calls are staged for one frame too and never pipelined)
static int reserve_frames(const Param* p, int nframes, size_t planes)
{
    int rc = ensure_device();
    if (rc) return rc;
    if (!p || nframes <= 0) return fail(VP_E_ARG, "vp_reserve_frames: bad arguments");
    if ((rc = check_render(CHK_IMAGE, p))) return rc;
    const Shard sh = shard_of(p);
    if (sh.per_frame == 0 || (nframes == 1 && planes == 1)) return VP_OK;
    // what do_render would allocate for the first launch of such a job (a one-frame call accumulates directly and stages nothing)
    const Target T      = {&G.target[0], G.stream};
    const size_t f      = std::min<size_t>((size_t)nframes, stage_frames_cap(sh.per_frame, T.rt->stage.bytes, planes));
    const size_t need   = sh.per_frame * f * sizeof(float4) * planes;
    // (decomposition estimator: the stream's state beside each staging slot of the approach kernel's hand-over, where a launch of this
    // configuration can walk ahead at all -- do_render asks the same)
    const size_t need4  = (G.est == VP_EST_DECOMP && approach_built()) ? sh.per_frame * f * sizeof(uint2) : 0;
    if ((rc = reserve_handover(T, need4, need4))) return rc;   // (failing: no walk ahead then)
    if (need > T.rt->stage.bytes)
    {
        if (la_quiesce()) return VP_E_NODEVICE;
        HIPCHK(hipStreamSynchronize(G.stream));
        (void)reserve_stage(T, need, need, true);
        if (need > T.rt->stage.bytes) return VP_OK;   // the render call will stage smaller batches: same bits
    }
    // ... and pipeline slot 1 where the job goes in one launch (best effort: a call the slot cannot hold renders on the caller's stream)
    if (planes == 1 && G.pipeline && f == (size_t)nframes && pipe_streams()) (void)pipe_reserve(1, sh.per_frame, nframes, need4 > 0);
    return VP_OK;
}
int vp_reserve_frames(const Param* p, int nframes) { return reserve_frames(p, nframes, 1); }
int vp_reserve_frames_groups(const Param* p, int nframes) { return reserve_frames(p, nframes, 2); }
int vp_groups_frames_per_launch(const Param* p, int planes)
{
    int rc = ensure_device();
    if (rc) return rc;
    if (!p || planes < 1 || planes > 2) return fail(VP_E_ARG, "vp_groups_frames_per_launch: bad arguments");
    const Shard sh = shard_of(p);
    if (sh.per_frame == 0) return 0;
    return (int)std::min<size_t>(stage_frames_cap(sh.per_frame, G.target[0].stage.bytes, (size_t)planes), 0x7fffffff);
}
}  // extern "C"
