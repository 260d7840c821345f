// gs_renderer.cpp -- the renderer object and the render entry points of include/gs3d_hip.h.
//
// Frame orchestration replaces Renderer::recordPreprocessCommandBuffer / recordRenderCommandBuffer /
// draw (src/Renderer.cpp:468-529, 532-717, 366-426): every pass is enqueued on one HIP stream with
// grids that do not depend on the data-dependent counts V (visible) and D (instances); the counts
// live in device memory, so the reference's mid-frame fence wait + 4-byte readback + command-buffer
// re-record (Renderer.cpp:391-399, 538) disappears.  The frame's last kernel publishes the counters to
// pinned memory only to detect instance-buffer overflow (Renderer.cpp:541-563 grows and retries too)
// or a bin that outgrew the bin-local depth order (then the frame is re-run on the global path).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>
#include <memory>
#include <utility>
#include <vector>

#include "gs_blend_tuner.h"
#include "gs_depth_policy.h"
#include "gs_internal.h"

using namespace gs_host;

// ------------------------------------------------------------------------------------------
// gs_renderer
// ------------------------------------------------------------------------------------------
// One complete set of per-frame device buffers + the stream its passes run on.  Frames alternate between
// sets, so with >= 2 sets the small launch-bound passes of frame i+1 (scans, binning) overlap the
// VALU-bound blend of frame i on the same GPU.
struct FrameBuffers {
    hipStream_t stream = nullptr;
    // per-Gaussian attributes
    DevBuf<uint32_t> tiles;
    DevBuf<float> depth;
    DevBuf<ushort4> aabb;
    DevBuf<gs::AttrRecord> rec;  // one 64-byte record per Gaussian: what the blend gathers
    DevBuf<uint4> vis;           // the frame's visible Gaussians as dense lists (gs::AttrView::vis): level 1's input on the bin-local path
    DevBuf<uint32_t> vis_count;  // the lists' counters, one per 128 bytes (the word behind each: the finished frame's count)
    // what the last frame on this set left of tiles / depth / aabb: written (0), or for the taps to rebuild -- from the dense lists it
    // streamed (1), or, a frame of the one-pass level 1, from its visibility bits and records (2)
    int planes_stale = 0;
    DevBuf<uint64_t> vis_mask;   // the one-pass level 1's visibility bits (gs::L1Fused::vis_mask)
    uint32_t vis_region_slots = 0;
    // global depth order (only allocated when that path is taken)
    DevBuf<uint32_t> dkeys[2], dvals[2];
    DevBuf<uint32_t> block_hist, digit_total;
    // two-level binning
    DevBuf<uint32_t> l1_hist, bin_count;  // [padded bins][level-1 blocks], [1024 counts + 1024 offsets]
    DevBuf<uint32_t> cand;                // [3 x cand_capacity] bin-major candidates: 12-byte records {depth bits, id, box} on the bin-local path, plain ids otherwise
    DevBuf<uint32_t> l1_words;            // the one-pass level 1's counters (gs::L1Fused::words), zero between frames
    DevBuf<uint32_t> sorted;              // [capacity + 4] per-tile lists, bin-major
    DevBuf<uint32_t> ranges;              // [T][2]
    DevBuf<uint8_t> slabs;                // depth-slab descriptors (level 4; allocated on first use)
    uint32_t slab_epoch = 0;              // k_bin_queue: one value per launch on these descriptors (BinLaunch::slab_epoch)
    DevBuf<gs::Counters> counters;
    DevBuf<uint64_t> stamps;              // the frame's timeline, written by its kernels (gs_kernels.h: FrameStamp)
    // HIP-graph replay (gs_set_graph_mode): the frame's fixed-shape launches captured once per configuration
    DevBuf<gs::FrameParams> params;
    // ... one per setting of the blend's lockstep: the tuner flips it several times per measurement, and re-capturing the frame on every
    // flip would make the measurement weigh the capture (round-5 advisor finding)
    hipGraphExec_t graph_execs[2] = {nullptr, nullptr};
    struct GraphKey {
        int level = -1, bin_shift = -1, hw_exp = 0, contract = 1;
        bool antialiased = false, lockstep = false, l1_fused = false, tile_cull = false;
        uint32_t width = 0, height = 0, capacity = 0, cand_capacity = 0;
        const void *tile_order = nullptr, *ranges = nullptr, *sh16 = nullptr;
        bool operator==(const GraphKey& o) const {
            return level == o.level && bin_shift == o.bin_shift && hw_exp == o.hw_exp && contract == o.contract &&
                   antialiased == o.antialiased && lockstep == o.lockstep && l1_fused == o.l1_fused && tile_cull == o.tile_cull &&
                   width == o.width && height == o.height && capacity == o.capacity && cand_capacity == o.cand_capacity &&
                   tile_order == o.tile_order && ranges == o.ranges && sh16 == o.sh16;
        }
    } graph_keys[2];
    void drop_graph(int which) {
        if (graph_execs[which]) (void)hipGraphExecDestroy(graph_execs[which]);
        graph_execs[which] = nullptr;
        graph_keys[which] = GraphKey{};
    }
    void drop_graph() {
        drop_graph(0);
        drop_graph(1);
    }
    size_t n = 0;
    bool ready = false;

    void init(size_t n_, uint32_t capacity, uint32_t cand_capacity, bool dense_lists) {
        n = n_;
        HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        tiles.alloc(n);
        depth.alloc(n);
        aabb.alloc(n);
        rec.alloc(n);
        vis_region_slots = gs::vis_region_slots(static_cast<uint32_t>(n));
        if (dense_lists) ensure_dense_lists();  // only scenes of >= dense_min Gaussians ever use them (16 B x N)
        l1_hist.alloc(1025 * static_cast<size_t>(gs::bin_level1_columns(static_cast<uint32_t>(n))));  // + the row of visible counts
        bin_count.alloc(2048);  // counts, then offsets (gs_bin.h: kBinOffsets)
        vis_mask.alloc((n + 63) / 64 + 1);
        l1_words.alloc(gs::kL1FusedWords);
        HIP_CHECK(hipMemset(l1_words.p, 0, l1_words.n * sizeof(uint32_t)));  // every one-pass frame's LAST kernel zeroes them again
        counters.alloc(1);
        stamps.alloc(gs::ST_COUNT);
        HIP_CHECK(hipMemset(stamps.p, 0, gs::ST_COUNT * sizeof(uint64_t)));
        params.alloc(1);
        set_capacity(capacity);
        set_cand_capacity(cand_capacity);
        ready = true;
    }
    void ensure_dense_lists() {  // the dense lists of visible Gaussians: only scenes of >= dense_min Gaussians ever use them (16 B x N)
        if (vis.p) return;
        vis.alloc(static_cast<size_t>(gs::kVisRegions) * vis_region_slots);
        vis_count.alloc(gs::kVisRegions * gs::kVisCounterStride);
        HIP_CHECK(hipMemset(vis_count.p, 0, vis_count.n * sizeof(uint32_t)));  // every frame's LAST kernel zeroes them again
    }
    void ensure_depth_order() {  // the global depth-order path's buffers
        if (dkeys[0].p) return;
        for (int k = 0; k < 2; ++k) {
            dkeys[k].alloc(n);
            dvals[k].alloc(n);
        }
        block_hist.alloc(256 * static_cast<size_t>(gs::kSortMaxBlocks));
        digit_total.alloc(256);
    }
    void set_capacity(uint32_t cap) {  // D: the per-tile lists
        drop_graph();  // the captured launches hold the old buffers
        sorted.alloc(static_cast<size_t>(cap) + 4);  // + 4: a 16-byte list store that starts inside the capacity may end past it
    }
    // E1: the level-1 candidates, sized on their own (round 5; they used to share the instance capacity: 3 words x 8 N, six times what
    // config B's 0.74 M records need).  A frame whose candidates overflow leaves a gap of unwritten entries that k_bin_build still
    // gathers through before the frame is re-run: the gap must hold valid Gaussian ids (0), never whatever hipMalloc handed back.
    void set_cand_capacity(uint32_t ccap) {
        drop_graph();
        cand.alloc(3 * static_cast<size_t>(ccap));
        HIP_CHECK(hipMemset(cand.p, 0, 3 * static_cast<size_t>(ccap) * sizeof(uint32_t)));
    }
    void sync() const { HIP_CHECK(hipStreamSynchronize(stream)); }
    void sync_nothrow() const { (void)hipStreamSynchronize(stream); }  // (the destructor's path)
    ~FrameBuffers() {
        drop_graph();
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// What a frame runs with: everything gs_renderer::plan_frame decides before the frame's first launch.  Decided once and stored once
// -- in the frame's slot of the ring, and, when the frame is the last one, in LastFrame; the graph key is made from it.
struct FramePlan {
    uint32_t width = 0, height = 0, tx = 0, ty = 0;  // the frame's size and its grid of tiles ...
    uint64_t num_tiles = 0;     // ... tx * ty of them
    int level = 0;              // the depth-order level the frame runs at (DepthPolicy::frame_level) ...
    BinGeometry geo{};          // ... on this bin grid
    bool l1_fused = false;      // k_preprocess files the level-1 candidates itself (gs::L1Fused) ...
    uint32_t l1_cap = 0;        // ... into bin regions of this many records
    bool dense_list = false;    // level 1 streams the dense lists of visible Gaussians, which k_preprocess writes beside the planes
    bool culled = false;        // level 2 makes the lists from the records' alpha-cut boxes (gs_renderer::tile_cull)
    bool lockstep = false;      // the blend's lockstep setting ...
    uint32_t tune_round = 0;    // ... and the tuner's round it belongs to (samples of an earlier round are ignored)
    int tune_shape = 0;         // ... and which of the bank's tuners (one per frame shape) that was
    bool stamped = false;       // the frame has Gaussians and pixels (one without launches nothing that stamps or publishes the counters)
    bool bin_local() const { return level < DepthPolicy::kGlobalLevel; }
    // the level-1 kernels that take their items in any order (bin-local path, bins of <= 8 x 8 tiles)
    bool l1_any_order() const { return bin_local() && geo.bin_shift <= 3; }
};

struct FrameSlot {
    gs_uniforms u{};
    float* rgba = nullptr;
    uint8_t* bgra = nullptr;
    hipEvent_t done = nullptr;           // the frame's one event: completion (round 5 bracketed every pass with one: 4.5 us of idle GPU each)
    gs::Counters* h_counters = nullptr;  // pinned
    uint64_t* h_stamps = nullptr;        // pinned [ST_COUNT]: the frame's timeline, written by its kernels and copied here by k_frame_end
    gs::FrameParams* h_params = nullptr;  // pinned staging of the frame's parameter block (graph replay)
    FramePlan plan;                      // what the frame ran with
};

// The frame the taps and the three passes answer from: the most recently enqueued one.  One value, replaced whole when a frame has
// been issued and emptied when the renderer loses its last frame (gs_renderer::forget_last_frame): nothing in it outlives its frame.
struct LastFrame {
    FrameBuffers* set = nullptr;  // the frame's buffers; null: there is no last frame
    FramePlan plan;
    uint64_t listed = 0;          // tile instances in the lists of the frame that retired last (once nothing is queued: this frame's)
    bool tap_lists = false;       // the renderer's tap buffers hold THIS frame's reference lists (gs_renderer::reference_lists)
    gs_uniforms u{};              // the uniforms the frame ran with ...
    bool antialiased = false;     // ... and its antialiased mode (gs_project_backward answers for the frame, not for a later setter)
};

struct gs_renderer {
    static constexpr int kMaxInFlight = 8;
    // twice what can be in flight: the frame-interval statistic reads the events of `latest_done`, which with frames
    // completing out of order across the sets may lie up to kMaxInFlight - 1 frames behind the oldest pending one
    static constexpr int kSlots = 2 * kMaxInFlight;

    gs_scene* scene = nullptr;
    bool timing = true;          // gs_set_timing: per-pass spans in the statistics (free since round 6: the kernels stamp them)
    double tick_ms = 1e-5;       // one tick of the kernels' clock in ms (100 MHz unless the device says otherwise)

    FrameBuffers sets[kMaxInFlight];
    int num_sets = 1;
    uint32_t capacity = 0;       // tile instances (D) the list buffers hold
    uint32_t cand_capacity = 0;  // level-1 candidates (E1) the candidate buffers hold
    uint32_t default_cand_capacity = 0;  // ... and what they held at creation (L1FusedPolicy::grow_to's ceiling is a multiple of it)
    // The one-pass level 1 (gs_kernels.h: L1Fused): when a frame takes it is L1FusedPolicy's rule; GS_L1_FUSED / gs_set_level1_fused set its mode
    L1FusedPolicy l1_policy;
    // gs_get_level1_fused's answer.  It does not drain, and it still describes a frame that failed or was dropped after it was enqueued,
    bool enqueued_l1_fused = false;  // so this one fact about the most recently enqueued frame is kept outside LastFrame
    // The alpha-cut tile cull (gs_tile_cull.h; GS_TILE_CULL / gs_set_tile_cull, default on).  k_preprocess's one-pass level 1 puts a
    // second, tighter box into every candidate record and k_bin_fast makes the lists the blend walks from it; D, the capacity check,
    // the statistics and the reference list taps follow the reference box.  Only those frames are culled: the three-kernel level 1,
    // the dense lists and the global path write the reference box twice, the slab levels read the reference half.
    bool tile_cull = true;
    LastFrame last_frame;

    // frames in flight: a ring of descriptors, all enqueued on `stream` (so device buffers are
    // reused in stream order); the host only waits when the ring is full or on gs_synchronize.
    FrameSlot slots[kSlots];
    int in_flight_limit = 1;  // the reference has FRAMES_IN_FLIGHT 1 (VulkanContext.h:6)
    uint64_t frames_enqueued = 0;
    int pending = 0;

    gs_frame_stats last{};  // stats of the most recently retired frame

    // How a frame's per-tile lists get their depth order, and the bin grid it runs with: the level of
    // the next frame, what an overflowed frame asks for, when to step back down -- all of it in gs_depth_policy.h.
    // GS_BIN_SHIFT sets its min_bin_shift, GS_SORT_PATH / gs_set_sort_path its sort_mode.
    DepthPolicy policy;
    static constexpr int kGlobalLevel = DepthPolicy::kGlobalLevel;
    bool graph_mode = false;     // replay each frame as one captured HIP graph (gs_set_graph_mode)
    // the blend's exp() (gs_set_exp_mode): 3 (default) the hardware's v_exp_f32 under the guard of render.comp:82 -- the reference's
    // decisions, its pixels to rounding noise; 2 libm's expf restated in binary64 -- the reference's bits; 0 pipeline polynomial, 1 v_exp_f32
    int exp_mode = 3;
    // a scene that holds an opacity > 1 is outside the guard's premises: blended with mode 2's arithmetic instead
    // (with the contractions on, mode 3 runs as mode 1 whatever the scene holds: there is nothing to guard -- gs3d_hip.h)
    int blend_exp_mode() const { return exp_mode == 3 && !contract && !scene->unit_opacity ? 2 : exp_mode; }
    bool contract = false;       // the three FMA contractions GLSL permits in render.comp:66,87 (gs_set_blend_contraction); default: as written
    bool antialiased = false;    // opacity scaled by the 0.3 dilation's compensation factor in k_preprocess (gs_set_antialiased)
    // The blend's LOCKSTEP (gs_blend.hip): the four waves of a tile take every chunk of its list together, so that their gathers of the
    // same records meet in L1.  Worth +25 % of the blend on trained-like scenes (L1-miss-bound: T(6e6) 505 -> 378 us; T(1e6) with three
    // frames in flight 2 675 -> 3 575 frames/s), -9 % on the S scenes (pair-loop-bound).  Nothing the renderer knows up front tells the
    // two apart, so it MEASURES (gs_blend_tuner.h: the rate at which frames complete over OFF - ON - OFF windows; the frames are bit-identical either way), keeps
    // lockstep where it wins by 3 %, and looks again every 4096 frames or when the frame's shape changes.  GS_BLEND_LOCKSTEP=0 / 1 (or gs_set_blend_lockstep)
    // pins it; the tuner then rests.  One tuner per frame shape (BlendTunerBank): alternating resolutions do not restart each other.
    BlendTunerBank tuners;
    // GS_L1_DENSE_MIN: scenes of at least this many Gaussians hand level 1 the dense lists of visible Gaussians (measured
    // A/B, profiles/r03_l1_dense_lists_ab.txt: 6 M Gaussians +2 % one frame at a time, +2..7 % with three in flight --
    // level 1 is several rounds of workgroups there; 1 M: -0.5 %, level 1 is one round of workgroups bound by its round
    // trips and k_preprocess pays 2 us for the lists; 2 M and 3.5 M, profiles/r03_l1_dense_threshold.txt: -2.2 % / -0.5 %
    // one frame at a time, +0.5 % with three in flight).  The GPU tests set it to 0 for small scenes.
    uint64_t dense_min = 4u << 20;
    // A scene that has its spatial copy (gs_scene: from 512 Ki Gaussians on) takes the lists below dense_min as well whenever it runs
    // the three any-order level-1 kernels -- the fall-back of the one-pass level 1: read in spatial order, the N-wide planes are
    // written by scene id, a store per Gaussian to a line of its own (B: 4 430 frames/s over the planes, 4 960 over the lists,
    // profiles/r16_l1_one_pass_ab.txt).  An explicit GS_L1_DENSE_MIN is taken at its word.
    bool dense_for_spatial = true;
    bool wants_dense_lists() const { return scene->n >= dense_min || (dense_for_spatial && scene->perm.p); }
    bool debug_levels = false, debug_occupancy = false;  // GS_DEBUG_LEVELS, GS_DEBUG_OCCUPANCY
    bool level2_queue = true;                            // GS_L2_QUEUE=0: level 4 as the two launches of round 4
    // test knobs (0: not given): start small so that the overflow / grow / re-run machinery is exercised by small scenes
    uint64_t initial_capacity = 0, initial_cand_capacity = 0;  // GS_INITIAL_CAPACITY, GS_INITIAL_CAND_CAPACITY
    // GS_DEBUG_STALLS=<ms>: a gs_render call that keeps the host longer than this is reported on stderr with the time each of
    // its parts took (wait for a free frame slot; the launches of each pass; the closing event records) -- how the runtime's
    // own hiccups (profiles/r05_stall_*.txt) are told from the renderer's
    double stall_ms = 0.0;

    // Every GS_* variable the renderer reads: once, at creation, before the first buffer set is sized (dense_min sizes it).  Each is
    // the initial value of the setter named beside it, or a debug / test knob that has no setter.
    void read_environment() {
        auto text = [](const char* name) { return std::getenv(name); };
        auto num = [&](const char* name, int unset) { return text(name) ? std::atoi(text(name)) : unset; };
        auto size = [&](const char* name) { return text(name) ? std::max<uint64_t>(256, std::strtoull(text(name), nullptr, 10)) : 0; };
        auto tri = [](int v) { return v < 0 ? -1 : (v != 0 ? 1 : 0); };
        tile_cull = num("GS_TILE_CULL", 1) != 0;                                     // gs_set_tile_cull
        dense_for_spatial = !text("GS_L1_DENSE_MIN");                                // (an explicit value is taken at its word)
        if (!dense_for_spatial) dense_min = std::strtoull(text("GS_L1_DENSE_MIN"), nullptr, 10);
        debug_levels = text("GS_DEBUG_LEVELS") != nullptr, debug_occupancy = text("GS_DEBUG_OCCUPANCY") != nullptr;
        level2_queue = num("GS_L2_QUEUE", 1) != 0;
        if (text("GS_DEBUG_STALLS")) stall_ms = std::atof(text("GS_DEBUG_STALLS"));
        if (text("GS_BLEND_LOCKSTEP")) tuners.pin(tri(num("GS_BLEND_LOCKSTEP", 0)));  // gs_set_blend_lockstep
        initial_capacity = size("GS_INITIAL_CAPACITY"), initial_cand_capacity = size("GS_INITIAL_CAND_CAPACITY");
        l1_policy.mode = tri(num("GS_L1_FUSED", l1_policy.mode));                    // gs_set_level1_fused
        graph_mode = num("GS_GRAPH", 0) != 0;                                        // gs_set_graph_mode
        exp_mode = std::min(3, std::max(0, num("GS_EXP_MODE", exp_mode)));           // gs_set_exp_mode
        contract = num("GS_BLEND_CONTRACTION", 0) != 0;                              // gs_set_blend_contraction
        antialiased = num("GS_ANTIALIASED", 0) != 0;                                 // gs_set_antialiased
        policy.min_bin_shift = std::min(5, std::max(2, num("GS_BIN_SHIFT", policy.min_bin_shift)));  // default bin edge
        policy.sort_mode = num("GS_SORT_PATH", 0);                                   // gs_set_sort_path, for hosts that cannot call it (the viewer)
        if (policy.sort_mode < 0 || policy.sort_mode > 2) throw Error(GS_ERR_INVALID, "GS_SORT_PATH must be 0 (auto), 1 (global) or 2 (bin-local)");
    }
    static constexpr int kLaps = 10;
    std::chrono::steady_clock::time_point laps[kLaps];
    void lap(int k) {
        if (stall_ms > 0.0) laps[k] = std::chrono::steady_clock::now();
    }
    void report_stall() {
        if (stall_ms <= 0.0) return;
        auto ms = [&](int a, int b) { return std::chrono::duration<double, std::milli>(laps[b] - laps[a]).count(); };
        if (ms(0, 9) < stall_ms) return;
        std::fprintf(stderr, "[gs3d] stall: frame %llu held the host %.3f ms: wait-for-slot %.3f, setup %.3f, preprocess %.3f, order %.3f, level1 %.3f, "
                             "level2 %.3f, blend %.3f, closing events %.3f\n", (unsigned long long)(frames_enqueued - 1), ms(0, 9), ms(0, 1), ms(1, 2), ms(2, 3),
                     ms(3, 4), ms(4, 5), ms(5, 6), ms(6, 7), ms(7, 9));
    }
    uint32_t retries = 0;       // lifetime count of re-run frames (statistics only)
    uint32_t redo_chain = 0;     // consecutive re-runs since a frame last retired cleanly: the runaway guard
    double total_ms[7] = {0, 0, 0, 0, 0, 0, 0};
    uint64_t total_frames = 0;
    uint64_t lifetime_frames = 0;  // frames retired since creation (gs_poll_stats)
    // completion-to-completion intervals of consecutive frames (the frame time a consumer sees with frames in flight)
    static constexpr size_t kIntervalRing = 8192;
    std::vector<float> intervals;
    bool prev_retired = false;  // the frame before the one being retired completed normally (its events are valid)
    uint64_t latest_done = 0;   // index of the retired frame whose blend ended last (at most sets - 1 frames back)

    ~gs_renderer() {
        for (auto& sl : slots) {
            if (sl.done) (void)hipEventDestroy(sl.done);
            if (sl.h_counters) (void)hipHostFree(sl.h_counters);
            if (sl.h_stamps) (void)hipHostFree(sl.h_stamps);
            if (sl.h_params) (void)hipHostFree(sl.h_params);
        }
    }

    void set_capacity(uint32_t cap) {
        capacity = cap;
        for (auto& fb : sets)
            if (fb.ready) fb.set_capacity(cap);
    }
    void set_cand_capacity(uint32_t ccap) {
        cand_capacity = ccap;
        for (auto& fb : sets)
            if (fb.ready) fb.set_cand_capacity(ccap);
    }

    void init() {
        HIP_CHECK(hipSetDevice(scene->device));
        {   // the clock the kernels stamp the frame's timeline with (wall_clock64): constant rate, in kHz
            int khz = 0;
            if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, scene->device) == hipSuccess && khz > 0) tick_ms = 1.0 / khz;
        }
        HIP_CHECK(gs::bin_prepare_device());
        if (debug_occupancy) gs::bin_debug_occupancy();
        for (auto& sl : slots) {
            HIP_CHECK(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
            HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&sl.h_stamps), gs::ST_COUNT * sizeof(uint64_t), hipHostMallocDefault));
            std::memset(sl.h_stamps, 0, gs::ST_COUNT * sizeof(uint64_t));
            HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&sl.h_counters), sizeof(gs::Counters), hipHostMallocDefault));
            *sl.h_counters = gs::Counters{};
            HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&sl.h_params), sizeof(gs::FrameParams), hipHostMallocDefault));
        }
        const uint64_t want = initial_capacity ? initial_capacity : std::max<uint64_t>(1u << 20, 8 * static_cast<uint64_t>(scene->n));
        capacity = static_cast<uint32_t>(std::min<uint64_t>(want, kMaxInstances));
        // candidates: E1 <= D always; ~1.5 per visible Gaussian with bins of 8 x 8 tiles, ~2 with 4 x 4 (config B 0.74 M, E 4.6 M, T 5.3 M)
        uint64_t want_cand = std::max<uint64_t>(1u << 18, 2 * static_cast<uint64_t>(scene->n));
        if (initial_cand_capacity) want_cand = initial_cand_capacity;
        else if (initial_capacity) want_cand = std::min<uint64_t>(want_cand, want);  // (the tests' small start applies to both)
        cand_capacity = static_cast<uint32_t>(std::min<uint64_t>(want_cand, capacity));
        default_cand_capacity = cand_capacity;
        sets[0].init(scene->n, capacity, cand_capacity, wants_dense_lists());
    }

    void set_num_sets(int k) {
        for (int i = 0; i < k; ++i)
            if (!sets[i].ready) sets[i].init(scene->n, capacity, cand_capacity, wants_dense_lists());
        num_sets = k;
    }

    // Blend workgroup -> tile table (shared by all buffer sets, rebuilt when the tile grid changes).  Workgroup b
    // runs on XCD b % 8 (observed dispatch rule), each XCD has a private L2, and the dispatcher hands out workgroups
    // in order, so a heavily loaded XCD holds the others back.  The screen is cut into blocks of B x B tiles and the
    // blocks are dealt to the XCDs like a skewed checkerboard: every XCD gets blocks from all over the image (balanced
    // for any scene) and the tiles of a block, which share most of their splat records, meet in one L2.
    DevBuf<uint32_t> tile_order;
    uint32_t order_tx = 0, order_ty = 0;
    void ensure_tile_order(uint32_t tx, uint32_t ty) {
        if (tx == order_tx && ty == order_ty && tile_order.p) return;
        drain();
        // B = 4 (64 x 64 px): on a clustered scene the blend takes 0.218 ms against 0.241 ms with one contiguous band
        // of tiles per XCD (max/mean XCD load 1.01 against 1.54); B = 2, 6, 8 and the bands all measured equal or slower
        constexpr uint32_t B = 4;
        const uint64_t nt = static_cast<uint64_t>(tx) * ty;
        std::vector<std::vector<uint32_t>> per_xcd(8);
        const uint32_t nbx = (tx + B - 1) / B, nby = (ty + B - 1) / B;
        for (uint32_t by = 0; by < nby; ++by)
            for (uint32_t bx = 0; bx < nbx; ++bx) {
                auto& list = per_xcd[(bx + 3 * by) % 8];
                for (uint32_t y = by * B; y < std::min(ty, (by + 1) * B); ++y)
                    for (uint32_t x = bx * B; x < std::min(tx, (bx + 1) * B); ++x) list.push_back(y * tx + x);
            }
        // workgroup b takes the next tile of XCD b % 8's list; lists that run dry borrow from the longest one
        std::vector<uint32_t> order(nt);
        size_t cursor[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (uint64_t b = 0; b < nt; ++b) {
            int x = static_cast<int>(b % 8);
            if (cursor[x] >= per_xcd[x].size()) {
                size_t best = 0;
                for (int k = 0; k < 8; ++k)
                    if (per_xcd[k].size() - cursor[k] > best) best = per_xcd[k].size() - cursor[k], x = k;
            }
            order[b] = per_xcd[x][cursor[x]++];
        }
        tile_order.ensure(nt);
        if (nt) HIP_CHECK(hipMemcpy(tile_order.p, order.data(), nt * sizeof(uint32_t), hipMemcpyHostToDevice));
        order_tx = tx;
        order_ty = ty;
    }

    BinGeometry bin_geometry(uint32_t tx, uint32_t ty) const {
        BinGeometry g;
        if (!policy.bin_geometry(tx, ty, &g)) throw Error(GS_ERR_INVALID, "resolution too large for the tile binning (max 16384 x 16384)");
        return g;
    }

    // What gs_render refuses because of the frame's size alone.  Depends on nothing but the size and min_bin_shift, which is fixed at
    // creation: the entry points ask before they wait for a queued frame or allocate, and a refused call changes nothing.
    void validate(const gs_uniforms& u) const {
        const uint32_t tx = tiles_across(u.width), ty = tiles_across(u.height);
        if (tx > 65535 || ty > 65535) throw Error(GS_ERR_INVALID, "resolution too large (tile box is 16-bit)");
        (void)bin_geometry(tx, ty);
    }

    // The renderer has no last frame (any more): the taps and the three passes refuse until a frame that is enqueued from here on
    // has retired.  `last`, what gs_get_stats reports, stays: the last frame that did retire.
    void forget_last_frame() { last_frame = LastFrame{}; }
    // (... and has retired: nothing is queued, and a frame that leaves the queue without retiring takes the last frame with it)
    bool has_last_frame() const { return last_frame.set != nullptr && pending == 0; }

    // ---- what a frame needs before it can be issued; asked before the wait of enqueue and again after it ----
    // buffers of the frame's set that a frame of `nt` tiles at depth-order level `lv` needs and the set does not have
    bool lacks_buffers(const FrameBuffers& fb, uint64_t nt, int lv) const {
        return 2 * nt > fb.ranges.n || (lv >= kGlobalLevel && !fb.dkeys[0].p) || (lv == gs::kBinSlabLevel && !fb.slabs.p);
    }
    // the one-pass level 1: does a frame of this size take it now (L1FusedPolicy)?
    L1FusedPolicy::Verdict l1_verdict(const gs_uniforms& u) const {
        const BinGeometry g = bin_geometry(tiles_across(u.width), tiles_across(u.height));
        return l1_policy.decide(policy.frame_level() < kGlobalLevel && g.bin_shift <= 3, scene->n < dense_min, scene->perm.p != nullptr,
                                u.width, u.height, g.bin_shift, cand_capacity, g.bins_x * g.bins_y);
    }
    // ... kept off it only by bin regions that are too small, the candidate buffers grow once: to this many candidates (0: they stay)
    uint32_t l1_growth(const gs_uniforms& u) const {
        if (scene->n == 0 || u.width == 0 || u.height == 0) return 0;
        const BinGeometry g = bin_geometry(tiles_across(u.width), tiles_across(u.height));
        return l1_policy.grow_to(l1_verdict(u), u.width, u.height, g.bin_shift, cand_capacity, g.bins_x * g.bins_y, default_cand_capacity);
    }

    // Three parts, in this order.  (1) Refuse what cannot run: nothing has been touched.  (2) Wait, if this frame needs buffers that
    // queued frames still use -- a failure of one of THOSE frames is thrown here, by rerun_queued, which has dropped them and the
    // last frame with them; nothing of this frame exists yet.  (3) issue(): decide, allocate, launch.  The frame becomes "the last
    // frame" only when every launch has been issued, and a failure in that part leaves the renderer without one (buffers of the last
    // frame's set, or the tile table every set shares, may already be this frame's).
    void enqueue(const gs_uniforms& u, float* d_rgba, uint8_t* d_bgra) {
        validate(u);
        HIP_CHECK(hipSetDevice(scene->device));
        const uint32_t tx = tiles_across(u.width), ty = tiles_across(u.height);
        // Every wait of this call.  New buffers, larger candidate buffers and a new tile table each wait for the queued frames that use
        // the old ones.  Retiring them may re-run a frame at another depth-order level or bin size (retire_oldest) and allocates on
        // the sets THEY run on: what this frame runs with, and which buffers its set lacks for that, is decided after the wait, when
        // nothing is queued and nothing can change it any more -- a frame queued with the level of before the wait fails at once
        // and, being judged as a failure of the new level, used to push the renderer onto the global path for slab_hold frames; and
        // a set that was looked at before the wait may lack the buffers of the level the wait ended at
        const bool new_grid = !(tx == order_tx && ty == order_ty && tile_order.p);
        if (pending > 0 && (new_grid || lacks_buffers(sets[frames_enqueued % num_sets], static_cast<uint64_t>(tx) * ty, policy.frame_level()) ||
                            l1_growth(u) != 0))
            drain();
        try {
            issue(u, d_rgba, d_bgra);
        } catch (...) {
            forget_last_frame();
            throw;
        }
    }

    // What the frame runs with, decided once.  The set and the renderer are made ready for it on the way, in the order these steps
    // have always had: the set's missing buffers, the one growth of the candidate buffers, the tile table, this shape's tuner -- the
    // decisions behind them (the one-pass level 1, its region capacity) see the candidate buffers as the frame will find them.
    FramePlan plan_frame(const gs_uniforms& u, FrameBuffers& fb) {
        FramePlan p;
        p.width = u.width, p.height = u.height;
        p.tx = tiles_across(u.width), p.ty = tiles_across(u.height), p.num_tiles = static_cast<uint64_t>(p.tx) * p.ty;
        p.stamped = scene->n != 0 && u.width != 0 && u.height != 0;
        p.level = policy.frame_level();
        if (lacks_buffers(fb, p.num_tiles, p.level)) {
            fb.ranges.ensure(2 * p.num_tiles);
            if (p.level >= kGlobalLevel) fb.ensure_depth_order();
            if (p.level == gs::kBinSlabLevel && !fb.slabs.p) {
                fb.slabs.alloc(static_cast<size_t>(gs::kSlabCapacity) * gs::kSlabDescBytes);
                HIP_CHECK(hipMemset(fb.slabs.p, 0, fb.slabs.n));  // no descriptor carries a launch's epoch yet
            }
        }
        if (const uint32_t grow = l1_growth(u); grow > cand_capacity) set_cand_capacity(grow);
        ensure_tile_order(p.tx, p.ty);
        p.tune_shape = tuners.select(u.width, u.height);  // this frame shape's own tuner (a new shape measures afresh)
        const BlendTuner& tuner = tuners.current();
        p.lockstep = tuner.current(), p.tune_round = tuner.round;
        p.geo = bin_geometry(p.tx, p.ty);
        p.l1_fused = p.stamped && l1_verdict(u) == L1FusedPolicy::kEngage;
        // the any-order level-1 kernels stream the dense list of visible Gaussians, which k_preprocess then writes beside the planes
        // (the lists exist only for scenes of >= dense_min Gaussians: FrameBuffers::init; the blend zeroes their counters)
        p.dense_list = p.l1_any_order() && !p.l1_fused && p.stamped && wants_dense_lists() && fb.vis.p;
        p.l1_cap = L1FusedPolicy::region_cap(cand_capacity, p.geo.bins_x * p.geo.bins_y);
        p.culled = tile_cull && p.l1_fused && p.level < gs::kBinSlabLevel;  // (the only frames that are: see tile_cull)
        return p;
    }

    // What a frame's own level 2 and the rebuild of its reference lists (reference_lists) hand gs::BinLaunch alike: the grid, the
    // capacities, the candidates with the counts and offsets of their bins, and the frame's own lists as the output.
    gs::BinLaunch bin_launch(const FrameBuffers& fb, const FramePlan& p) const {
        gs::BinLaunch b{};
        b.n_bound = static_cast<uint32_t>(scene->n);
        b.bin_count = fb.bin_count.p, b.cand = fb.cand.p;
        b.ranges = fb.ranges.p, b.sorted_gid = fb.sorted.p, b.counters = fb.counters.p;
        b.capacity = capacity, b.cand_capacity = cand_capacity;
        b.tiles_x = p.tx, b.tiles_y = p.ty;
        b.bins_x = p.geo.bins_x, b.bins_y = p.geo.bins_y;
        b.bin_shift = p.geo.bin_shift, b.grid_shift = p.geo.grid_shift;
        return b;
    }

    // What a captured frame was captured for: the plan and the renderer's settings its launches carry as arguments.
    FrameBuffers::GraphKey graph_key(const FrameBuffers& fb, const FramePlan& p, const void* sh16) const {
        FrameBuffers::GraphKey k;
        k.level = p.level, k.bin_shift = p.geo.bin_shift, k.hw_exp = blend_exp_mode(), k.contract = contract ? 1 : 0;
        k.antialiased = antialiased, k.lockstep = p.lockstep, k.l1_fused = p.l1_fused, k.tile_cull = tile_cull;
        k.width = p.width, k.height = p.height, k.capacity = capacity, k.cand_capacity = cand_capacity;
        k.tile_order = tile_order.p, k.ranges = fb.ranges.p, k.sh16 = sh16;
        return k;
    }

    // The scene as the kernels that read Gaussians take it: the frame's preprocess and the two backward passes to the parameters.
    gs::SceneView scene_view() const {
        const uint32_t n = static_cast<uint32_t>(scene->n);
        return {scene->render_blob(), scene->cov3d.p, n, static_cast<uint32_t>(gs::blob_stride(n)),
                scene->sh_half ? scene->sh16.p : nullptr, scene->acut.p, scene->perm.p};
    }

    // Part (3) of enqueue.  Nothing that is queued needs to retire in here (ensure_tile_order's own drain finds nothing queued).
    void issue(const gs_uniforms& u, float* d_rgba, uint8_t* d_bgra) {
        FrameSlot& sl = slots[frames_enqueued % kSlots];
        FrameBuffers& fb = sets[frames_enqueued % num_sets];
        hipStream_t stream = fb.stream;
        const uint32_t n = static_cast<uint32_t>(scene->n);
        const FramePlan plan = plan_frame(u, fb);
        lap(2);

        const gs::SceneView sv = scene_view();
        gs::Counters* cnt = fb.counters.p;
        gs::AttrView av{fb.tiles.p, fb.depth.p, fb.aabb.p, fb.rec.p, plan.dense_list ? fb.vis.p : nullptr, plan.dense_list ? fb.vis_count.p : nullptr,
                        fb.vis_region_slots};
        const gs::L1Fused lf{plan.l1_fused ? fb.l1_words.p : nullptr, fb.cand.p, plan.l1_cap, fb.vis_mask.p, plan.tx, plan.ty,
                             plan.geo.bins_x, plan.geo.bins_y, plan.geo.bin_shift, plan.geo.grid_shift};
        fb.planes_stale = plan.dense_list ? 1 : (plan.l1_fused ? 2 : 0);

        // the first and the last kernel of the frame clear / publish the counters themselves; the blit nodes (and
        // their fences) are only needed when one of the two is not launched
        if (!plan.stamped) {
            HIP_CHECK(hipMemsetAsync(cnt, 0, sizeof(gs::Counters), stream));
            HIP_CHECK(hipMemsetAsync(fb.ranges.p, 0, 2 * plan.num_tiles * sizeof(uint32_t), stream));  // no Gaussians: every tile (0, 0)
        }
        // the frame's launches; `fp` non-null = replayable form (per-frame values read from fb.params), no span events
        uint64_t* const stamps = fb.stamps.p;
        auto passes = [&](const gs::FrameParams* fp) {
            gs::launch_preprocess(sv, u, av, cnt, fp, stamps, antialiased, lf, stream);
            lap(3);
            if (!plan.bin_local() && n != 0) {
                // ---- global depth order of the visible Gaussians: 4 x 8-bit stable passes on bits(depth) ----
                const int blocks = std::max(1, std::min<int>(gs::kSortMaxBlocks, (n + gs::kSortTileKeys - 1) / gs::kSortTileKeys));
                const uint32_t* kin = reinterpret_cast<const uint32_t*>(fb.depth.p);
                const uint32_t* vin = nullptr;
                for (int pass = 0; pass < 4; ++pass) {
                    gs::RadixPass p{};
                    const int dst = pass & 1;
                    p.keys_in = kin;
                    p.vals_in = vin;
                    p.keys_out = fb.dkeys[dst].p;
                    p.vals_out = fb.dvals[dst].p;
                    p.n_in = &cnt->visible;
                    p.n_static = n;
                    p.tiles = fb.tiles.p;
                    p.n_out = &cnt->visible;
                    p.block_hist = fb.block_hist.p;
                    p.digit_total = fb.digit_total.p;
                    p.shift = pass * 8;
                    p.bits = 8;
                    p.blocks = blocks;
                    p.first = pass == 0;
                    p.stamps = pass == 0 ? stamps : nullptr;
                    gs::launch_radix_pass(p, stream);
                    kin = fb.dkeys[dst].p;
                    vin = fb.dvals[dst].p;
                }
            }
            lap(4);
            if (n != 0) {
                gs::BinLaunch b = bin_launch(fb, plan);
                b.order = plan.bin_local() ? nullptr : fb.dvals[1].p;
                b.n_items = plan.bin_local() ? nullptr : &cnt->visible;
                b.tiles = fb.tiles.p;
                b.aabb = fb.aabb.p;
                b.depth = fb.depth.p;
                b.vis = av.vis;
                b.vis_count = av.vis_count;
                b.vis_region_slots = av.vis_region_slots;
                b.hist = fb.l1_hist.p;
                b.l1_fused_words = lf.words;
                b.l1_fused_cap = plan.l1_cap;
                b.reference_boxes = !tile_cull;
                b.slabs = fb.slabs.p;
                b.slab_capacity = fb.slabs.p ? gs::kSlabCapacity : 0u;
                // level 4 as one launch over a queue of bins and slabs -- not in a captured frame (a replay repeats its arguments,
                // and a descriptor is ready when it holds THIS launch's epoch); GS_L2_QUEUE=0: the two launches of round 4
                b.slab_epoch = 0;
                if (level2_queue && !fp && plan.level == gs::kBinSlabLevel) {
                    if (++fb.slab_epoch == 0) ++fb.slab_epoch;
                    b.slab_epoch = fb.slab_epoch;
                }
                b.stamps = stamps;
                // ---- level 1: which Gaussian touches which bin (count + scan, then the per-bin candidate lists) ----
                // (one pass: k_preprocess has filed the candidates; level 2 reads the bins' cursors)
                if (!plan.l1_fused) {
                    gs::launch_bin_level1_count(b, stream);
                    gs::launch_bin_level1_scatter(b, plan.l1_any_order(), stream);
                }
                lap(5);
                // ---- level 2: order inside the bin (bin-local path), tile ranges, per-tile lists ----
                gs::launch_bin_level2(b, plan.level, stream);
            }
            lap(6);
            // ---- blend ----
            gs::launch_blend(fb.ranges.p, fb.sorted.p, tile_order.p, av, u.width, u.height, d_rgba, d_bgra, cnt,
                             plan.stamped ? sl.h_counters : nullptr, blend_exp_mode(), contract, fp, plan.lockstep, stamps, stream);
            gs::launch_frame_end(stamps, sl.h_stamps, fp, lf.words, gs::kVisRegions + (1u << (2 * plan.geo.grid_shift)), stream);
            lap(7);
        };
        const bool replay = graph_mode && plan.stamped;
        if (replay) {
            *sl.h_params = gs::FrameParams{u, d_rgba, d_bgra, sl.h_counters, sl.h_stamps};
            HIP_CHECK(hipMemcpyAsync(fb.params.p, sl.h_params, sizeof(gs::FrameParams), hipMemcpyHostToDevice, stream));
            const FrameBuffers::GraphKey key = graph_key(fb, plan, sv.sh16);
            const int gi = plan.lockstep ? 1 : 0;
            if (!fb.graph_execs[gi] || !(key == fb.graph_keys[gi])) {  // first frame of this configuration: capture its launches
                fb.drop_graph(gi);
                hipGraph_t graph = nullptr;
                HIP_CHECK(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
                try {
                    passes(fb.params.p);
                } catch (...) {
                    (void)hipStreamEndCapture(stream, &graph);
                    if (graph) (void)hipGraphDestroy(graph);
                    throw;
                }
                HIP_CHECK(hipStreamEndCapture(stream, &graph));
                const hipError_t e = hipGraphInstantiate(&fb.graph_execs[gi], graph, nullptr, nullptr, 0);
                (void)hipGraphDestroy(graph);
                HIP_CHECK(e);
                fb.graph_keys[gi] = key;
            }
            HIP_CHECK(hipGraphLaunch(fb.graph_execs[gi], stream));
        } else {
            passes(nullptr);
        }
        if (!plan.stamped) HIP_CHECK(hipMemcpyAsync(sl.h_counters, cnt, sizeof(gs::Counters), hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipEventRecord(sl.done, stream));
        HIP_CHECK(hipGetLastError());

        // every launch has been issued: this is the last frame now
        last_frame = LastFrame{&fb, plan};
        last_frame.u = u, last_frame.antialiased = antialiased;
        enqueued_l1_fused = plan.l1_fused;

        sl.plan = plan;
        sl.u = u, sl.rgba = d_rgba, sl.bgra = d_bgra;
        ++frames_enqueued;
        ++pending;
        lap(9);
    }

    FrameSlot& oldest() { return slots[(frames_enqueued - pending) % kSlots]; }
    FrameSlot& queued(int k) { return slots[(frames_enqueued - pending + k) % kSlots]; }

    // Wait for the oldest queued frame and record its stats; if it overflowed -- the instance or candidate buffers
    // (Renderer.cpp:541-563 grows and retries too) or a bin its depth-order level -- re-run it and every frame queued behind it.
    void retire_oldest() {
        FrameSlot& sl = oldest();
        HIP_CHECK(hipEventSynchronize(sl.done));
        if (sl.h_counters->overflow) {
            rerun_queued();
            return;
        }
        redo_chain = 0;
        policy.frame_retired(sl.plan.level, sl.h_counters->max_bin, sl.plan.geo.bin_shift);
        l1_policy.frame_retired(sl.u.width, sl.u.height, sl.plan.geo.bin_shift, sl.h_counters->max_bin, sl.h_counters->bin_entries, sl.h_counters->visible);
        last = frame_stats(sl);
        last_frame.listed = sl.plan.culled ? sl.h_counters->listed : sl.h_counters->instances;
        const float v[7] = {last.ms_preprocess, last.ms_prefix_sum, last.ms_preprocess_sort, last.ms_sort,
                            last.ms_tile_boundary, last.ms_render, last.ms_total};
        for (int k = 0; k < 7; ++k) total_ms[k] += v[k];
        ++total_frames;
        ++lifetime_frames;
        note_completion(sl, last.ms_total);
        --pending;
    }

    // The oldest queued frame overflowed: every queued frame is dropped from the ring, the policy picks the level and the bins,
    // the buffers grow to what the frames counted, and the frames are enqueued again.
    void rerun_queued() {
        for (auto& fb : sets)
            if (fb.ready) fb.sync();
        struct Redo {
            gs_uniforms u;
            float* rgba;
            uint8_t* bgra;
        };
        std::vector<Redo> redo;
        std::vector<DepthPolicy::QueuedFrame> ran;
        uint64_t need = 0, need_cand = 0;  // (0: that buffer did not run over)
        for (int k = 0; k < pending; ++k) {
            const FrameSlot& q = queued(k);
            const gs::Counters& c = *q.h_counters;
            redo.push_back({q.u, q.rgba, q.bgra});
            ran.push_back({q.plan.level, q.plan.geo.bin_shift, q.u.width, q.u.height, c.overflow, c.max_bin});
            // the one-pass level 1: a bin's region ran over (its cursor ended beyond it) -- the frames re-run on the three kernels
            if (q.plan.l1_fused && (c.overflow & 1u) && c.max_bin > q.plan.l1_cap) l1_policy.region_overflowed();
            if (c.overflow & 1u) {
                // which of the two ran over: the level-1 candidates (E1: the frame's instance count then means nothing -- its
                // bins were skipped) or the per-tile lists (D)
                if (c.bin_entries > cand_capacity) need_cand = std::max<uint64_t>(need_cand, c.bin_entries);
                else need = std::max<uint64_t>(need, c.instances);
            }
        }
        if (debug_levels) report_overflow();
        // the queued frames are dropped from the ring first: whatever is thrown below, the renderer stays usable.  The last frame is
        // one of them (the most recently enqueued one): its set holds the lists of a frame that overflowed or never finished, and
        // the renderer has no last frame until the frames enqueued again below have retired -- or, if one of the errors below is
        // thrown instead, until a later frame has
        frames_enqueued -= pending;
        pending = 0;
        prev_retired = false;
        forget_last_frame();
        switch (policy.frames_overflowed(ran.data(), static_cast<int>(ran.size()))) {
            case DepthPolicy::kDepthsTooCrowded:
                throw Error(GS_ERR_OVERFLOW, "a bin's depths are too crowded for the bin-local order (one depth bucket beyond a slab, or more than 65 equal depths in one): needs the global depth-order path");
            case DepthPolicy::kBinTooFull:
                throw Error(GS_ERR_OVERFLOW, "a bin holds more candidates than the bin-local sort can order");
            case DepthPolicy::kRerun:
                break;
        }
        // runaway guard: one frame may need a path fall-back and a few grow steps (each grow is sized from the counts
        // the overflowing frame reported, so it converges at once unless the chunk table and the lists take turns)
        if (++redo_chain > 8) throw Error(GS_ERR_OVERFLOW, "instance buffers overflowed repeatedly");
        if (need_cand > cand_capacity) {
            need_cand = need_cand + need_cand / 2 + 4096;  // 1.5x head-room: a moving camera should not re-grow every few frames
            if (need_cand > kMaxInstances) throw Error(GS_ERR_OVERFLOW, "more than 2^30 level-1 candidates");
            set_cand_capacity(static_cast<uint32_t>(need_cand));
        }
        if (need > capacity) {
            need = need + need / 2 + 4096;
            if (need > kMaxInstances) throw Error(GS_ERR_OVERFLOW, "more than 2^30 tile instances");
            set_capacity(static_cast<uint32_t>(need));
        }
        ++retries;
        for (const Redo& f : redo) enqueue(f.u, f.rgba, f.bgra);
    }

    void report_overflow() {  // GS_DEBUG_LEVELS: what made the renderer change its depth-order level
        std::fprintf(stderr, "[gs3d] frame %llu overflowed at level %d (refined %d, hold %u):", (unsigned long long)(frames_enqueued - pending),
                     oldest().plan.level, (int)policy.refined, policy.slab_hold);
        for (int k = 0; k < pending; ++k) {
            const FrameSlot& q = queued(k);
            std::fprintf(stderr, " [lvl %d bin 2^%d ovf %u max_bin %u E1 %u D %u slabs %u]", q.plan.level, q.plan.geo.bin_shift, q.h_counters->overflow,
                         q.h_counters->max_bin, q.h_counters->bin_entries, q.h_counters->instances, q.h_counters->slabs);
        }
        std::fprintf(stderr, " capacity %u candidates %u\n", capacity, cand_capacity);
    }

    gs_frame_stats frame_stats(const FrameSlot& sl) const {
        const FramePlan& p = sl.plan;
        gs_frame_stats st{};
        st.num_gaussians = scene->n;
        st.num_visible = sl.h_counters->visible;
        st.num_instances = sl.h_counters->instances;
        st.num_bin_entries = sl.h_counters->bin_entries;
        st.max_bin_entries = sl.h_counters->max_bin;
        st.sort_path = p.bin_local() ? 2u : 1u;
        st.sort_level = static_cast<uint32_t>(p.level);
        st.bin_tiles = 1u << p.geo.bin_shift;
        st.instance_capacity = capacity;
        // The frame's timeline as its kernels stamped it (gs_kernels.h: FrameStamp), in ticks of the device's constant-rate clock: a
        // span runs from the start of a pass's first kernel to the start of the next pass's -- the seam behind a pass belongs to it.
        const uint64_t* const ts = sl.h_stamps;
        auto span = [&](int a, int b) {
            const int64_t d = static_cast<int64_t>(ts[b] - ts[a]);
            return d > 0 ? static_cast<float>(static_cast<double>(d) * tick_ms) : 0.0f;
        };
        if (p.stamped) st.ms_total = span(gs::ST_PREPROCESS, gs::ST_END);
        if (p.stamped && timing) {
            // The reference's six span names (Renderer.cpp:484-526, 580-699).  prefix_sum = the level-1 count + scan,
            // preprocess_sort = the level-1 scatter (what lands where), sort = the global depth order (when taken) +
            // k_bin_build.  k_bin_build also produces the tile ranges: tile_boundary.comp's work has no kernel of
            // its own any more, so that span is 0 by construction.
            const bool global = !p.bin_local();  // (only then is ST_ORDER this frame's)
            // (one-pass level 1: no level-1 kernel stamped -- the pass is part of k_preprocess, and its two spans are 0)
            st.ms_preprocess = span(gs::ST_PREPROCESS, global ? gs::ST_ORDER : (p.l1_fused ? gs::ST_L2 : gs::ST_L1_COUNT));
            st.ms_prefix_sum = p.l1_fused ? 0.0f : span(gs::ST_L1_COUNT, gs::ST_L1_SCATTER);
            st.ms_preprocess_sort = p.l1_fused ? 0.0f : span(gs::ST_L1_SCATTER, gs::ST_L2);
            st.ms_sort = (global ? span(gs::ST_ORDER, gs::ST_L1_COUNT) : 0.0f) + span(gs::ST_L2, gs::ST_BLEND);
            st.ms_tile_boundary = 0.0f;
            st.ms_render = span(gs::ST_BLEND, gs::ST_END);
        }
        st.retries = retries;
        return st;
    }

    // The completion-to-completion interval the oldest queued frame closes, for gs_get_frame_intervals and the blend tuner.
    // Frames on different streams may finish out of order: measured against the latest completion so far.
    void note_completion(const FrameSlot& sl, float ms_total) {
        const uint64_t idx = frames_enqueued - pending;  // this frame
        if (prev_retired) {
            // (the frames' END stamps: one clock for every stream)
            const int64_t dticks = static_cast<int64_t>(sl.h_stamps[gs::ST_END] - slots[latest_done % kSlots].h_stamps[gs::ST_END]);
            const float dt = dticks > 0 ? static_cast<float>(static_cast<double>(dticks) * tick_ms) : 0.0f;  // 0: it had already finished when its predecessor did
            if (intervals.size() >= kIntervalRing) intervals.erase(intervals.begin(), intervals.begin() + kIntervalRing / 2);
            intervals.push_back(dt);
            // the blend tuner compares completion rates (or, for a host-paced consumer, the frames' own spans: BlendTuner::cost)
            tuners.sample(sl.plan.tune_shape, sl.u.width, sl.u.height, dt, ms_total, sl.plan.lockstep, sl.plan.tune_round);
            if (dt > 0.0f) latest_done = idx;
        } else {
            latest_done = idx;
        }
        prev_retired = true;
    }

    // what gs_get_stats and gs_poll_stats report: the most recently retired frame, the renderer's current figures over it
    void latest_stats(gs_frame_stats* out) const {
        *out = last;
        out->num_gaussians = scene->n;
        out->instance_capacity = capacity;
        out->retries = retries;
        out->blend_redo = out->blend_resolved = 0;  // (the blend's own counters: gs_get_stats reads them from the device)
    }

    void make_room() {
        while (pending >= in_flight_limit) retire_oldest();
    }
    void drain() {
        while (pending > 0) retire_oldest();
    }

    // What the passes over the last frame's tile lists do after their own argument checks (gs_accumulate_contributions,
    // gs_blend_features, gs_lift_pixels, gs_blend_backward, gs_project_backward, gs_camera_backward, gs_visible_mask,
    // gs_accumulate_densify_stats), in this order: queued frames retire (an overflowed one is re-run: the lists are the last
    // frame's, complete); without a frame the call is refused; with nothing asked for it is done; otherwise launch(lists, stream)
    // enqueues the pass over the frame's own lists on the last frame's stream and the call waits for it.
    template <class Launch>
    void over_last_frame(bool nothing_asked, Launch&& launch) {
        drain();
        if (!has_last_frame()) throw Error(GS_ERR_INVALID, "no frame rendered yet");
        if (nothing_asked) return;
        HIP_CHECK(hipSetDevice(scene->device));
        const FrameBuffers& fb = *last_frame.set;
        launch(gs::TileLists{fb.ranges.p, fb.sorted.p, tile_order.p, fb.rec.p, last_frame.plan.width, last_frame.plan.height}, fb.stream);
        HIP_CHECK(hipGetLastError());
        fb.sync();
    }

    // ---- the stage taps of the last frame (gs_debug_download, which has drained and found a last frame) ----
    // The reference's lists of the last frame.  An unculled frame's own lists are those.  For a culled one: level 2 once more over that
    // frame's candidate records with BinLaunch::reference_boxes, into buffers and counters of the taps' own, which the renderer keeps
    // across frames; whether they hold the last frame's lists is LastFrame::tap_lists.  Nothing of the frame moves.
    DevBuf<double> camera_partials;  // gs_camera_backward's rows of 27 partial sums, one per workgroup (allocated on first use)
    // gs_photometric_loss's scratch: the three binary64 P maps of an image (only a call that asks for grad_rgb with lambda > 0 needs
    // them) and the rows of three partial sums, one per workgroup.  Both grow on demand and are never shrunk.
    DevBuf<double> loss_maps, loss_partials;
    DevBuf<uint32_t> tap_ranges, tap_sorted;
    DevBuf<gs::Counters> tap_counters;
    using Lists = std::pair<const uint32_t*, const uint32_t*>;  // (ranges, lists)
    Lists reference_lists() {
        LastFrame& lf = last_frame;
        FrameBuffers& fb = *lf.set;
        if (!lf.plan.culled) return {fb.ranges.p, fb.sorted.p};
        if (!lf.tap_lists) {
            tap_ranges.ensure(2 * lf.plan.num_tiles);
            tap_sorted.ensure(static_cast<size_t>(capacity) + 4);
            tap_counters.ensure(1);
            HIP_CHECK(hipMemsetAsync(tap_counters.p, 0, sizeof(gs::Counters), fb.stream));
            // l1_fused_words stays null: level 2 reads the counts and offsets the frame's bin workgroups left in bin_count
            // (BuildArgs::bin_count_save); stamps stays null: the frame's timeline is the frame's
            gs::BinLaunch b = bin_launch(fb, lf.plan);
            b.ranges = tap_ranges.p, b.sorted_gid = tap_sorted.p, b.counters = tap_counters.p;
            b.reference_boxes = true;
            gs::launch_bin_level2(b, lf.plan.level, fb.stream);
            HIP_CHECK(hipGetLastError());
            gs::Counters c{};
            HIP_CHECK(hipMemcpyAsync(&c, tap_counters.p, sizeof c, hipMemcpyDeviceToHost, fb.stream));
            HIP_CHECK(hipStreamSynchronize(fb.stream));
            if (c.overflow != 0 || c.instances != last.num_instances)
                throw Error(GS_ERR_DEVICE, "the reference lists of a culled frame do not add up to the frame's instance count");
            lf.tap_lists = true;
        }
        return {tap_ranges.p, tap_sorted.p};
    }

    // tiles / depth / aabb of a frame that wrote no per-Gaussian planes, rebuilt on the first tap that asks for one of them
    void rebuild_planes() {
        FrameBuffers& fb = *last_frame.set;
        if (!fb.planes_stale) return;
        const gs::AttrView pv{fb.tiles.p, fb.depth.p, fb.aabb.p, fb.rec.p, fb.vis.p, fb.vis_count.p, fb.vis_region_slots};
        // the frame streamed the dense lists of visible Gaussians: from the lists
        if (fb.planes_stale == 1) gs::launch_vis_to_planes(pv, static_cast<uint32_t>(scene->n), fb.stream);
        // (... or took the one-pass level 1: from its visibility bits and the records)
        else gs::launch_records_to_planes(fb.vis_mask.p, scene->perm.p, pv, static_cast<uint32_t>(scene->n), last_frame.plan.width, last_frame.plan.height, fb.stream);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(fb.stream));
        fb.planes_stale = 0;
    }

    // fields of the 64-byte attribute records (only the visible Gaussians' records are written: the rest
    // of the tap is whatever an earlier frame left, like the reference's VertexAttribute buffer)
    void tap_record_field(int stage, void* dst, uint64_t bytes) {
        const uint64_t n = scene->n;
        const size_t width = stage == GS_STAGE_RADIUS || stage == GS_STAGE_B || stage == GS_STAGE_ALPHA_CUT ? 1 : 4;
        if (bytes < n * width * 4) throw Error(GS_ERR_INVALID, "destination too small for stage buffer");
        std::vector<gs::AttrRecord> recs(n);
        if (n) HIP_CHECK(hipMemcpy(recs.data(), last_frame.set->rec.p, n * sizeof(gs::AttrRecord), hipMemcpyDeviceToHost));
        float* out = static_cast<float*>(dst);
        for (uint64_t i = 0; i < n; ++i) {
            const gs::AttrRecord& a = recs[i];
            if (stage == GS_STAGE_RADIUS) out[i] = a.depth_radius.y;
            else if (stage == GS_STAGE_B) out[i] = a.b_cut_r.x;
            else if (stage == GS_STAGE_ALPHA_CUT) out[i] = a.b_cut_r.y;
            else std::memcpy(out + 4 * i, stage == GS_STAGE_CONIC_OPACITY ? &a.conic_op : &a.uv_rg, 16);
        }
    }

    // The per-tile lists are stored bin-major (the tiles of a bin consecutive, the bins wherever their workgroup's atomic add put
    // them); `ranges` holds each tile's (start, end) in that buffer.  The reference's buffers are the same lists laid end to end in
    // tile order: the taps present them so.  (The _CULLED pair: the frame's own lists, as the blend walked them; the others: the
    // reference's lists, made once more from the reference boxes where the frame's are culled.)
    void tap_lists(int stage, void* dst, uint64_t bytes) {
        const bool own = stage == GS_STAGE_LISTS_CULLED || stage == GS_STAGE_RANGES_CULLED;
        const auto [ranges_src, lists_src] = own ? Lists{last_frame.set->ranges.p, last_frame.set->sorted.p} : reference_lists();
        const uint64_t d = std::min<uint64_t>(own ? last_frame.listed : last.num_instances, capacity);
        if (stage == GS_STAGE_RANGES_CULLED) stage = GS_STAGE_RANGES;
        if (stage == GS_STAGE_LISTS_CULLED) stage = GS_STAGE_SORTED_GID;
        const uint64_t nt = last_frame.plan.num_tiles;
        std::vector<uint32_t> rg(2 * nt);
        if (nt) HIP_CHECK(hipMemcpy(rg.data(), ranges_src, rg.size() * 4, hipMemcpyDeviceToHost));
        if (stage == GS_STAGE_RANGES) {
            if (bytes < nt * 8) throw Error(GS_ERR_INVALID, "destination too small for stage buffer");
            uint32_t* out = static_cast<uint32_t*>(dst);
            uint64_t pos = 0;
            for (uint64_t t = 0; t < nt; ++t) {
                const uint32_t len = rg[2 * t + 1] - rg[2 * t];
                out[2 * t] = len ? static_cast<uint32_t>(pos) : 0u;  // tile_boundary.comp leaves absent tiles (0, 0)
                out[2 * t + 1] = len ? static_cast<uint32_t>(pos + len) : 0u;
                pos += len;
            }
            return;
        }
        if (bytes < d * 4) throw Error(GS_ERR_INVALID, "destination too small for stage buffer");
        std::vector<uint32_t> lists;
        if (stage == GS_STAGE_SORTED_GID) {
            lists.resize(capacity);
            HIP_CHECK(hipMemcpy(lists.data(), lists_src, lists.size() * 4, hipMemcpyDeviceToHost));
        }
        uint32_t* out = static_cast<uint32_t*>(dst);
        uint64_t pos = 0;
        for (uint64_t t = 0; t < nt; ++t)
            for (uint64_t i = rg[2 * t]; i < rg[2 * t + 1] && pos < d; ++i)
                out[pos++] = stage == GS_STAGE_SORTED_GID ? lists[i] : static_cast<uint32_t>(t);
    }
};

// What the passes refuse of their pointers before anything else looks at them: each of `members` {pointer, name}, in order, must
// be k-byte aligned (by the pointer's value alone: nothing is dereferenced, and a null pointer passes).
struct NamedPointer {
    const void* p;
    const char* name;
};
static void require_aligned(unsigned k, std::initializer_list<NamedPointer> members) {
    for (const NamedPointer& m : members)
        if (reinterpret_cast<uintptr_t>(m.p) % k != 0)
            throw Error(GS_ERR_INVALID, std::string(m.name) + " must be " + std::to_string(k) + "-byte aligned");
}

// ------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------
extern "C" {

int gs_renderer_create(gs_scene* scene, gs_renderer** out) {
    return guarded([&] {
        if (!scene || !out) throw Error(GS_ERR_INVALID, "null argument");
        auto r = std::make_unique<gs_renderer>();
        r->scene = scene;
        r->read_environment();  // (before init: GS_L1_DENSE_MIN sizes the buffer sets)
        r->init();
        *out = r.release();
    });
}

void gs_renderer_destroy(gs_renderer* r) {
    if (r)
        for (auto& fb : r->sets)
            if (fb.ready) fb.sync_nothrow();
    delete r;
}

int gs_render(gs_renderer* r, const gs_uniforms* u, float* d_rgba, uint8_t* d_bgra) {
    return guarded([&] {
        if (!r || !u) throw Error(GS_ERR_INVALID, "null argument");
        if (u->width == 0 || u->height == 0) throw Error(GS_ERR_INVALID, "empty framebuffer");
        r->validate(*u);  // (before any queued frame is waited for: a refused call changes nothing)
        r->lap(0);
        r->make_room();  // at most in_flight_limit frames queued; resolves pending overflows first
        r->lap(1);
        if (r->stall_ms > 0.0)
            for (int k = 2; k < gs_renderer::kLaps; ++k) r->laps[k] = r->laps[1];
        r->enqueue(*u, d_rgba, d_bgra);
        r->report_stall();
    });
}

int gs_render_host(gs_renderer* r, const gs_uniforms* u, float* h_rgba, uint8_t* h_bgra) {
    return guarded([&] {
        if (!r || !u) throw Error(GS_ERR_INVALID, "null argument");
        if (u->width == 0 || u->height == 0) throw Error(GS_ERR_INVALID, "empty framebuffer");
        r->validate(*u);  // (before anything is allocated or waited for: a refused call changes nothing)
        HIP_CHECK(hipSetDevice(r->scene->device));
        const size_t px = static_cast<size_t>(u->width) * u->height;
        DevBuf<float> d_rgba;
        DevBuf<uint8_t> d_bgra;
        if (h_rgba) d_rgba.alloc(px * 4);
        if (h_bgra) d_bgra.alloc(px * 4);
        r->drain();
        r->enqueue(*u, h_rgba ? d_rgba.p : nullptr, h_bgra ? d_bgra.p : nullptr);
        r->drain();
        if (h_rgba) HIP_CHECK(hipMemcpy(h_rgba, d_rgba.p, px * 4 * sizeof(float), hipMemcpyDeviceToHost));
        if (h_bgra) HIP_CHECK(hipMemcpy(h_bgra, d_bgra.p, px * 4, hipMemcpyDeviceToHost));
    });
}

int gs_synchronize(gs_renderer* r) {
    return guarded([&] {
        if (!r) throw Error(GS_ERR_INVALID, "null argument");
        r->drain();
    });
}

int gs_set_timing(gs_renderer* r, int enabled) {
    return guarded([&] {
        if (!r) throw Error(GS_ERR_INVALID, "null argument");
        r->drain();
        r->timing = enabled != 0;
    });
}

int gs_set_frames_in_flight(gs_renderer* r, int frames) {
    return guarded([&] {
        if (!r) throw Error(GS_ERR_INVALID, "null argument");
        if (frames < 1 || frames > gs_renderer::kMaxInFlight) throw Error(GS_ERR_INVALID, "frames in flight must be 1..8");
        r->drain();
        r->in_flight_limit = frames;
        r->set_num_sets(frames);
    });
}

int gs_get_stats(gs_renderer* r, gs_frame_stats* out) {
    return guarded([&] {
        if (!r || !out) throw Error(GS_ERR_INVALID, "null argument");
        r->drain();
        r->latest_stats(out);
        // written by the blend itself, after it published the other counters: read from the device (everything has retired)
        if (r->has_last_frame() && r->last_frame.set->counters.p) {
            gs::Counters c{};
            HIP_CHECK(hipMemcpy(&c, r->last_frame.set->counters.p, sizeof c, hipMemcpyDeviceToHost));
            out->blend_redo = c.blend_redo;
            out->blend_resolved = c.blend_resolved;
        }
    });
}

int gs_poll_stats(gs_renderer* r, gs_frame_stats* out, uint64_t* frames_retired) {
    return guarded([&] {
        if (!r || !out) throw Error(GS_ERR_INVALID, "null argument");
        HIP_CHECK(hipSetDevice(r->scene->device));
        while (r->pending > 0) {  // retire what has completed, without waiting for what has not
            const hipError_t e = hipEventQuery(r->oldest().done);
            if (e == hipErrorNotReady) break;
            HIP_CHECK(e);
            r->retire_oldest();
        }
        r->latest_stats(out);
        if (frames_retired) *frames_retired = r->lifetime_frames;
    });
}

int gs_get_timing_totals(gs_renderer* r, gs_frame_stats* sum, uint64_t* frames, int reset) {
    return guarded([&] {
        if (!r || !sum || !frames) throw Error(GS_ERR_INVALID, "null argument");
        r->drain();
        *sum = r->last;
        sum->ms_preprocess = static_cast<float>(r->total_ms[0]);
        sum->ms_prefix_sum = static_cast<float>(r->total_ms[1]);
        sum->ms_preprocess_sort = static_cast<float>(r->total_ms[2]);
        sum->ms_sort = static_cast<float>(r->total_ms[3]);
        sum->ms_tile_boundary = static_cast<float>(r->total_ms[4]);
        sum->ms_render = static_cast<float>(r->total_ms[5]);
        sum->ms_total = static_cast<float>(r->total_ms[6]);
        *frames = r->total_frames;
        if (reset) {
            for (double& v : r->total_ms) v = 0.0;
            r->total_frames = 0;
        }
    });
}

int gs_get_frame_intervals(gs_renderer* r, float* out_ms, uint64_t capacity, uint64_t* n_out, int reset) {
    return guarded([&] {
        if (!r || !n_out || (!out_ms && capacity)) throw Error(GS_ERR_INVALID, "null argument");
        r->drain();
        const uint64_t n = std::min<uint64_t>(capacity, r->intervals.size());
        if (n) std::memcpy(out_ms, r->intervals.data() + (r->intervals.size() - n), n * sizeof(float));
        *n_out = r->intervals.size();
        if (reset) {
            r->intervals.clear();
            r->prev_retired = false;
        }
    });
}

int gs_set_sort_path(gs_renderer* r, int mode) {
    return guarded([&] {
        if (!r) throw Error(GS_ERR_INVALID, "renderer is null");
        if (mode < 0 || mode > 2) throw Error(GS_ERR_INVALID, "sort path must be 0 (auto), 1 (global) or 2 (bin-local)");
        r->drain();
        r->policy.set_sort_mode(mode);
    });
}

int gs_set_exp_mode(gs_renderer* r, int mode) {
    return guarded([&] {
        if (!r) throw Error(GS_ERR_INVALID, "renderer is null");
        if (mode < 0 || mode > 3)
            throw Error(GS_ERR_INVALID, "exp mode must be 0 (pipeline polynomial), 1 (hardware v_exp_f32), 2 (libm's expf in binary64) or 3 (guarded v_exp_f32)");
        r->drain();
        r->exp_mode = mode;
    });
}

int gs_set_blend_contraction(gs_renderer* r, int enabled) {
    return guarded([&] {
        if (!r) throw Error(GS_ERR_INVALID, "renderer is null");
        r->drain();
        r->contract = enabled != 0;
    });
}

int gs_set_antialiased(gs_renderer* r, int enabled) {
    return guarded([&] {
        if (!r) throw Error(GS_ERR_INVALID, "renderer is null");
        r->drain();
        r->antialiased = enabled != 0;
    });
}

int gs_get_antialiased(gs_renderer* r) {
    int on = 0;
    const int rc = guarded([&] {
        if (!r) throw Error(GS_ERR_INVALID, "renderer is null");
        on = r->antialiased ? 1 : 0;
    });
    return rc != 0 ? rc : on;
}

int gs_set_blend_lockstep(gs_renderer* r, int mode) {
    return guarded([&] {
        if (!r) throw Error(GS_ERR_INVALID, "null argument");
        if (mode < -1 || mode > 1) throw Error(GS_ERR_INVALID, "blend lockstep: -1 automatic, 0 off, 1 on");
        r->drain();
        r->tuners.pin(mode);
    });
}

int gs_get_blend_lockstep(gs_renderer* r, int* settled) {
    int now = 0;
    const int rc = guarded([&] {
        if (!r) throw Error(GS_ERR_INVALID, "null argument");
        const BlendTuner& t = r->tuners.current();  // (the shape of the most recently enqueued frame)
        now = t.current() ? 1 : 0;
        if (settled) *settled = (t.forced >= 0 || t.phase == 3) ? 1 : 0;
    });
    return rc != 0 ? rc : now;
}

int gs_set_level1_fused(gs_renderer* r, int mode) {
    return guarded([&] {
        if (!r) throw Error(GS_ERR_INVALID, "null argument");
        if (mode < -1 || mode > 1) throw Error(GS_ERR_INVALID, "level-1 fusion: -1 by rule, 0 off, 1 on");
        r->drain();
        r->l1_policy.mode = mode;
    });
}

int gs_get_level1_fused(gs_renderer* r) {
    int on = 0;
    const int rc = guarded([&] {
        if (!r) throw Error(GS_ERR_INVALID, "null argument");
        on = r->enqueued_l1_fused ? 1 : 0;  // (the most recently enqueued frame)
    });
    return rc != 0 ? rc : on;
}

int gs_set_tile_cull(gs_renderer* r, int enabled) {
    return guarded([&] {
        if (!r) throw Error(GS_ERR_INVALID, "null argument");
        r->drain();
        r->tile_cull = enabled != 0;
    });
}

int gs_get_tile_cull(gs_renderer* r, int* last_frame_culled) {
    int on = 0;
    const int rc = guarded([&] {
        if (!r) throw Error(GS_ERR_INVALID, "null argument");
        on = r->tile_cull ? 1 : 0;
        if (last_frame_culled) *last_frame_culled = r->last_frame.set != nullptr && r->last_frame.plan.culled ? 1 : 0;  // (the most recently enqueued frame)
    });
    return rc != 0 ? rc : on;
}

int gs_get_listed_instances(gs_renderer* r, uint64_t* out) {
    return guarded([&] {
        if (!r || !out) throw Error(GS_ERR_INVALID, "null argument");
        r->drain();
        if (!r->has_last_frame()) throw Error(GS_ERR_INVALID, "no frame rendered yet");
        *out = r->last_frame.listed;
    });
}

int gs_set_graph_mode(gs_renderer* r, int enabled) {
    return guarded([&] {
        if (!r) throw Error(GS_ERR_INVALID, "renderer is null");
        r->drain();
        r->graph_mode = enabled != 0;
        if (!r->graph_mode)
            for (auto& fb : r->sets) fb.drop_graph();
    });
}

int gs_debug_download(gs_renderer* r, int stage, void* dst, uint64_t bytes) {
    return guarded([&] {
        if (!r || !dst) throw Error(GS_ERR_INVALID, "null argument");
        r->drain();
        if (!r->has_last_frame()) throw Error(GS_ERR_INVALID, "no frame rendered yet");
        const FrameBuffers& fb = *r->last_frame.set;
        if (stage == GS_STAGE_DEPTH_ORDER && r->last_frame.plan.bin_local())
            throw Error(GS_ERR_INVALID, "the depth-order tap exists only on the global depth-order path (gs_set_sort_path(r, 1))");
        const uint64_t n = r->scene->n;
        const void* src = nullptr;
        uint64_t size = 0;
        switch (stage) {
            case GS_STAGE_TILES: r->rebuild_planes(); src = fb.tiles.p; size = n * 4; break;
            case GS_STAGE_DEPTH: r->rebuild_planes(); src = fb.depth.p; size = n * 4; break;
            case GS_STAGE_AABB: r->rebuild_planes(); src = fb.aabb.p; size = n * 8; break;
            case GS_STAGE_RADIUS:
            case GS_STAGE_CONIC_OPACITY:
            case GS_STAGE_UV_RG:
            case GS_STAGE_B:
            case GS_STAGE_ALPHA_CUT: r->tap_record_field(stage, dst, bytes); return;
            case GS_STAGE_DEPTH_ORDER: src = fb.dvals[1].p; size = static_cast<uint64_t>(r->last.num_visible) * 4; break;
            case GS_STAGE_SORTED_TILE:
            case GS_STAGE_SORTED_GID:
            case GS_STAGE_RANGES:
            case GS_STAGE_LISTS_CULLED:
            case GS_STAGE_RANGES_CULLED: r->tap_lists(stage, dst, bytes); return;
            case GS_STAGE_LISTS_RAW:
            case GS_STAGE_RANGES_RAW:
                {
                    const auto [ranges_src, lists_src] = r->reference_lists();
                    if (stage == GS_STAGE_LISTS_RAW) src = lists_src, size = std::min<uint64_t>(r->last.num_instances, r->capacity) * 4;
                    else src = ranges_src, size = r->last_frame.plan.num_tiles * 8;
                    break;
                }
            default: throw Error(GS_ERR_INVALID, "unknown stage");
        }
        if (bytes < size) throw Error(GS_ERR_INVALID, "destination too small for stage buffer");
        if (size) HIP_CHECK(hipMemcpy(dst, src, size, hipMemcpyDeviceToHost));
    });
}

int gs_accumulate_contributions(gs_renderer* r, const gs_contributions* c) {
    return guarded([&] {
        if (!r || !c) throw Error(GS_ERR_INVALID, "null argument");
        require_aligned(8, {{c->weight, "weight"}});
        require_aligned(4, {{c->pixels, "pixels"}, {c->top_id, "top_id"}});
        r->over_last_frame(!c->weight && !c->pixels && !c->top_id, [&](const gs::TileLists& lists, hipStream_t s) {
            gs::launch_contributions(lists, c->mask, c->weight, c->pixels, c->top_id, s);
        });
    });
}

int gs_blend_features(gs_renderer* r, const gs_feature_maps* m) {
    return guarded([&] {
        if (!r || !m) throw Error(GS_ERR_INVALID, "null argument");
        // (all by the members' values alone: nothing is dereferenced and no device is touched before they pass)
        if (m->channels > GS_FEATURE_CHANNELS_MAX) throw Error(GS_ERR_INVALID, "channels exceeds GS_FEATURE_CHANNELS_MAX (256)");
        if (m->channels > 0 && !m->features) throw Error(GS_ERR_INVALID, "channels > 0 needs features");
        if (m->channels > 0 && !m->out_features) throw Error(GS_ERR_INVALID, "features given without out_features");
        require_aligned(4, {{m->features, "features"}, {m->out_features, "out_features"}, {m->out_alpha, "out_alpha"},
                            {m->out_depth, "out_depth"}, {m->out_depth_median, "out_depth_median"}});
        float* out_features = m->channels > 0 ? m->out_features : nullptr;  // channels == 0: that output is not touched
        r->over_last_frame(!out_features && !m->out_alpha && !m->out_depth && !m->out_depth_median, [&](const gs::TileLists& lists, hipStream_t s) {
            gs::launch_features(lists, m->features, m->channels, out_features, m->out_alpha, m->out_depth, m->out_depth_median, s);
        });
    });
}

int gs_lift_pixels(gs_renderer* r, const gs_pixel_lift* l) {
    return guarded([&] {
        if (!r || !l) throw Error(GS_ERR_INVALID, "null argument");
        // (all by the members' values alone: nothing is dereferenced and no device is touched before they pass)
        if (l->channels > GS_LIFT_CHANNELS_MAX) throw Error(GS_ERR_INVALID, "channels exceeds GS_LIFT_CHANNELS_MAX (256)");
        if (l->channels > 0 && !l->values) throw Error(GS_ERR_INVALID, "channels > 0 needs values");
        if (l->channels > 0 && !l->out) throw Error(GS_ERR_INVALID, "values given without out");
        require_aligned(4, {{l->values, "values"}});
        require_aligned(8, {{l->out, "out"}, {l->out_weight, "out_weight"}});
        double* out = l->channels > 0 ? l->out : nullptr;  // channels == 0: that output is not touched
        r->over_last_frame(!out && !l->out_weight, [&](const gs::TileLists& lists, hipStream_t s) {
            gs::launch_lift(lists, l->mask, l->values, l->channels, out, l->out_weight, s);
        });
    });
}

int gs_blend_backward(gs_renderer* r, const gs_blend_grads* g) {
    return guarded([&] {
        if (!r || !g) throw Error(GS_ERR_INVALID, "null argument");
        // (all by the members' values alone: nothing is dereferenced and no device is touched before they pass)
        const bool asked = g->d_colour || g->d_opacity || g->d_conic || g->d_uv;
        if (asked && !g->grad_rgb) throw Error(GS_ERR_INVALID, "an output is given without grad_rgb");
        require_aligned(4, {{g->grad_rgb, "grad_rgb"}, {g->grad_alpha, "grad_alpha"}});
        require_aligned(8, {{g->d_colour, "d_colour"}, {g->d_opacity, "d_opacity"}, {g->d_conic, "d_conic"}, {g->d_uv, "d_uv"}});
        r->over_last_frame(!asked, [&](const gs::TileLists& lists, hipStream_t s) {
            gs::launch_blend_backward(lists, g->grad_rgb, g->grad_alpha, g->d_colour, g->d_opacity, g->d_conic, g->d_uv, s);
        });
    });
}

int gs_project_backward(gs_renderer* r, const gs_project_grads* g) {
    return guarded([&] {
        if (!r || !g) throw Error(GS_ERR_INVALID, "null argument");
        // (all by the members' values alone: nothing is dereferenced and no device is touched before they pass)
        require_aligned(8, {{g->d_colour, "d_colour"}, {g->d_opacity, "d_opacity"}, {g->d_conic, "d_conic"}, {g->d_uv, "d_uv"},
                            {g->d_means, "d_means"}, {g->d_log_scales, "d_log_scales"}, {g->d_quats, "d_quats"},
                            {g->d_opacity_logits, "d_opacity_logits"}, {g->d_sh_dc, "d_sh_dc"}, {g->d_sh_rest, "d_sh_rest"}});
        const uint32_t k = g->sh_rest_coeffs;
        if (k != 0 && k != 3 && k != 8 && k != 15) throw Error(GS_ERR_INVALID, "sh_rest_coeffs must be 0, 3, 8 or 15");
        if (k != 0 && !g->d_sh_rest) throw Error(GS_ERR_INVALID, "sh_rest_coeffs > 0 needs d_sh_rest");
        const bool asked = g->d_means || g->d_log_scales || g->d_quats || g->d_opacity_logits || g->d_sh_dc || (g->d_sh_rest && k != 0);
        r->over_last_frame(!asked, [&](const gs::TileLists& lists, hipStream_t s) {
            r->rebuild_planes();  // visibility is the tiles tap's answer (a frame of the dense lists or the one-pass level 1 wrote no planes)
            gs::launch_project_backward(r->scene_view(), r->last_frame.set->tiles.p, lists.rec, r->last_frame.u, r->last_frame.antialiased, *g, s);
        });
    });
}

int gs_camera_backward(gs_renderer* r, const gs_camera_grads* g) {
    return guarded([&] {
        if (!r || !g) throw Error(GS_ERR_INVALID, "null argument");
        // (all by the members' values alone: nothing is dereferenced and no device is touched before they pass)
        require_aligned(8, {{g->d_colour, "d_colour"}, {g->d_opacity, "d_opacity"}, {g->d_conic, "d_conic"}, {g->d_uv, "d_uv"},
                            {g->d_view_mat, "d_view_mat"}, {g->d_proj_mat, "d_proj_mat"}, {g->d_camera_position, "d_camera_position"}});
        const bool asked = g->d_view_mat || g->d_proj_mat || g->d_camera_position;
        r->over_last_frame(!asked, [&](const gs::TileLists& lists, hipStream_t s) {
            r->rebuild_planes();  // visibility is the tiles tap's answer, as in gs_project_backward
            r->camera_partials.ensure(gs::camera_backward_partials());
            gs::launch_camera_backward(r->scene_view(), r->last_frame.set->tiles.p, lists.rec, r->last_frame.u, r->last_frame.antialiased, *g,
                                       r->camera_partials.p, s);
        });
    });
}

int gs_photometric_loss(gs_renderer* r, const gs_photo_loss* l) {
    return guarded([&] {
        if (!r || !l) throw Error(GS_ERR_INVALID, "null argument");
        // (all by the members' values alone: nothing is dereferenced and no device is touched before they pass)
        const bool asked = l->terms || l->grad_rgb;
        if (asked && !l->image) throw Error(GS_ERR_INVALID, "an output is given without image");
        if (asked && !l->target) throw Error(GS_ERR_INVALID, "an output is given without target");
        if (l->width < 1 || l->width > GS_PHOTO_LOSS_MAX_EXTENT) throw Error(GS_ERR_INVALID, "width must be 1 .. 16384");
        if (l->height < 1 || l->height > GS_PHOTO_LOSS_MAX_EXTENT) throw Error(GS_ERR_INVALID, "height must be 1 .. 16384");
        if (l->image_stride != 3 && l->image_stride != 4) throw Error(GS_ERR_INVALID, "image_stride must be 3 or 4");
        if (l->target_stride != 3 && l->target_stride != 4) throw Error(GS_ERR_INVALID, "target_stride must be 3 or 4");
        if (!(l->lambda_dssim >= 0.0 && l->lambda_dssim <= 1.0)) throw Error(GS_ERR_INVALID, "lambda_dssim must lie in [0, 1]");
        require_aligned(4, {{l->image, "image"}, {l->target, "target"}, {l->grad_rgb, "grad_rgb"}});
        require_aligned(8, {{l->terms, "terms"}});
        if (!asked) return;
        // Behind queued frames: they retire first, as for the passes over the last frame (an overflowed one is re-run, so `image`
        // may be the target of a gs_render that has not retired).  Nothing of the last frame is read or written from here on.
        r->drain();
        HIP_CHECK(hipSetDevice(r->scene->device));
        if (l->grad_rgb && l->lambda_dssim != 0.0) r->loss_maps.ensure(gs::photo_loss_maps(l->width, l->height));
        r->loss_partials.ensure(gs::photo_loss_partials(l->width, l->height));
        const FrameBuffers& fb = r->sets[0];
        gs::launch_photo_loss(*l, r->loss_maps.p, r->loss_partials.p, fb.stream);
        HIP_CHECK(hipGetLastError());
        fb.sync();
    });
}

int gs_visible_mask(gs_renderer* r, uint8_t* mask, int accumulate) {
    return guarded([&] {
        if (!r || !mask) throw Error(GS_ERR_INVALID, "null argument");
        r->over_last_frame(false, [&](const gs::TileLists&, hipStream_t s) {
            r->rebuild_planes();  // visibility is the tiles tap's answer, as in gs_project_backward
            gs::launch_visible_mask(r->last_frame.set->tiles.p, mask, static_cast<uint32_t>(r->scene->n), accumulate != 0, s);
        });
    });
}

int gs_accumulate_densify_stats(gs_renderer* r, const gs_densify_stats* st) {
    return guarded([&] {
        if (!r || !st) throw Error(GS_ERR_INVALID, "null argument");
        // (all by the members' values alone: nothing is dereferenced and no device is touched before they pass)
        if (!st->d_uv || !st->grad_sum || !st->count || !st->max_radius) throw Error(GS_ERR_INVALID, "null member: d_uv, grad_sum, count and max_radius are all required");
        require_aligned(8, {{st->d_uv, "d_uv"}, {st->grad_sum, "grad_sum"}});
        require_aligned(4, {{st->count, "count"}, {st->max_radius, "max_radius"}});
        r->over_last_frame(false, [&](const gs::TileLists& lists, hipStream_t s) {
            r->rebuild_planes();  // visibility is the tiles tap's answer, as in gs_project_backward
            gs::launch_densify_stats(r->last_frame.set->tiles.p, lists.rec, *st, static_cast<uint32_t>(r->scene->n), lists.width, lists.height, s);
        });
    });
}

void* gs_renderer_stream(gs_renderer* r) { return r ? r->sets[0].stream : nullptr; }

}  // extern "C"
