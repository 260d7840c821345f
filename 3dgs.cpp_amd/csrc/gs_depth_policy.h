// gs_depth_policy.h -- how a frame's per-tile lists get their depth order, and the bin grid that goes
// with it: which level the next frame runs at, what a frame that overflowed its level asks for, when to step back down.
// Integer arithmetic on two of a frame's counters (`overflow`, `max_bin`).  Plain C++ without a device in sight:
// tests/test_depth_policy.py drives it on the CPU.  tests/limit_scenes.py restates frames_overflowed and the bin geometry in
// Python (predict, base_shift, can_refine) to predict a fresh renderer's stats: a change of the rules here changes them there.
#pragma once

#include <algorithm>
#include <cstdint>

#include "gs_levels.h"

namespace gs_host {

inline uint32_t tiles_across(uint32_t pixels) { return (pixels + gs::kTile - 1) / gs::kTile; }

// The bin grid of a frame: bins of S x S tiles, at most 32 x 32 of them, padded to a 16- or 32-wide grid.
struct BinGeometry {
    int bin_shift, grid_shift;
    uint32_t bins_x, bins_y;
};

// level 0 .. 4: bin-local -- the workgroup that builds a bin's lists orders its candidates in LDS first (up to 4096 / 8192 /
// 12288 / 16384 per bin, or, level 4, up to 65535 in depth slabs of <= 12288; 6 kernels per frame); level 5: global -- the V
// visible Gaussians are ordered first (12 more kernels; any bin size).
// sort_mode 0 = automatic: start at level 0; a bin that does not fit re-runs the frame at the level its size asks for;
// after 32 frames that would have fitted the level below, go back down.
struct DepthPolicy {
    static constexpr int kGlobalLevel = gs::kBinSortLevels;
    static constexpr int kOneSizeShift = 4;  // bins of 2^4 x 2^4 tiles or more: one in-LDS size (16384) at every bin-local level, no slabs
    static uint32_t level_limit(int lv) { return gs::kBinSortLimit[lv]; }

    int sort_mode = 0;  // 0 auto, 1 global depth order, 2 bin-local (forced: a bin beyond 16384 is an error)
    int level = 0;
    uint32_t frames_since_fallback = 0;
    // Depth slabs (level 4) can fail for reasons that have nothing to do with the bin's size -- one depth bucket beyond a slab, a
    // run of more than 65 exactly equal depths inside one (the run's first element counts at most 64 more), more slabs than
    // descriptors: the frame then goes to the global path,
    // and since `max_bin` still fits level 4 the step-down below would send it straight back into the same failure every 32
    // frames, for ever.  Each such failure doubles the frames the renderer stays on the global path before it tries the slabs
    // again (32 .. 8192); 64 clean frames at level 4 reset it.
    uint32_t slab_hold = 32, slab_clean_frames = 0;
    int min_bin_shift = 3;      // log2 of the default bin edge in tiles (8 x 8 tiles)
    bool refined = false;       // bins of half that edge: taken when a bin outgrows the largest in-LDS order
    bool settle_level = false;  // the next clean frame at the level a refinement jumped to tells which level its bins really need

    int frame_level() const { return sort_mode == 1 ? kGlobalLevel : level; }
    // another sort path: the climb starts over (the slab hold and a pending settle outlive it)
    void set_sort_mode(int mode) {
        sort_mode = mode;
        level = 0;
        refined = false;
        frames_since_fallback = 0;
    }

    // ---- the bin grid ----
    static bool grid_fits(uint32_t tx, uint32_t ty, int s) { return (((tx - 1) >> s) + 1) <= 32 && (((ty - 1) >> s) + 1) <= 32; }
    // the coarsest-allowed choice: bins of 8 x 8 tiles (or min_bin_shift), larger only to keep the grid within 32 x 32
    static int base_shift(uint32_t tx, uint32_t ty, int min_shift) {
        int s = std::max(2, min_shift);
        while (!grid_fits(tx, ty, s)) ++s;
        return s;
    }
    // log2 of the bin edge a frame of tx x ty tiles runs with now; beyond 5 the resolution is too large for the binning
    int bin_shift(uint32_t tx, uint32_t ty) const {
        int s = base_shift(tx, ty, min_bin_shift);
        // `refined`: a bin outgrew the largest in-LDS order -> bins of half the edge (a quarter of the candidates or so)
        if (refined && s > 2 && grid_fits(tx, ty, s - 1)) --s;
        return s;
    }
    // false: resolution too large for the tile binning (max 16384 x 16384)
    bool bin_geometry(uint32_t tx, uint32_t ty, BinGeometry* g) const {
        if (base_shift(tx, ty, min_bin_shift) > 5) return false;
        const int s = bin_shift(tx, ty);
        g->bin_shift = s;
        g->bins_x = ((tx - 1) >> s) + 1;
        g->bins_y = ((ty - 1) >> s) + 1;
        g->grid_shift = (g->bins_x <= 16 && g->bins_y <= 16) ? 4 : 5;
        return true;
    }
    bool can_refine(uint32_t width, uint32_t height) const {
        const uint32_t tx = tiles_across(width), ty = tiles_across(height);
        const int s = base_shift(tx, ty, min_bin_shift);
        return !refined && s > 2 && s <= 5 && grid_fits(tx, ty, s - 1);
    }

    // ---- transitions ----
    // One of the frames that were queued when the oldest of them came back with `overflow` set: what it ran with, what it counted.
    struct QueuedFrame {
        int level, bin_shift;
        uint32_t width, height;
        uint32_t overflow;  // bit 1: a bin outgrew the in-LDS order of the frame's level
        uint32_t max_bin;   // candidates in the fullest bin
    };
    // kRerun: run the frames again with the policy's (possibly new) level and bins.  The other two: the forced bin-local mode
    // cannot order this frame (the caller reports the error); what was changed before that was found stays changed.
    enum Verdict { kRerun = 0, kBinTooFull, kDepthsTooCrowded };
    // frames[0] is the oldest queued frame, the one whose overflow was seen
    Verdict frames_overflowed(const QueuedFrame* frames, int count) {
        bool bin_too_big = false;
        uint32_t fullest = 0;
        for (int k = 0; k < count; ++k) {
            const QueuedFrame& q = frames[k];
            // (a frame that ran with another level or bin size than the current ones says nothing about those)
            const bool current = q.level == frame_level() && q.bin_shift == bin_shift(tiles_across(q.width), tiles_across(q.height));
            if (q.level < kGlobalLevel && (q.overflow & 2u) && current) bin_too_big = true;
            if (current) fullest = std::max(fullest, q.max_bin);
        }
        if (!bin_too_big) return kRerun;
        // a bin outgrew the in-LDS order of this level: one level up from here on
        const int failed_level = frames[0].level;
        // bins of 16 x 16 tiles or more are ordered by one kernel at every bin-local level (k_bin_build: 16384 candidates in LDS,
        // whatever the level) and have no slabs: a bin beyond that has nothing to climb to but smaller bins or the global path,
        // and its failure says nothing about the slabs
        const bool one_size = frames[0].bin_shift >= kOneSizeShift;
        const bool slabs_unsuitable = !one_size && failed_level == gs::kBinSlabLevel && fullest <= level_limit(gs::kBinSlabLevel);
        if (slabs_unsuitable) {  // not the bin's size: equal or crowded depths (see slab_hold)
            slab_hold = std::min<uint32_t>(slab_hold * 2, 8192);
            slab_clean_frames = 0;
        }
        int wanted = failed_level + 1;
        while (wanted < kGlobalLevel && fullest > level_limit(wanted)) ++wanted;
        if (one_size) wanted = kGlobalLevel;
        if (wanted >= gs::kBinSlabLevel && can_refine(frames[0].width, frames[0].height)) {  // smaller bins before slabs or the global path
            refined = true;
            wanted = gs::kBinSlabLevel - 1;  // (what the smaller bins hold is not known yet: the largest in-LDS order)
            settle_level = true;
        } else {
            if (sort_mode == 2 && wanted >= kGlobalLevel) return slabs_unsuitable ? kDepthsTooCrowded : kBinTooFull;
            level = std::max(level, wanted);
        }
        if (refined) level = std::max(level, wanted);
        frames_since_fallback = 0;
        return kRerun;
    }

    // a frame that ran at `ran_level` with bins of 2^ran_bin_shift tiles retired without overflow; `max_bin`: the candidates in
    // its fullest bin
    void frame_retired(int ran_level, uint32_t max_bin, int ran_bin_shift = 3) {
        if (ran_level == gs::kBinSlabLevel && ++slab_clean_frames >= 64) slab_hold = 32;  // the slabs work on this scene (again)
        if (settle_level && sort_mode != 1 && ran_level == level && level < kGlobalLevel) {
            // the first clean frame after the bins were refined: its fullest bin says which order the smaller bins need -- straight
            // there instead of 32 frames at the largest one per step down (config C: level 3 -> 2, k_bin_fast<16> -> <12>)
            while (level > 0 && max_bin <= level_limit(level - 1) * 7 / 8) --level;
            frames_since_fallback = 0;
            settle_level = false;
        }
        if (sort_mode != 1 && level > 0) {  // one level down once the bins have fitted it for a while
            // (bins without slabs leave the global path only for what their one kernel holds: frames_overflowed would send a
            // fuller bin straight back, every slab_hold frames, and no longer doubles the hold for it)
            const bool no_slabs_below = level == kGlobalLevel && ran_bin_shift >= kOneSizeShift;
            if (max_bin <= level_limit(no_slabs_below ? gs::kBinSlabLevel - 1 : level - 1) * 7 / 8) {
                // (from the global path back to the slabs: only after slab_hold frames, see there)
                if (++frames_since_fallback >= (level == kGlobalLevel ? slab_hold : 32u)) {
                    --level;
                    frames_since_fallback = 0;
                }
            } else {
                frames_since_fallback = 0;
            }
        } else if (sort_mode != 1 && refined) {  // at the smallest order with the small bins: try the default bins again
            if (max_bin <= level_limit(0) / 2) {  // four times the tiles per bin should still fit level 3 (<= 16384)
                if (++frames_since_fallback >= 32) {
                    refined = false;
                    level = gs::kBinSlabLevel - 1;
                    frames_since_fallback = 0;
                }
            } else {
                frames_since_fallback = 0;
            }
        }
    }
};

// When k_preprocess files the level-1 candidates itself (gs_kernels.h: L1Fused) instead of the three level-1
// kernels.  Every bin owns cap = cand_capacity / on-screen bins records of the candidate buffer; the path costs one device atomic
// per (workgroup, bin the workgroup touches), so it pays where a workgroup's Gaussians are neighbours on the screen too.
struct L1FusedPolicy {
    static constexpr uint32_t kHold = 32;        // frames on the three-kernel path after a bin's region ran over (as slab_hold starts)
    static constexpr uint32_t kGrowCeiling = 4;  // the candidate buffer may grow to this many times its default size for the path
    // Wide splats: E1 / V (bins per visible Gaussian) beyond which the same-address atomics cost more than the launches they replace.
    // profiles/r16_atomic_rate_sparse.txt: a workgroup reserving in k bins adds 1.8 us (k = 8), 7.8 us (k = 16), 25 us (k = 32) to
    // the kernel; the three launches take 24.4 us, so the crossover is k ~ 31 bins per workgroup.  A Morton block of small splats
    // spans ~2 x 2 bins (k = 4.3 at E1 / V = 1.5); splats of m x m bins widen that to ~(m + 1)^2: k = 31 at m = 4.6, E1 / V = 21.
    // The path is left at 8 (k ~ 15, 7 us of atomics): beyond it the gain is within the noise, well short of the crossover.
    static constexpr uint32_t kWideRatio = 8;

    int mode = -1;      // -1 by rule, 0 off, 1 on wherever the frame's structure allows (the hold after an overflow still applies)
    uint32_t hold = 0;  // frames left on the three-kernel path
    // the last retired frame, and its shape
    bool have_last = false;
    uint32_t last_width = 0, last_height = 0, last_max_bin = 0, last_e1 = 0, last_v = 0;
    int last_bin_shift = -1;

    static uint32_t region_cap(uint32_t cand_capacity, uint32_t bins) { return bins ? cand_capacity / bins : 0u; }
    // cap is at least 5/4 of the fullest bin
    static bool cap_suffices(uint32_t cap, uint32_t max_bin) { return 4ull * cap >= 5ull * max_bin; }
    bool knows(uint32_t width, uint32_t height, int bin_shift) const {
        return have_last && width == last_width && height == last_height && bin_shift == last_bin_shift;
    }

    enum Verdict { kEngage = 0, kSwitchedOff, kNotAnyOrder, kDenseRegime, kNoSpatialCopy, kHeld, kCapTooSmall, kWideSplats };
    // any_order: the frame is bin-local with bins of <= 8 x 8 tiles; planes_regime: the scene is below dense_min
    Verdict decide(bool any_order, bool planes_regime, bool spatial_copy, uint32_t width, uint32_t height, int bin_shift,
                   uint32_t cand_capacity, uint32_t bins) const {
        if (mode == 0) return kSwitchedOff;
        if (!any_order) return kNotAnyOrder;
        if (!planes_regime) return kDenseRegime;
        if (hold != 0) return kHeld;
        const uint32_t cap = region_cap(cand_capacity, bins);
        if (cap == 0) return kCapTooSmall;
        if (mode == 1) return kEngage;
        if (!spatial_copy) return kNoSpatialCopy;
        if (knows(width, height, bin_shift)) {  // (no frame of this shape has retired yet: engage, the frame tells)
            if ((uint64_t)last_e1 > (uint64_t)kWideRatio * last_v) return kWideSplats;
            if (!cap_suffices(cap, last_max_bin)) return kCapTooSmall;
        }
        return kEngage;
    }
    // The candidates the buffer should hold for the path to engage, when `cap` alone keeps the frame on the three-kernel path
    // (decide() == kCapTooSmall by rule); 0: leave the buffer alone (nothing to gain, or beyond the ceiling).
    uint32_t grow_to(Verdict v, uint32_t width, uint32_t height, int bin_shift, uint32_t cand_capacity, uint32_t bins,
                     uint32_t default_cand_capacity) const {
        if (v != kCapTooSmall || mode != -1 || !knows(width, height, bin_shift)) return 0;
        const uint64_t cap = ((uint64_t)last_max_bin * 5 + 3) / 4 + last_max_bin / 4;  // 5/4, and as much again as head-room: a moving camera
        const uint64_t want = cap * bins;
        if (want <= cand_capacity || want > (uint64_t)kGrowCeiling * default_cand_capacity) return 0;
        return (uint32_t)want;
    }
    void frame_retired(uint32_t width, uint32_t height, int bin_shift, uint32_t max_bin, uint32_t e1, uint32_t v) {
        if (hold != 0) --hold;
        have_last = true;
        last_width = width, last_height = height, last_bin_shift = bin_shift;
        last_max_bin = max_bin, last_e1 = e1, last_v = v;
    }
    // a frame that ran the one-pass level 1 came back with a region overflow: the queued frames re-run on the three kernels
    void region_overflowed() { hold = kHold; }
};

}  // namespace gs_host
