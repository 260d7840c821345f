// gs_host::DepthPolicy behind a C interface: tests/test_depth_policy.py plays the renderer -- it hands the policy the counters
// of frames that overflowed or retired and reads back the level, the bins and the hold counters.
// Built by that test with g++; nothing here touches a GPU.
#include <cstdint>
#include <vector>

#include "gs_depth_policy.h"

using gs_host::DepthPolicy;

extern "C" {

void* dp_new(int sort_mode, int min_bin_shift) {
    DepthPolicy* p = new DepthPolicy;
    p->sort_mode = sort_mode;
    p->min_bin_shift = min_bin_shift;
    return p;
}
void dp_free(void* h) { delete static_cast<DepthPolicy*>(h); }

// state[8]: sort_mode, level, refined, settle_level, frames_since_fallback, slab_hold, slab_clean_frames, min_bin_shift
void dp_get(void* h, int64_t* state) {
    const DepthPolicy& p = *static_cast<DepthPolicy*>(h);
    const int64_t v[8] = {p.sort_mode, p.level, p.refined, p.settle_level, p.frames_since_fallback, p.slab_hold, p.slab_clean_frames, p.min_bin_shift};
    for (int i = 0; i < 8; ++i) state[i] = v[i];
}
void dp_set(void* h, const int64_t* state) {
    DepthPolicy& p = *static_cast<DepthPolicy*>(h);
    p.sort_mode = static_cast<int>(state[0]);
    p.level = static_cast<int>(state[1]);
    p.refined = state[2] != 0;
    p.settle_level = state[3] != 0;
    p.frames_since_fallback = static_cast<uint32_t>(state[4]);
    p.slab_hold = static_cast<uint32_t>(state[5]);
    p.slab_clean_frames = static_cast<uint32_t>(state[6]);
    p.min_bin_shift = static_cast<int>(state[7]);
}
void dp_set_sort_mode(void* h, int mode) { static_cast<DepthPolicy*>(h)->set_sort_mode(mode); }
int dp_frame_level(void* h) { return static_cast<DepthPolicy*>(h)->frame_level(); }

// the grid of a width x height frame: geo[4] = bin_shift, bins_x, bins_y, grid_shift; returns 0 for "resolution too large"
int dp_geometry(void* h, uint32_t width, uint32_t height, int* geo) {
    gs_host::BinGeometry g{};
    if (!static_cast<DepthPolicy*>(h)->bin_geometry(gs_host::tiles_across(width), gs_host::tiles_across(height), &g)) return 0;
    geo[0] = g.bin_shift;
    geo[1] = static_cast<int>(g.bins_x);
    geo[2] = static_cast<int>(g.bins_y);
    geo[3] = g.grid_shift;
    return 1;
}
int dp_can_refine(void* h, uint32_t width, uint32_t height) { return static_cast<DepthPolicy*>(h)->can_refine(width, height) ? 1 : 0; }

// frames: 6 words per queued frame (level, bin_shift, width, height, overflow, max_bin), oldest first; returns the Verdict
int dp_overflowed(void* h, const uint32_t* frames, int count) {
    std::vector<DepthPolicy::QueuedFrame> q;
    for (int k = 0; k < count; ++k) {
        const uint32_t* f = frames + 6 * k;
        q.push_back({static_cast<int>(f[0]), static_cast<int>(f[1]), f[2], f[3], f[4], f[5]});
    }
    return static_cast<int>(static_cast<DepthPolicy*>(h)->frames_overflowed(q.data(), count));
}
void dp_retired(void* h, int ran_level, uint32_t max_bin) { static_cast<DepthPolicy*>(h)->frame_retired(ran_level, max_bin); }
// the same for a frame that ran with bins of 2^bin_shift tiles (the renderer always says which)
void dp_retired_at(void* h, int ran_level, uint32_t max_bin, int bin_shift) {
    static_cast<DepthPolicy*>(h)->frame_retired(ran_level, max_bin, bin_shift);
}

int dp_verdict(int which) {  // 0 re-run, 1 "holds more candidates", 2 "too crowded"
    const DepthPolicy::Verdict v[3] = {DepthPolicy::kRerun, DepthPolicy::kBinTooFull, DepthPolicy::kDepthsTooCrowded};
    return static_cast<int>(v[which]);
}
int dp_limit(int level) { return static_cast<int>(DepthPolicy::level_limit(level)); }

}  // extern "C"
