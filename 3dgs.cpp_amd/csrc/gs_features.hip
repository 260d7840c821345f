// gs_features.hip -- k_features: per-pixel maps of the last frame (gs_blend_features, gs3d_hip.h): caller-supplied per-Gaussian
// channels blended the way the colour is, coverage, expected and median depth.
//
// Part of libgs3d_hip.so (gfx950 only).  Built with -ffp-contract=off, like the blend and gs_contrib.hip: every product and sum
// below is rounded on its own.  No kernel of the frame lives here and none is touched: the pass READS the per-tile lists (ranges,
// sorted_gid), the attribute records the last frame left in HBM and the caller's feature rows, and WRITES caller-owned arrays only.
// Reference restated: render.comp:61-89 (the shader gs_blend.hip restates), in gs_tile_walk.h.
#include "gs_tile_walk.h"

namespace gs {

// ---------------------------------------------------------------------------------------
// The definition.  A pixel walks its tile's list as render.comp:61-89 does, always with the REFERENCE's arithmetic (gs_tile_walk.h:
// walk_chunk).  An entry of Gaussian g that reaches :87 adds, with that line's alpha and T (T before :88),
//     F[c] = F[c] + (features[g][c] alpha) T        D = D + (depth[g] alpha) T        (the order of :87)
//     M    = depth[g]   if this is the first blended entry with T (1 - alpha) < 0.5
// T only falls (every blended alpha is >= 1/255), so "M is still unset" is `T >= 0.5` and needs no flag.  At the walk's end the
// pixel writes F, 1 - T, D and M (+inf if unset).  One lane adds one pixel's entries in list order: the outputs are defined bit
// for bit, there are no atomics, and two calls give the same bits.
//
// The shape is the shared walk's (gs_tile_walk.h: tile per workgroup, quadrant per wave, chunks of 64 staged once per workgroup).
// Beside the records, wave 3 stages the chunk's ids and depths (ListPipeline<true>).  There are no LDS slots and no mask:
// `alive` starts from `inside`.
//
// Barriers: the two per chunk of gs_tile_walk.h (staged -> walk -> the next chunk may be staged), taken by all four waves; a wave
// that walks nothing more, or that lies outside the image, stays as a quarter of the loader.
//
// Channel groups.  Every lane keeps T, D, M and G feature sums in registers; G is a template argument, kFeatureGroup = 16 for a
// whole group.  A request of more channels runs ceil(channels / 16) launches on the same stream, each walking the list again
// for its own channels; the first launch, or the channel-less instantiation <0> when channels == 0, also writes alpha and the
// two depths.  Channel sums do not depend on one another, so grouping changes no bit.  The LAST group may be short: 1 .. 4
// channels (RGB, normals, a label, a heat map) run the kernel of exactly that size, <1> .. <4>; 5 .. 15 run <16, FULL = false>,
// which tests every row access against `gc`, the channels that exist, so that nothing past a row's end is read or written (its
// sixteen uniform branches per blended entry cost more than the whole group's one wide fetch: 0.72 ms against 0.55 ms at
// 1920 x 1080 when three channels still ran through it).  The resource report (-Rpass-analysis=kernel-resource-usage) gives
//     k_features<0>           44 VGPRs,  47 SGPRs, no spills, occupancy 8 waves per SIMD
//     k_features<1> .. <4>    45 .. 48,  56 .. 58,            occupancy 8
//     k_features<16, true>    59 VGPRs,  70 SGPRs, no spills, occupancy 8
//     k_features<16, false>   59 VGPRs, 101 SGPRs, no spills, occupancy 7 (the SGPRs of sixteen separate row fetches)
// G = 16 is the largest power of two that keeps the walk at 64 VGPRs or fewer, i.e. at the full eight waves per SIMD -- the walk's own
// state is 44 registers, a group adds one per channel; G = 32 would take about 80 and fall to six waves while halving the
// number of walks, which is the trade to revisit if wide requests (64 channels: four walks, 2.1 ms) matter more than narrow ones.
//
// Feature rows.  The kept entry k of the pair loop is wave-uniform, so its row features + gid channels + c0 is one address for the
// whole wave: it is read as such INSIDE the loop, through readfirstlane(gid), and only for an entry that some lane of the wave
// blends.  The alternative -- staging rows into LDS per chunk -- either moves all 64 rows (on trained-like scenes a quadrant keeps
// one entry in seven, so most of that traffic is wasted) or needs a compaction of the survivors per wave with a third barrier and
// 4 x 64 x G floats of LDS; the uniform fetch moves exactly the rows that are used, needs no barrier, and keeps the barrier
// structure the shared walk's.  Its price is the row's latency in front of the first add; tools/feature_maps_rate.py
// measures it.  A row is only ever ADDED on the lanes that blend the entry: a NaN in the row of a Gaussian nobody blends, or in a
// lane that skipped the entry, reaches no output.
// Stores are plain vector stores; out_features is channel-innermost, so a lane writes its group's consecutive floats.
// ---------------------------------------------------------------------------------------
template <int G, bool FULL>
__global__ __launch_bounds__(BLOCK) void k_features(const uint2* __restrict__ ranges, const uint32_t* __restrict__ sorted_gid,
                                                    const uint32_t* __restrict__ tile_order, const AttrRecord* __restrict__ rec,
                                                    uint32_t width, uint32_t height, uint32_t tiles_x,
                                                    const float* __restrict__ features, uint32_t channels, uint32_t c0, uint32_t gc,
                                                    float* __restrict__ out_features, float* __restrict__ out_alpha,
                                                    float* __restrict__ out_depth, float* __restrict__ out_median) {
    __shared__ float4 s_rec[3][WAVE];  // the chunk's records (gs_tile_walk.h)
    __shared__ uint32_t s_gid[WAVE];
    __shared__ float s_dep[WAVE];
    __shared__ uint2 s_exptab[32];
    __shared__ uint32_t s_done;        // waves of the tile with no pixel left to walk

    const WalkPixel q = walk_pixel(tile_order, width, height, tiles_x);
    const int lane = q.lane, w = q.w;
    walk_init_shared(s_exptab, &s_done);
    __syncthreads();  // the table and s_done are published
    uint64_t alive = walk_begin(q.inside, lane, &s_done);  // pixels that have not broken
    float T = 1.0f, D = 0.0f, M = __uint_as_float(0x7F800000u);
    float F[G > 0 ? G : 1];
#pragma unroll
    for (int c = 0; c < G; ++c) F[c] = 0.0f;

    ListPipeline<true> pipe{sorted_gid, rec, ranges[q.tile], lane, w};  // (wave 3: r_nxt.x = the depth)
    pipe.prime();
    const uint2 range = pipe.range;
    for (uint32_t base = range.x; base < range.y; base += WAVE) {
        const uint32_t n_here = range.y - base < (uint32_t)WAVE ? range.y - base : (uint32_t)WAVE;
        if (w < 3) {
            s_rec[w][lane] = pipe.r_nxt;
        } else {
            s_gid[lane] = pipe.g_nxt;
            s_dep[lane] = pipe.r_nxt.x;
        }
        pipe.advance(base);
        __syncthreads();  // the chunk is staged
        walk_chunk(s_rec, s_exptab, &s_done, q, n_here, alive, T,
                   [&](int k, uint64_t, bool upd, float alpha, float test_T, float& T) {
                       const float dep = s_dep[k];
                       if constexpr (G > 0) {
                           // the entry's row: one address for the wave (k is uniform), read only now that somebody blends it
                           const uint32_t gid = __builtin_amdgcn_readfirstlane(s_gid[k]);
                           const float* __restrict__ row = features + (size_t)gid * channels + c0;
                           float f[G];
#pragma unroll
                           for (int c = 0; c < G; ++c) f[c] = (FULL || (uint32_t)c < gc) ? row[c] : 0.0f;  // (never past the row)
                           if (upd) {
#pragma unroll
                               for (int c = 0; c < G; ++c) F[c] = F[c] + (f[c] * alpha) * T;  // :87
                           }
                       }
                       if (upd) {
                           D = D + (dep * alpha) * T;
                           if (T >= 0.5f && test_T < 0.5f) M = dep;  // the first blended entry that takes T below one half
                           T = test_T;                               // :88
                       }
                   });
        __syncthreads();  // every wave has walked the chunk: it may be overwritten, and s_done is what this chunk left
        if (s_done == BLOCK / WAVE) break;  // (uniform: gs_tile_walk.h, Barriers)
    }
    if (!q.inside) return;  // nothing is written for positions outside the image
    const size_t p = q.p;
    if constexpr (G > 0) {
        float* __restrict__ o = out_features + p * channels + c0;
#pragma unroll
        for (int c = 0; c < G; ++c)
            if (FULL || (uint32_t)c < gc) o[c] = F[c];
    }
    if (out_alpha) out_alpha[p] = 1.0f - T;
    if (out_depth) out_depth[p] = D;
    if (out_median) out_median[p] = M;
}

void launch_features(const TileLists& t, const float* features, uint32_t channels, float* out_features, float* out_alpha,
                     float* out_depth, float* out_median, hipStream_t s) {
    const uint32_t *sorted_gid = t.sorted_gid, *tile_order = t.tile_order, width = t.width, height = t.height;
    const AttrRecord* rec = t.rec;
    if (width == 0 || height == 0) return;
    constexpr int G = kFeatureGroup;
    const uint32_t tx = (width + kTile - 1) / kTile, ty = (height + kTile - 1) / kTile;
    const uint2* rg = reinterpret_cast<const uint2*>(t.ranges);
    if (!out_features) channels = 0;
    if (channels == 0) {
        if (out_alpha || out_depth || out_median)
            hipLaunchKernelGGL((k_features<0, true>), dim3(tx * ty), dim3(BLOCK), 0, s, rg, sorted_gid, tile_order, rec, width, height, tx,
                               nullptr, 0u, 0u, 0u, nullptr, out_alpha, out_depth, out_median);
        return;
    }
    for (uint32_t c0 = 0; c0 < channels; c0 += G) {
        const uint32_t gc = channels - c0 < (uint32_t)G ? channels - c0 : (uint32_t)G;
        // (the first group's launch also writes alpha and the depths)
        float* a = c0 == 0 ? out_alpha : nullptr;
        float* d = c0 == 0 ? out_depth : nullptr;
        float* m = c0 == 0 ? out_median : nullptr;
#define GS_FEATURES_LAUNCH(GROUP, FULL)                                                                                          \
    hipLaunchKernelGGL((k_features<GROUP, FULL>), dim3(tx * ty), dim3(BLOCK), 0, s, rg, sorted_gid, tile_order, rec, width, height, \
                       tx, features, channels, c0, gc, out_features, a, d, m)
        switch (gc) {  // (a last group of 1 .. 4 channels -- RGB, normals, a label, a heat map -- has a kernel of exactly its size)
            case 1: GS_FEATURES_LAUNCH(1, true); break;
            case 2: GS_FEATURES_LAUNCH(2, true); break;
            case 3: GS_FEATURES_LAUNCH(3, true); break;
            case 4: GS_FEATURES_LAUNCH(4, true); break;
            case G: GS_FEATURES_LAUNCH(G, true); break;
            default: GS_FEATURES_LAUNCH(G, false); break;
        }
#undef GS_FEATURES_LAUNCH
    }
}

}  // namespace gs
