// gs_contrib.hip -- k_contrib: what every Gaussian contributed to the last frame (gs_accumulate_contributions, gs3d_hip.h).
//
// Part of libgs3d_hip.so (gfx950 only).  Built with -ffp-contract=off, like the blend: every product and sum below is rounded on
// its own.  No kernel of the frame lives here and none is touched: the pass READS the per-tile lists (ranges, sorted_gid) and the
// attribute records the last frame left in HBM and WRITES caller-owned arrays only.
// Reference restated: render.comp:61-89 (the shader gs_blend.hip restates), in gs_tile_walk.h.
#include "gs_tile_walk.h"

namespace gs {

// ---------------------------------------------------------------------------------------
// The definition.  A pixel walks its tile's list as render.comp:61-89 does, always with the REFERENCE's arithmetic, whatever mode
// the frame was blended in (gs_tile_walk.h: walk_chunk).  An entry that reaches :87 is BLENDED at that pixel, with weight
// w = fl(alpha T) (T as :87 reads it) and
//     q = w 2^24 rounded to the nearest integer, ties to even        (the product is exact; 6 <= q < 2^24)
// Per Gaussian g, over the counted pixels (inside the image, mask != 0) that blend it:  weight[g] += sum q,  pixels[g] += 1;
// per pixel: top_id = the id with the largest w, the earlier list entry on equal w, 0xFFFFFFFF if none or not counted.
// The sums are INTEGERS, so they do not depend on the order in which the adds arrive: two runs give the same bits.
//
// The shape is the shared walk's (gs_tile_walk.h: tile per workgroup, quadrant per wave, chunks of 64 staged once per workgroup).
// Beside the records, wave 3 keeps the chunk's ids and clears the chunk's 64 slots {sum of q, count}.  Per (entry, wave) that
// some counted lane blends, the wave adds the ballot's population count and a 32-bit wave reduction of q (64 x 2^24 = 2^30; the
// tile's 256 pixels stay below 2^32) to the entry's slot with two LDS atomics.  At the chunk's end wave 3 flushes the slots that
// are not zero: ONE no-return 64-bit and ONE 32-bit device-scope atomic add per blended entry and tile -- never an atomic per
// pixel, never one for an entry nobody blended.
//
// Barriers: the two per chunk of gs_tile_walk.h (staged -> walk -> flush), taken by all four waves; a wave that walks nothing more
// stays as a third of the loader.  A tile without a counted pixel returns before it reads its range.
// ---------------------------------------------------------------------------------------
constexpr uint32_t kContribNone = 0xFFFFFFFFu;

// Sum of v over the wave's 64 lanes, wave-uniform; every lane must be active.  Four DPP adds make each row of 16 lanes hold its
// own sum (lane ^ 1, lane ^ 2, the half row mirrored, the row mirrored), four v_readlane and three scalar adds join the rows:
// eleven instructions, against six ds_bpermute round trips for the shuffle form (measured at S(1e6), 1920 x 1080: the whole pass
// 0.58 ms against 0.72 ms).
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    int x = (int)v;
    x += __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, false);   // quad_perm [1, 0, 3, 2]
    x += __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xF, 0xF, false);   // quad_perm [2, 3, 0, 1]
    x += __builtin_amdgcn_update_dpp(0, x, 0x141, 0xF, 0xF, false);  // row_half_mirror
    x += __builtin_amdgcn_update_dpp(0, x, 0x140, 0xF, 0xF, false);  // row_mirror
    return (uint32_t)__builtin_amdgcn_readlane(x, 0) + (uint32_t)__builtin_amdgcn_readlane(x, 16) +
           (uint32_t)__builtin_amdgcn_readlane(x, 32) + (uint32_t)__builtin_amdgcn_readlane(x, 48);
}

__global__ __launch_bounds__(BLOCK) void k_contrib(const uint2* __restrict__ ranges, const uint32_t* __restrict__ sorted_gid,
                                                   const uint32_t* __restrict__ tile_order, const AttrRecord* __restrict__ rec,
                                                   uint32_t width, uint32_t height, uint32_t tiles_x, const uint8_t* __restrict__ mask,
                                                   unsigned long long* __restrict__ weight, uint32_t* __restrict__ pixels,
                                                   uint32_t* __restrict__ top_id) {
    __shared__ float4 s_rec[3][WAVE];  // the chunk's records (gs_tile_walk.h)
    __shared__ uint32_t s_gid[WAVE], s_sum[WAVE], s_cnt[WAVE];
    __shared__ uint2 s_exptab[32];
    __shared__ uint32_t s_done;        // waves of the tile with no counted pixel left

    const WalkPixel q = walk_pixel(tile_order, width, height, tiles_x);
    const int lane = q.lane, w = q.w;
    const bool counted = q.inside && (mask == nullptr || mask[q.p] != 0);
    walk_init_shared(s_exptab, &s_done);
    if (__syncthreads_or(counted) == 0) {  // (also publishes the table and s_done)
        if (top_id && q.inside) top_id[q.p] = kContribNone;
        return;
    }
    uint64_t alive = walk_begin(counted, lane, &s_done);  // counted pixels that have not broken
    float T = 1.0f, best_w = 0.0f;  // (every blended w is > 0)
    uint32_t best_id = kContribNone;

    ListPipeline<false> pipe{sorted_gid, rec, ranges[q.tile], lane, w};
    pipe.prime();
    const uint2 range = pipe.range;
    for (uint32_t base = range.x; base < range.y; base += WAVE) {
        const uint32_t n_here = range.y - base < (uint32_t)WAVE ? range.y - base : (uint32_t)WAVE;
        const uint32_t g_cur = pipe.g_nxt;
        if (w < 3) {
            s_rec[w][lane] = pipe.r_nxt;
        } else {
            s_gid[lane] = g_cur;
            s_sum[lane] = 0;
            s_cnt[lane] = 0;
        }
        pipe.advance(base);
        __syncthreads();  // the chunk is staged, its slots are zero
        walk_chunk(s_rec, s_exptab, &s_done, q, n_here, alive, T,
                   [&](int k, uint64_t bl, bool upd, float alpha, float test_T, float& T) {
                       const float wgt = upd ? alpha * T : 0.0f;  // w = fl(alpha T)
                       if (upd) {
                           if (wgt > best_w) {  // (strictly: on equal w the earlier entry stays)
                               best_w = wgt;
                               best_id = s_gid[k];
                           }
                           T = test_T;  // :88
                       }
                       uint32_t sum = 0;
                       if (weight) sum = wave_sum((uint32_t)__builtin_rintf(wgt * 16777216.0f));  // v_rndne_f32, then an exact conversion
                       if (lane == 0) {
                           atomicAdd(&s_sum[k], sum);
                           atomicAdd(&s_cnt[k], (uint32_t)__popcll(bl));
                       }
                   });
        __syncthreads();  // the four waves' partials have met in the slots
        if (w == 3) {     // (the wave that holds the chunk's ids and clears the slots for the next chunk)
            const uint32_t c = s_cnt[lane];
            if (c != 0) {
                if (weight) atomicAdd(weight + g_cur, (unsigned long long)s_sum[lane]);
                if (pixels) atomicAdd(pixels + g_cur, c);
            }
        }
        if (s_done == BLOCK / WAVE) break;  // (uniform: gs_tile_walk.h, Barriers)
    }
    if (top_id && q.inside) top_id[q.p] = counted ? best_id : kContribNone;
}

void launch_contributions(const TileLists& t, const uint8_t* mask, uint64_t* weight, uint32_t* pixels, uint32_t* top_id, hipStream_t s) {
    if (t.width == 0 || t.height == 0) return;
    const uint32_t tx = (t.width + kTile - 1) / kTile, ty = (t.height + kTile - 1) / kTile;
    hipLaunchKernelGGL(k_contrib, dim3(tx * ty), dim3(BLOCK), 0, s, reinterpret_cast<const uint2*>(t.ranges), t.sorted_gid, t.tile_order,
                       t.rec, t.width, t.height, tx, mask, reinterpret_cast<unsigned long long*>(weight), pixels, top_id);
}

}  // namespace gs
