// gs_lift.hip -- k_lift: per-pixel values carried back onto the Gaussians of the last frame (gs_lift_pixels, gs3d_hip.h): the
// transpose of gs_blend_features in its `features` argument, with the weights of gs_accumulate_contributions.
//
// Part of libgs3d_hip.so (gfx950 only).  Built with -ffp-contract=off, like the blend, gs_contrib.hip and gs_features.hip: every
// product and sum below is rounded on its own.  No kernel of the frame lives here and none is touched: the pass READS the per-tile
// lists (ranges, sorted_gid), the attribute records the last frame left in HBM, the caller's mask and values, and ADDS to
// caller-owned arrays only.
// Reference restated: render.comp:61-89 (the shader gs_blend.hip restates), in gs_tile_walk.h.
#include "gs_tile_walk.h"
#include "gs_wave_f64.h"

namespace gs {

// ---------------------------------------------------------------------------------------
// The definition.  A pixel walks its tile's list as render.comp:61-89 does, always with the REFERENCE's arithmetic, whatever mode
// the frame was blended in (gs_tile_walk.h: walk_chunk).  An entry of Gaussian g that reaches :87 at a COUNTED pixel p (inside
// the image, mask NULL or != 0 there) is blended there with w = fl32(alpha T) (T as :87 reads it, before :88), k_contrib's w, and
// contributes
//     out[g][c]     += (double)w * (double)values[p][c]      (the product of two binary32 values is exact in binary64)
//     out_weight[g] += (double)w
// Every add is a binary64 add and the order of the adds is unspecified: the sums are not integers, so two calls need not give the
// same bits; the result is within (n - 1) 2^-53 sum|terms| of the exact sum of its n terms, and bit-exact when a Gaussian gets at
// most two terms into arrays that held zero (a binary64 add is commutative, and x + 0 is x).  A term is SELECTED, never multiplied
// by zero: a NaN at an uncounted pixel (never read), at a pixel outside every list, or in a lane that skipped the entry reaches no
// output.
//
// The shape is the shared walk's (gs_tile_walk.h: tile per workgroup, quadrant per wave, chunks of 64 staged once per workgroup).
// Beside the records, wave 3 keeps the chunk's ids.  A lane loads its own pixel's channels of the launch's group ONCE, before the
// loop, and only if the pixel is counted (in the order lift_reduce wants them, which differs by lane).
//
// The wave's partial.  Per (entry, wave) that some counted lane blends -- nothing happens for an empty ballot, the common case --
// every lane forms its terms t_c = (double)w (double)v[c], with w and v[c] SELECTED to 0 in a lane that does not blend the entry,
// and the wave sums them in binary64 into the entry's LDS slots -- double s_acc[64][G], double s_w[64] -- with ds_add_f64, and
// adds the ballot's population count to s_cnt[64].  The weight is summed with wave_sum's DPP pattern applied to both 32-bit
// halves (wave_sum_f64, gs_wave_f64.h: 23 VALU instructions) and added by lane 0.  Doing the same per channel costs 23 G instructions per
// blended (entry, wave) against the forward's G multiply-adds -- an earlier form of this kernel did, and measured 4.9 ms for 16
// channels at S(1e6), 1920 x 1080, where the forward takes 0.56 ms (HISTORICAL: that code was removed and is not in the tree;
// profiles/pixel_lift_rate_per_channel_dpp.txt keeps its figures) -- so the channels go through a TRANSPOSE-REDUCE instead (lift_reduce, gs_wave_f64.h), which halves
// the live channels at each DPP step and leaves every lane with one channel's sum over its row of 16 lanes; the 64 lanes then
// add to the G slots of the entry with ONE ds_add_f64 (the four rows of the wave meet in the slot).  It is the same set of
// binary64 adds of the same terms in another order, which the definition leaves open.
//
// The flush.  At the chunk's end the slots of the entries whose count is not zero are flushed by the WHOLE workgroup (there are
// 64 G of them): thread i, i + 256, ... takes slot i = entry * G + channel, so ONE no-return device-scope global_atomic_add_f64
// per (blended entry, tile, channel) and one per (blended entry, tile) for the weight -- never an atomic per pixel, never one for
// an entry nobody blended.  The thread that flushes a slot clears it; the thread of channel 0 also flushes and clears s_w and
// s_cnt of its entry.  The G threads of an entry are consecutive lanes of ONE wave (G divides 64), and every one of them reads
// s_cnt[entry] in one instruction at the top, before the channel-0 lane's store to it further down: a wave has one program
// counter and the LDS takes a wave's instructions in order, so no lane can see the cleared count.
//
// Barriers: the two per chunk of gs_tile_walk.h (staged -> walk -> flush), taken by all four waves; a wave that walks nothing more
// stays as a third of the loader and a quarter of the flush.
// What lies between the second barrier of chunk i and the first of chunk i + 1 is the flush of i and the staging of i + 1, by
// different threads with no order between them, so they must not touch the same words:
//   - the flush reads and clears s_acc, s_w, s_cnt, which the staging does not touch (the slots start zero, cleared before the
//     first barrier, and are zero again when their owner has flushed them; the walk of i + 1 adds to them only after barrier
//     one of i + 1, which every flushing thread has reached by then);
//   - the flush reads the chunk's ids, which the staging of i + 1 would overwrite: s_gid is therefore DOUBLE-BUFFERED by the
//     chunk's parity.  Buffer i & 1 is written again by the staging of i + 2, after barrier one of i + 1, i.e. after every
//     thread has finished the flush of i;
//   - the staging writes s_rec, which only the walk reads, between the two barriers of one chunk, as in k_contrib.
// So the two barriers suffice and there is no third.  A tile without a counted pixel returns before it reads its range.
//
// Channel groups.  G = kLiftGroup = 16 channels per launch, one launch per group on the same stream, each walking the lists
// again; the first launch (or the channel-less instantiation <0> when channels == 0) also adds out_weight.  The last group may
// be short: 1 .. 4 channels (a mask, a label, an error, RGB) run the kernel of four, 5 .. 15 the kernel of sixteen, both with
// FULL = false, which tests every row access against `gc`, the channels that exist: nothing past a pixel's row is read (a
// channel that does not exist lifts 0 into a slot nobody flushes), nothing past a Gaussian's row is written.  The resource report
// (-Rpass-analysis=kernel-resource-usage):
//     k_lift<0, true>              45 VGPRs, 58 SGPRs, no spills, no scratch, occupancy 8 waves per SIMD,  4 872 bytes of LDS
//     k_lift<4, true>, <4, false>  53 VGPRs, 60 / 62,  no spills, no scratch, occupancy 8,                 6 920 bytes of LDS
//     k_lift<16, true>, <16, false>  92 VGPRs, 58 / 60, no spills, no scratch, occupancy 5,               13 064 bytes of LDS
// The walk's own state is about 45 registers, the group's values add G, and the binary64 working set of lift_reduce the
// rest: after step A eight doubles are live beside the terms being formed.  (The float-to-double conversions are pinned inside
// the walk: hoisted, sixteen more registers would be held through it.)  Five waves per SIMD for the kernel of sixteen is the
// price of reducing sixteen channels at once -- what runs between two barriers is dependent VALU arithmetic on registers, with the
// sixteen channels' independent chains for the scheduler to interleave -- and it buys 1.33 ms for 16 channels at S(1e6),
// 1920 x 1080 (tools/pixel_lift_rate.py) where the removed per-channel form, at 78 registers and six waves, took 4.88 ms
// (historical, as above: a measurement of code that is no longer here).  G = 8 would
// return to more waves and walk the lists twice as often; the walk alone (<0>) is 0.57 ms.  The LDS allows twelve workgroups
// per CU, more than the registers do.
// ---------------------------------------------------------------------------------------
template <int G, bool FULL>
__global__ __launch_bounds__(BLOCK) void k_lift(const uint2* __restrict__ ranges, const uint32_t* __restrict__ sorted_gid,
                                                const uint32_t* __restrict__ tile_order, const AttrRecord* __restrict__ rec,
                                                uint32_t width, uint32_t height, uint32_t tiles_x, const uint8_t* __restrict__ mask,
                                                const float* __restrict__ values, uint32_t channels, uint32_t c0, uint32_t gc,
                                                double* __restrict__ out, double* __restrict__ out_weight) {
    static_assert(G == 0 || (WAVE % G == 0 && (WAVE * G) % BLOCK == 0), "an entry's G slots are flushed by lanes of one wave");
    __shared__ float4 s_rec[3][WAVE];  // the chunk's records (gs_tile_walk.h)
    __shared__ uint32_t s_gid[2][WAVE], s_cnt[WAVE];
    __shared__ double s_w[WAVE], s_acc[WAVE][G > 0 ? G : 1];
    __shared__ uint2 s_exptab[32];
    __shared__ uint32_t s_done;        // waves of the tile with no counted pixel left

    const WalkPixel q = walk_pixel(tile_order, width, height, tiles_x);
    const int tid = threadIdx.x, lane = q.lane, w = q.w;
    const bool counted = q.inside && (mask == nullptr || mask[q.p] != 0);
    walk_init_shared(s_exptab, &s_done);
    if (tid < WAVE) {
        s_cnt[tid] = 0;
        s_w[tid] = 0.0;
    }
    if constexpr (G > 0) {
#pragma unroll
        for (int j = 0; j < (WAVE * G) / BLOCK; ++j) (&s_acc[0][0])[j * BLOCK + tid] = 0.0;
    }
    if (__syncthreads_or(counted) == 0) return;  // (also publishes the table, the zeroed slots and s_done)
    float v[G > 0 ? G : 1];  // this pixel's channels of the group in lift_channel's order: read only where the pixel is counted
    uint32_t c_mine = 0;     // the channel of the group whose row sum this lane holds after lift_reduce
    if constexpr (G > 0) {
        c_mine = lift_final<G>(lane);
#pragma unroll
        for (int j = 0; j < G; ++j) v[j] = 0.0f;
        if (counted) {
            const float* __restrict__ row = values + q.p * channels + c0;
#pragma unroll
            for (int j = 0; j < G; ++j) {
                const uint32_t c = lift_channel<G>(j, lane);
                if (FULL || c < gc) v[j] = row[c];  // (never past the row; a channel that does not exist lifts 0)
            }
        }
    }
    uint64_t alive = walk_begin(counted, lane, &s_done);  // counted pixels that have not broken
    float T = 1.0f;

    ListPipeline<false> pipe{sorted_gid, rec, ranges[q.tile], lane, w};
    pipe.prime();
    const uint2 range = pipe.range;
    int par = 0;  // the chunk's parity: which half of s_gid holds its ids
    for (uint32_t base = range.x; base < range.y; base += WAVE, par ^= 1) {
        const uint32_t n_here = range.y - base < (uint32_t)WAVE ? range.y - base : (uint32_t)WAVE;
        if (w < 3) s_rec[w][lane] = pipe.r_nxt;
        else s_gid[par][lane] = pipe.g_nxt;
        pipe.advance(base);
        __syncthreads();  // the chunk is staged, its slots are zero
        walk_chunk(s_rec, s_exptab, &s_done, q, n_here, alive, T,
                   [&](int k, uint64_t bl, bool upd, float alpha, float test_T, float& T) {
                       const double wd = upd ? (double)(alpha * T) : 0.0;  // w = fl(alpha T), exactly; selected
                       if (upd) T = test_T;                                // :88
                       if (out_weight) {
                           const double sum = wave_sum_f64(wd);
                           if (lane == 0) atomicAdd(&s_w[k], sum);
                       }
                       if constexpr (G > 0) {
                           const double sum = lift_reduce<G>(v, wd, upd);  // channel c_mine over this lane's row of 16
                           if (G == 16 || (lane & 12) == 0) atomicAdd(&s_acc[k][c_mine], sum);  // (G = 4: a row's quads hold the same sums)
                       }
                       if (lane == 0) atomicAdd(&s_cnt[k], (uint32_t)__popcll(bl));
                   });
        __syncthreads();  // the four waves' partials have met in the slots
        if constexpr (G > 0) {
#pragma unroll
            for (int j = 0; j < (WAVE * G) / BLOCK; ++j) {
                const int i = j * BLOCK + tid, e = i / G, c = i % G;
                if (s_cnt[e] != 0) {  // (read by the entry's G lanes at once, before lane c == 0 clears it below)
                    const uint32_t gid = s_gid[par][e];
                    if (FULL || (uint32_t)c < gc) atomicAdd(out + (size_t)gid * channels + c0 + c, s_acc[e][c]);
                    s_acc[e][c] = 0.0;
                    if (c == 0) {
                        if (out_weight) atomicAdd(out_weight + gid, s_w[e]);
                        s_w[e] = 0.0;
                        s_cnt[e] = 0;
                    }
                }
            }
        } else {
            if (tid < WAVE && s_cnt[tid] != 0) {
                atomicAdd(out_weight + s_gid[par][tid], s_w[tid]);  // (<0> is launched only with out_weight)
                s_w[tid] = 0.0;
                s_cnt[tid] = 0;
            }
        }
        if (s_done == BLOCK / WAVE) break;  // (uniform: gs_tile_walk.h, Barriers)
    }
}

void launch_lift(const TileLists& t, const uint8_t* mask, const float* values, uint32_t channels, double* out, double* out_weight,
                 hipStream_t s) {
    const uint32_t *sorted_gid = t.sorted_gid, *tile_order = t.tile_order, width = t.width, height = t.height;
    const AttrRecord* rec = t.rec;
    if (width == 0 || height == 0) return;
    constexpr int G = kLiftGroup;
    const uint32_t tx = (width + kTile - 1) / kTile, ty = (height + kTile - 1) / kTile;
    const uint2* rg = reinterpret_cast<const uint2*>(t.ranges);
    if (!out) channels = 0;
    if (channels == 0) {
        if (out_weight)
            hipLaunchKernelGGL((k_lift<0, true>), dim3(tx * ty), dim3(BLOCK), 0, s, rg, sorted_gid, tile_order, rec, width, height, tx,
                               mask, nullptr, 0u, 0u, 0u, nullptr, out_weight);
        return;
    }
    for (uint32_t c0 = 0; c0 < channels; c0 += G) {
        const uint32_t gc = channels - c0 < (uint32_t)G ? channels - c0 : (uint32_t)G;
        double* ow = c0 == 0 ? out_weight : nullptr;  // (the first group's launch also adds the weights)
#define GS_LIFT_LAUNCH(GROUP, FULL)                                                                                              \
    hipLaunchKernelGGL((k_lift<GROUP, FULL>), dim3(tx * ty), dim3(BLOCK), 0, s, rg, sorted_gid, tile_order, rec, width, height, tx, \
                       mask, values, channels, c0, gc, out, ow)
        // (a last group of 1 .. 4 channels -- a mask, a label, an error, RGB -- runs the small kernel)
        if (gc == (uint32_t)G) GS_LIFT_LAUNCH(G, true);
        else if (gc > (uint32_t)kLiftGroupSmall) GS_LIFT_LAUNCH(G, false);
        else if (gc == (uint32_t)kLiftGroupSmall) GS_LIFT_LAUNCH(kLiftGroupSmall, true);
        else GS_LIFT_LAUNCH(kLiftGroupSmall, false);
#undef GS_LIFT_LAUNCH
    }
}

}  // namespace gs
