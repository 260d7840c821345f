// gs_features.hip -- k_features: per-pixel maps of the last frame (gs_blend_features, gs3d_hip.h): caller-supplied per-Gaussian
// channels blended the way the colour is, coverage, expected and median depth.
//
// Part of libgs3d_hip.so (gfx950 only).  Built with -ffp-contract=off, like the blend and gs_contrib.hip: every product and sum
// below is rounded on its own.  No kernel of the frame lives here and none is touched: the pass READS the per-tile lists (ranges,
// sorted_gid), the attribute records the last frame left in HBM and the caller's feature rows, and WRITES caller-owned arrays only.
// Reference restated: render.comp:61-89 (the shader gs_blend.hip restates).
#include "gs_device.h"

namespace gs {

// ---------------------------------------------------------------------------------------
// The definition.  A pixel walks its tile's list as k_contrib does (gs_contrib.hip; render.comp:61-89): `power > 0` skips the
// entry (:68), `power` below the record's alpha cut skips it (:78), `T (1 - alpha) < 1e-4` ends the walk (:83) -- always with the
// REFERENCE's arithmetic: `power` uncontracted, exp = gs_expf_libm.  An entry of Gaussian g that reaches :87 adds, with that
// line's alpha and T (T before :88),
//     F[c] = F[c] + (features[g][c] alpha) T        D = D + (depth[g] alpha) T        (the order of :87)
//     M    = depth[g]   if this is the first blended entry with T (1 - alpha) < 0.5
// T only falls (every blended alpha is >= 1/255), so "M is still unset" is `T >= 0.5` and needs no flag.  At the walk's end the
// pixel writes F, 1 - T, D and M (+inf if unset).  One lane adds one pixel's entries in list order: the outputs are defined bit
// for bit, there are no atomics, and two calls give the same bits.
//
// The shape is k_contrib's, whose barrier rules are argued there: one workgroup per tile in tile_order, one pixel per lane, a
// wave per 8 x 8 quadrant with the blend's exact quadrant test (gs_device.h: min_q_rect, the same slack); the list in chunks of
// 64 entries STAGED ONCE PER WORKGROUP -- waves 0, 1, 2 gather one 16-byte third of the 64 records each, wave 3 the chunk's ids
// and depths (the first float of a record's fourth 16-byte part) -- with the next chunk's parts (and the ids of the chunk after
// it) loaded into registers while this one is walked.  There are no LDS slots and no mask: `alive` starts from `inside`.
//
// Barriers.  Two per chunk (staged -> walk -> the next chunk may be staged), taken by ALL FOUR waves of the tile: a wave whose
// pixels have all broken (or that lies outside the image) walks nothing more but stays -- it is a quarter of the loader -- and
// says so once in s_done; the workgroup leaves the loop together, at the chunk after which s_done reads 4 or at the list's end.
// No wave ends early, so no barrier waits for a wave that has left, and no barrier follows the loop.
//
// Channel groups.  Every lane keeps T, D, M and G feature sums in registers; G is a template argument, kFeatureGroup = 16 for a
// whole group.  A request of more channels runs ceil(channels / 16) launches on the same stream, each walking the list again
// for its own channels; the first launch, or the channel-less instantiation <0> when channels == 0, also writes alpha and the
// two depths.  Channel sums do not depend on one another, so grouping changes no bit.  The LAST group may be short: 1 .. 4
// channels (RGB, normals, a label, a heat map) run the kernel of exactly that size, <1> .. <4>; 5 .. 15 run <16, FULL = false>,
// which tests every row access against `gc`, the channels that exist, so that nothing past a row's end is read or written (its
// sixteen uniform branches per blended entry cost more than the whole group's one wide fetch: 0.72 ms against 0.55 ms at
// 1920 x 1080 when three channels still ran through it).  The resource report (-Rpass-analysis=kernel-resource-usage) gives
//     k_features<0>           47 VGPRs,  49 SGPRs, no spills, occupancy 8 waves per SIMD
//     k_features<1> .. <4>    48 .. 50,  58 .. 62,            occupancy 8
//     k_features<16, true>    62 VGPRs,  74 SGPRs, no spills, occupancy 8
//     k_features<16, false>   63 VGPRs, 103 SGPRs, no spills, occupancy 7 (the SGPRs of sixteen separate row fetches)
// G = 16 is the largest power of two that keeps the walk at 64 VGPRs or fewer, i.e. at the full eight waves per SIMD -- the walk's own
// state is 47 registers, a group adds one per channel; G = 32 would take about 80 and fall to six waves while halving the
// number of walks, which is the trade to revisit if wide requests (64 channels: four walks, 2.1 ms) matter more than narrow ones.
//
// Feature rows.  The kept entry k of the pair loop is wave-uniform, so its row features + gid channels + c0 is one address for the
// whole wave: it is read as such INSIDE the loop, through readfirstlane(gid), and only for an entry that some lane of the wave
// blends.  The alternative -- staging rows into LDS per chunk -- either moves all 64 rows (on trained-like scenes a quadrant keeps
// one entry in seven, so most of that traffic is wasted) or needs a compaction of the survivors per wave with a third barrier and
// 4 x 64 x G floats of LDS; the uniform fetch moves exactly the rows that are used, needs no barrier, and keeps the barrier
// structure identical to k_contrib's.  Its price is the row's latency in front of the first add; tools/feature_maps_rate.py
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
    __shared__ float4 s_rec[3][WAVE];  // the chunk's {c00 c01 c11 o} {u v r g} {b cut r11 r00}, plane-major
    __shared__ uint32_t s_gid[WAVE];
    __shared__ float s_dep[WAVE];
    __shared__ uint2 s_exptab[32];
    __shared__ uint32_t s_done;        // waves of the tile with no pixel left to walk

    const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
    const uint32_t tile = tile_order[blockIdx.x];
    const uint32_t tile_x = tile % tiles_x, tile_y = tile / tiles_x;
    const uint32_t qx0 = tile_x * kTile + (w & 1) * 8, qy0 = tile_y * kTile + (w >> 1) * 8;
    const uint32_t px = qx0 + (lane & 7), py = qy0 + (lane >> 3);
    const bool inside = px < width && py < height;  // render.comp:36-39
    const size_t p = (size_t)py * width + px;
    if (tid < 32) {
        const uint64_t v = kExpfTab[tid];
        s_exptab[tid] = make_uint2((uint32_t)v, (uint32_t)(v >> 32));
    }
    if (tid == 0) s_done = 0;
    __syncthreads();  // the table and s_done are published
    const float fx = (float)px, fy = (float)py;
    const float rx0 = (float)qx0, ry0 = (float)qy0, rx1 = (float)qx0 + 7.0f, ry1 = (float)qy0 + 7.0f;
    const uint2 range = ranges[tile];
    uint64_t alive = __builtin_amdgcn_ballot_w64(inside);  // pixels that have not broken
    if (alive == 0 && lane == 0) atomicAdd(&s_done, 1u);
    float T = 1.0f, D = 0.0f, M = __uint_as_float(0x7F800000u);
    float F[G > 0 ? G : 1];
#pragma unroll
    for (int c = 0; c < G; ++c) F[c] = 0.0f;

    // software pipeline, as k_contrib's: ids two chunks ahead, this thread's part of a record one chunk ahead, both in registers
    uint32_t g_nxt = 0, g_next = 0;
    float4 r_nxt = make_float4(0, 0, 0, 0);  // (wave 3: .x = the depth)
    {
        const uint32_t i0 = range.x + (uint32_t)lane;
        if (i0 < range.y) {
            g_nxt = sorted_gid[i0];
            if (w < 3) r_nxt = reinterpret_cast<const float4*>(rec + g_nxt)[w];
            else r_nxt.x = rec[g_nxt].depth_radius.x;
        }
        const uint32_t i1 = i0 + WAVE;
        if (i1 < range.y) g_next = sorted_gid[i1];
    }
    for (uint32_t base = range.x; base < range.y; base += WAVE) {
        const uint32_t n_here = range.y - base < (uint32_t)WAVE ? range.y - base : (uint32_t)WAVE;
        if (w < 3) {
            s_rec[w][lane] = r_nxt;
        } else {
            s_gid[lane] = g_nxt;
            s_dep[lane] = r_nxt.x;
        }
        {
            const uint32_t i1 = base + WAVE + (uint32_t)lane;
            g_nxt = g_next;
            if (i1 < range.y) {
                if (w < 3) r_nxt = reinterpret_cast<const float4*>(rec + g_nxt)[w];
                else r_nxt.x = rec[g_nxt].depth_radius.x;
            }
            const uint32_t i2 = i1 + WAVE;
            if (i2 < range.y) g_next = sorted_gid[i2];
        }
        __syncthreads();  // the chunk is staged
        if (alive != 0) {
            // entry `lane` of the chunk against this wave's quadrant: the blend's test (gs_blend.hip, blend_walk), the same slack.
            // An entry it drops is skipped by every pixel of the quadrant (power < cut there), so dropping it changes no bit.
            const float4 co = s_rec[0][lane], uv = s_rec[1][lane], bc = s_rec[2][lane];
            const float cut = bc.y;
            const float h00 = 0.5f * co.x, h11 = 0.5f * co.z;
            uint64_t bm = __builtin_amdgcn_ballot_w64((uint32_t)lane < n_here) & __builtin_amdgcn_ballot_w64(cut <= 0.0f);
            {
                const float mq = min_q_rect(h00, co.y, h11, bc.z, bc.w, uv.x, uv.y, rx0, rx1, ry0, ry1);
                const float ax = fmaxf(fabsf(uv.x - rx0), fabsf(uv.x - rx1));
                const float ay = fmaxf(fabsf(uv.y - ry0), fabsf(uv.y - ry1));
                const float mag = __builtin_fmaf(fabsf(h00) * ax, ax, __builtin_fmaf(fabsf(h11) * ay, ay, fabsf(co.y) * ax * ay));
                bm &= __builtin_amdgcn_ballot_w64(!(mq > __builtin_fmaf(mag, 9.6e-7f, -cut)));  // NaN -> keep
            }
            while (bm) {
                const int k = __ffsll((unsigned long long)bm) - 1;
                bm &= bm - 1;
                const float4 e0 = s_rec[0][k], e1 = s_rec[1][k];
                const float ecut = s_rec[2][k].y;
                const float dx = e1.x - fx, dy = e1.y - fy;
                // :66  -0.5 * (c00 dx dx + c11 dy dy) - c01 dx dy, every product and sum rounded (the scaling by -0.5 is exact)
                const float cx = -0.5f * e0.x, cy = -e0.y, cz = -0.5f * e0.z;
                const float s = cx * dx * dx + cz * dy * dy;
                const float power = s + cy * dx * dy;
                // :68 and :78 (a NaN power skips the entry; power >= cut  <=>  alpha >= 1/255 with the reference's exp)
                const uint64_t m2 = alive & __builtin_amdgcn_ballot_w64(power <= 0.0f) & __builtin_amdgcn_ballot_w64(!(power < ecut));
                if (m2 == 0) continue;
                const float alpha = fminf(0.99f, e0.w * gs_expf_libm(power, s_exptab));  // :77
                const float test_T = T * (1 - alpha);
                const uint64_t mk = m2 & __builtin_amdgcn_ballot_w64(test_T < 0.0001f);  // :82-85 break
                const uint64_t bl = m2 & ~mk;                                            // lanes that reach :87
                if (bl != 0) {
                    const bool upd = __builtin_amdgcn_inverse_ballot_w64(bl);
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
                }
                alive &= ~mk;
                if (alive == 0) break;
            }
            if (alive == 0 && lane == 0) atomicAdd(&s_done, 1u);
        }
        __syncthreads();  // every wave has walked the chunk: it may be overwritten, and s_done is what this chunk left
        if (s_done == BLOCK / WAVE) break;  // (uniform: nobody writes s_done between this barrier and the next)
    }
    if (!inside) return;  // nothing is written for positions outside the image
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

void launch_features(const uint32_t* ranges, const uint32_t* sorted_gid, const uint32_t* tile_order, const AttrRecord* rec,
                     uint32_t width, uint32_t height, const float* features, uint32_t channels, float* out_features, float* out_alpha,
                     float* out_depth, float* out_median, hipStream_t s) {
    if (width == 0 || height == 0) return;
    constexpr int G = kFeatureGroup;
    const uint32_t tx = (width + kTile - 1) / kTile, ty = (height + kTile - 1) / kTile;
    const uint2* rg = reinterpret_cast<const uint2*>(ranges);
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
