// gs_contrib.hip -- k_contrib: what every Gaussian contributed to the last frame (gs_accumulate_contributions, gs3d_hip.h).
//
// Part of libgs3d_hip.so (gfx950 only).  Built with -ffp-contract=off, like the blend: every product and sum below is rounded on
// its own.  No kernel of the frame lives here and none is touched: the pass READS the per-tile lists (ranges, sorted_gid) and the
// attribute records the last frame left in HBM and WRITES caller-owned arrays only.
// Reference restated: render.comp:61-89 (the shader gs_blend.hip restates).
#include "gs_device.h"

namespace gs {

// ---------------------------------------------------------------------------------------
// The definition.  A pixel walks its tile's list as render.comp:61-89 does -- `power > 0` skips the entry (:68), `alpha < 1/255`
// skips it (:78, decided on `power` against the record's alpha cut, as every blend mode decides it), `T (1 - alpha) < 1e-4` ends
// the walk (:83) -- always with the REFERENCE's arithmetic, whatever mode the frame was blended in: `power` uncontracted,
// exp = gs_expf_libm.  An entry that reaches :87 is BLENDED at that pixel, with weight w = fl(alpha T) (T as :87 reads it) and
//     q = w 2^24 rounded to the nearest integer, ties to even        (the product is exact; 6 <= q < 2^24)
// Per Gaussian g, over the counted pixels (inside the image, mask != 0) that blend it:  weight[g] += sum q,  pixels[g] += 1;
// per pixel: top_id = the id with the largest w, the earlier list entry on equal w, 0xFFFFFFFF if none or not counted.
// The sums are INTEGERS, so they do not depend on the order in which the adds arrive: two runs give the same bits.
//
// The shape.  One workgroup per tile, one pixel per lane, a wave per 8 x 8 quadrant -- the blend's geometry, so the blend's exact
// quadrant test (gs_device.h: min_q_rect, the same slack) lets a wave skip the entries none of its pixels keeps.  The list is
// taken in chunks of 64 entries STAGED ONCE PER WORKGROUP: waves 0, 1, 2 gather one 16-byte third of the 64 records each (the 48
// bytes the walk reads), wave 3 keeps the chunk's ids and clears the chunk's 64 slots {sum of q, count}; the next chunk's
// records (and the ids of the chunk after it) are loaded into registers while this one is walked.  Per (entry, wave) that some
// counted lane blends -- nothing happens for an empty ballot, the common case -- the wave adds the ballot's population count and
// a 32-bit wave reduction of q (64 x 2^24 = 2^30; the tile's 256 pixels stay below 2^32) to the entry's slot with two LDS
// atomics.  At the chunk's end wave 3 flushes the slots that are not zero: ONE no-return 64-bit and ONE 32-bit device-scope
// atomic add per blended entry and tile -- never an atomic per pixel, never one for an entry nobody blended.
//
// Barriers.  Two per chunk (staged -> walk -> flush), taken by ALL FOUR waves of the tile: a wave whose counted pixels have all
// broken (or that never had one) walks nothing more but stays -- it is a third of the loader -- and says so once in s_done; the
// workgroup leaves the loop together, at the chunk after which s_done reads 4 or at the list's end.  No wave ends early, so no
// barrier waits for a wave that has left (cf. gs_blend.hip's header), and no barrier follows the loop.
// A tile without a counted pixel returns before it reads its range.
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
    __shared__ float4 s_rec[3][WAVE];  // the chunk's {c00 c01 c11 o} {u v r g} {b cut r11 r00}, plane-major
    __shared__ uint32_t s_gid[WAVE], s_sum[WAVE], s_cnt[WAVE];
    __shared__ uint2 s_exptab[32];
    __shared__ uint32_t s_done;        // waves of the tile with no counted pixel left

    const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
    const uint32_t tile = tile_order[blockIdx.x];
    const uint32_t tile_x = tile % tiles_x, tile_y = tile / tiles_x;
    const uint32_t qx0 = tile_x * kTile + (w & 1) * 8, qy0 = tile_y * kTile + (w >> 1) * 8;
    const uint32_t px = qx0 + (lane & 7), py = qy0 + (lane >> 3);
    const bool inside = px < width && py < height;  // render.comp:36-39
    const size_t p = (size_t)py * width + px;
    const bool counted = inside && (mask == nullptr || mask[p] != 0);
    if (tid < 32) {
        const uint64_t v = kExpfTab[tid];
        s_exptab[tid] = make_uint2((uint32_t)v, (uint32_t)(v >> 32));
    }
    if (tid == 0) s_done = 0;
    if (__syncthreads_or(counted) == 0) {  // (also publishes the table and s_done)
        if (top_id && inside) top_id[p] = kContribNone;
        return;
    }
    const float fx = (float)px, fy = (float)py;
    const float rx0 = (float)qx0, ry0 = (float)qy0, rx1 = (float)qx0 + 7.0f, ry1 = (float)qy0 + 7.0f;
    const uint2 range = ranges[tile];
    uint64_t alive = __builtin_amdgcn_ballot_w64(counted);  // counted pixels that have not broken
    if (alive == 0 && lane == 0) atomicAdd(&s_done, 1u);
    float T = 1.0f, best_w = 0.0f;  // (every blended w is > 0)
    uint32_t best_id = kContribNone;

    // software pipeline, as the blend's: ids two chunks ahead, this thread's third of a record one chunk ahead, both in registers
    uint32_t g_nxt = 0, g_next = 0;
    float4 r_nxt = make_float4(0, 0, 0, 0);
    {
        const uint32_t i0 = range.x + (uint32_t)lane;
        if (i0 < range.y) {
            g_nxt = sorted_gid[i0];
            if (w < 3) r_nxt = reinterpret_cast<const float4*>(rec + g_nxt)[w];
        }
        const uint32_t i1 = i0 + WAVE;
        if (i1 < range.y) g_next = sorted_gid[i1];
    }
    for (uint32_t base = range.x; base < range.y; base += WAVE) {
        const uint32_t n_here = range.y - base < (uint32_t)WAVE ? range.y - base : (uint32_t)WAVE;
        const uint32_t g_cur = g_nxt;
        if (w < 3) {
            s_rec[w][lane] = r_nxt;
        } else {
            s_gid[lane] = g_cur;
            s_sum[lane] = 0;
            s_cnt[lane] = 0;
        }
        {
            const uint32_t i1 = base + WAVE + (uint32_t)lane;
            g_nxt = g_next;
            if (i1 < range.y && w < 3) r_nxt = reinterpret_cast<const float4*>(rec + g_nxt)[w];
            const uint32_t i2 = i1 + WAVE;
            if (i2 < range.y) g_next = sorted_gid[i2];
        }
        __syncthreads();  // the chunk is staged, its slots are zero
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
                    const float wgt = upd ? alpha * T : 0.0f;  // w = fl(alpha T)
                    if (upd) {
                        if (wgt > best_w) {  // (strictly: on equal w the earlier entry stays)
                            best_w = wgt;
                            best_id = s_gid[k];
                        }
                        T = test_T;
                    }
                    uint32_t sum = 0;
                    if (weight) sum = wave_sum((uint32_t)__builtin_rintf(wgt * 16777216.0f));  // v_rndne_f32, then an exact conversion
                    if (lane == 0) {
                        atomicAdd(&s_sum[k], sum);
                        atomicAdd(&s_cnt[k], (uint32_t)__popcll(bl));
                    }
                }
                alive &= ~mk;
                if (alive == 0) break;
            }
            if (alive == 0 && lane == 0) atomicAdd(&s_done, 1u);
        }
        __syncthreads();  // the four waves' partials have met in the slots
        if (w == 3) {     // (the wave that holds the chunk's ids and clears the slots for the next chunk)
            const uint32_t c = s_cnt[lane];
            if (c != 0) {
                if (weight) atomicAdd(weight + g_cur, (unsigned long long)s_sum[lane]);
                if (pixels) atomicAdd(pixels + g_cur, c);
            }
        }
        if (s_done == BLOCK / WAVE) break;  // (uniform: nobody writes s_done between this barrier and the next)
    }
    if (top_id && inside) top_id[p] = counted ? best_id : kContribNone;
}

void launch_contributions(const uint32_t* ranges, const uint32_t* sorted_gid, const uint32_t* tile_order, const AttrRecord* rec,
                          uint32_t width, uint32_t height, const uint8_t* mask, uint64_t* weight, uint32_t* pixels, uint32_t* top_id,
                          hipStream_t s) {
    if (width == 0 || height == 0) return;
    const uint32_t tx = (width + kTile - 1) / kTile, ty = (height + kTile - 1) / kTile;
    hipLaunchKernelGGL(k_contrib, dim3(tx * ty), dim3(BLOCK), 0, s, reinterpret_cast<const uint2*>(ranges), sorted_gid, tile_order, rec,
                       width, height, tx, mask, reinterpret_cast<unsigned long long*>(weight), pixels, top_id);
}

}  // namespace gs
