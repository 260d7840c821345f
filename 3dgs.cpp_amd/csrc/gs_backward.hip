// gs_backward.hip -- k_blend_backward: the screen-space gradients of the last frame per Gaussian (gs_blend_backward, gs3d_hip.h):
// dL/d(colour, opacity, conic, uv) from dL/d(image RGB) and dL/d(out_alpha), the backward of the blend of render.comp:61-89.
//
// Part of libgs3d_hip.so (gfx950 only).  Built with -ffp-contract=off, like the blend, gs_contrib.hip, gs_features.hip and
// gs_lift.hip: every product and sum below is rounded on its own.  No kernel of the frame lives here and none is touched: the pass
// READS the per-tile lists (ranges, sorted_gid), the attribute records the last frame left in HBM and the caller's two gradient
// maps, and ADDS to caller-owned arrays only.
// Reference restated: render.comp:61-89 (the shader gs_blend.hip restates), in gs_tile_walk.h.
#include "gs_tile_walk.h"
#include "gs_wave_f64.h"

namespace gs {

// ---------------------------------------------------------------------------------------
// The definition is gs3d_hip.h's (gs_blend_backward); in short, for the blended entries i = 1 .. L of a pixel, in list order, with
// the binary32 alpha_i, T_i (before :88), prod_i = fl32(o e_i), dx_i, dy_i, m_i = fl32(1 - alpha_i) of the walk, T_f the pixel's
// final T, G = grad_rgb[p], ga = grad_alpha[p] or 0, and everything below in binary64 on exact conversions of those:
//     a_i = G_r r + G_g g + G_b b      w_i = (double)fl32(alpha_i T_i)      R_i = sum over j > i of a_j w_j
//     d_colour[g] += w_i G                                      (gs_lift_pixels of grad_rgb)
//     galpha_i = T_i a_i - (R_i - ga T_f) / m_i
//     where prod_i <= 0.99f (alpha is not the clamp; false for a NaN product):
//         d_opacity[g] += galpha_i e_i                          gp = galpha_i alpha_i
//         d_conic[g]   += gp (-0.5 dx^2, -dx dy, -0.5 dy^2)     d_uv[g] += gp (-(c00 dx + c01 dy), -(c01 dx + c11 dy))
// The decisions of the walk are constants.  A term is SELECTED, never multiplied by zero, so a NaN gradient at a pixel reaches only
// the Gaussians blended there.
//
// Two walks in one launch.  R_i needs what lies BEHIND entry i and the walker goes front to back, so the kernel walks the tile's
// list twice (GEOM; with d_colour alone, one walk and no R):
//   walk 1  per lane R_tot = sum of a_j w_j in binary64, and T_f, the T the walk ends with (a break at :83 leaves it as it was);
//   walk 2  carries the prefix P_i = sum over j <= i, forms R_i = R_tot - P_i and emits the nine terms.
// Both walks form a_j w_j with the SAME expression (bwd_a times the converted fl32(alpha T), in that order, uncontracted), so the
// summands of R_tot and of P_i are the same binary64 values: R_i differs from the exact suffix sum of those values only by the
// roundings of the L - 1 + i adds and the subtraction, at most (2 L - 1) 2^-53 sum |a_j| w_j -- what tests/backward_reference.py
// budgets for.  Both walks take the same decisions: walk_chunk's are functions of the records and the pixel alone.
//
// Barriers.  Each walk is the loop of gs_tile_walk.h: two barriers per chunk, taken by all four waves, and the uniform exit on its
// s_done word after the second.  The two walks have ONE WORD EACH, s_done[0] and s_done[1], both zeroed before the kernel's first
// barrier: walk 2 never writes the word that a slower wave may still be testing at the exit of walk 1, and walk 2's word is written
// only by walk_begin (before walk 2's first barrier) and between the barriers of its chunks, read only after a second barrier: the
// rule of gs_tile_walk.h, once per walk.  Nothing else crosses from walk 1 to walk 2 through LDS -- R_tot and T_f are the lane's
// own registers -- and s_rec is restaged for walk 2's first chunk only by threads that have left walk 1's loop, i.e. after the
// second barrier of its last walked chunk, behind which no wave reads s_rec: so NO barrier stands between the walks.  The pipeline
// is primed again (ids and records of the first two chunks: L2 hits), alive and T start over.
//
// The reduce is k_lift's (gs_lift.hip): per (entry, wave) that some lane blends, the lane's terms, selected to 0 where the lane
// does not blend the entry (or, for the six that flow through alpha, where alpha is the clamp), go through a binary64
// transpose-reduce (gs_wave_f64.h) into the entry's LDS slots, s_acc[64][16], with ds_add_f64: the colour as lift_reduce<4> of
// G (r, g, b, 0: slots 0 .. 3), {opacity, conic} as row_reduce4_f64 (slots 4 .. 7), uv as row_reduce2_f64 (slots 8, 9; 10 .. 15
// are never touched: sixteen slots so that an entry's flushing threads are lanes of one wave).  s_flag[entry] gets bit 0 when some
// lane blends the entry and bit 1 when one of those pairs flows through alpha.  At the chunk's end the WHOLE workgroup flushes:
// thread i, i + 256, .. takes slot i = entry * 16 + component: one no-return global_atomic_add_f64 per (blended entry, tile,
// component); colour needs bit 0, the other six bit 1 -- a Gaussian whose every pair is clamped gets no add at all to d_opacity,
// d_conic, d_uv, not an add of zero -- and a NULL output is not flushed.  The flusher clears its slot, component 0's thread the
// flag; the sixteen threads of an entry are consecutive lanes of one wave and read the flag in one instruction before that store.
// s_gid is double-buffered by the chunk's parity for the reason gs_lift.hip gives: the flush of chunk i runs beside the staging of
// chunk i + 1.
//
// A tile with an empty range returns before it reads anything else; so does one with no pixel inside the image, before it reads
// a gradient or a record.  The gradients of a pixel are read once, before the walks, only inside the image.
//
// The resource report (-Rpass-analysis=kernel-resource-usage), all nine components in one launch:
//     k_blend_backward<true>   93 VGPRs, 80 SGPRs, no spills, no scratch, occupancy 5 waves per SIMD, 12 552 bytes of LDS
//     k_blend_backward<false>  61 VGPRs, 70 SGPRs, no spills, no scratch, occupancy 8,                  12 552 bytes of LDS
// The walk's own state is about 45 registers (k_lift<0>); R_tot, the prefix and ga T_f are six more, the six binary64 terms
// and what they are formed from the rest.  Five waves per SIMD is k_lift<16>'s occupancy; the LDS allows twelve workgroups per CU.
// Nothing had to be split into two launches.
// ---------------------------------------------------------------------------------------
constexpr int kBwdSlots = 16;  // LDS slots per entry: 0 .. 2 colour, 4 opacity, 5 .. 7 conic, 8 .. 9 uv

// a = G_r r + G_g g + G_b b: three exact products, two rounded adds.  The ONE expression both walks use.
__device__ __forceinline__ double bwd_a(const float (&g)[3], float r, float gr, float b) {
    return ((double)g[0] * (double)r + (double)g[1] * (double)gr) + (double)g[2] * (double)b;
}

template <bool GEOM>
__global__ __launch_bounds__(BLOCK) void k_blend_backward(const uint2* __restrict__ ranges, const uint32_t* __restrict__ sorted_gid,
                                                          const uint32_t* __restrict__ tile_order, const AttrRecord* __restrict__ rec,
                                                          uint32_t width, uint32_t height, uint32_t tiles_x,
                                                          const float* __restrict__ grad_rgb, const float* __restrict__ grad_alpha,
                                                          double* __restrict__ d_colour, double* __restrict__ d_opacity,
                                                          double* __restrict__ d_conic, double* __restrict__ d_uv) {
    __shared__ float4 s_rec[3][WAVE];  // the chunk's records (gs_tile_walk.h)
    __shared__ uint32_t s_gid[2][WAVE], s_flag[WAVE];
    __shared__ double s_acc[WAVE][kBwdSlots];
    __shared__ uint2 s_exptab[32];
    __shared__ uint32_t s_done[2];     // per walk: waves of the tile with no pixel left to walk

    const WalkPixel q = walk_pixel(tile_order, width, height, tiles_x);
    const int tid = threadIdx.x, lane = q.lane, w = q.w;
    const uint2 range = ranges[q.tile];
    if (range.x >= range.y) return;  // (uniform: nothing to blend, nothing is read)
    walk_init_shared(s_exptab, &s_done[0]);
    if (tid == 0) s_done[1] = 0;
    if (tid < WAVE) s_flag[tid] = 0;
#pragma unroll
    for (int j = 0; j < (WAVE * kBwdSlots) / BLOCK; ++j) (&s_acc[0][0])[j * BLOCK + tid] = 0.0;
    if (__syncthreads_or(q.inside) == 0) return;  // (also publishes the table, the zeroed slots and both s_done words)

    float g[3] = {0.0f, 0.0f, 0.0f}, ga = 0.0f;  // this pixel's gradients: read only inside the image
    if (q.inside) {
        g[0] = grad_rgb[q.p * 3 + 0];
        g[1] = grad_rgb[q.p * 3 + 1];
        g[2] = grad_rgb[q.p * 3 + 2];
        if (GEOM && grad_alpha) ga = grad_alpha[q.p];
    }
    float v[4];  // G in lift_channel<4>'s order, channel 3 = 0: the colour's terms are lift_reduce<4>'s
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t c = lift_channel<4>(j, lane);
        v[j] = c == 0 ? g[0] : c == 1 ? g[1] : c == 2 ? g[2] : 0.0f;
    }
    const uint32_t c_mine = lift_final<4>(lane);

    ListPipeline<false> pipe{sorted_gid, rec, range, lane, w};
    double R_tot = 0.0, gaTf = 0.0;
    if constexpr (GEOM) {
        // ---- walk 1: R_tot and T_f
        uint64_t alive = walk_begin(q.inside, lane, &s_done[0]);
        float T = 1.0f;
        pipe.prime();
        for (uint32_t base = range.x; base < range.y; base += WAVE) {
            const uint32_t n_here = range.y - base < (uint32_t)WAVE ? range.y - base : (uint32_t)WAVE;
            if (w < 3) s_rec[w][lane] = pipe.r_nxt;
            pipe.advance(base);
            __syncthreads();  // the chunk is staged
            walk_chunk(s_rec, s_exptab, &s_done[0], q, n_here, alive, T,
                       [&](int k, uint64_t bl, bool upd, float alpha, float test_T, float& T) {
                           const float4 e1 = s_rec[1][k];
                           const double aw = bwd_a(g, e1.z, e1.w, s_rec[2][k].x) * (double)(alpha * T);
                           if (upd) {
                               R_tot = R_tot + aw;
                               T = test_T;  // :88
                           }
                       });
            __syncthreads();  // every wave has walked the chunk and said in s_done[0] whether it walks on
            if (s_done[0] == BLOCK / WAVE) break;  // (uniform: gs_tile_walk.h, Barriers)
        }
        gaTf = (double)ga * (double)T;  // ga T_f, exact
    }

    // ---- walk 2 (the only one without GEOM): the terms
    uint64_t alive = walk_begin(q.inside, lane, &s_done[1]);
    float T = 1.0f;
    double prefix = 0.0;
    pipe.prime();
    int par = 0;  // the chunk's parity: which half of s_gid holds its ids
    for (uint32_t base = range.x; base < range.y; base += WAVE, par ^= 1) {
        const uint32_t n_here = range.y - base < (uint32_t)WAVE ? range.y - base : (uint32_t)WAVE;
        if (w < 3) s_rec[w][lane] = pipe.r_nxt;
        else s_gid[par][lane] = pipe.g_nxt;
        pipe.advance(base);
        __syncthreads();  // the chunk is staged, its slots are zero
        walk_chunk(s_rec, s_exptab, &s_done[1], q, n_here, alive, T,
                   [&](int k, uint64_t bl, bool upd, float alpha, float test_T, float& T) {
                       const float4 e0 = s_rec[0][k], e1 = s_rec[1][k];
                       const double wd = (double)(alpha * T);  // w = fl(alpha T), exactly
                       uint32_t flag = 1;
                       if constexpr (GEOM) {
                           // :66 and :77 once more, with walk_chunk's expressions: the same bits
                           const float dx = e1.x - q.fx, dy = e1.y - q.fy;
                           const float cx = -0.5f * e0.x, cy = -e0.y, cz = -0.5f * e0.z;
                           const float s = cx * dx * dx + cz * dy * dy;
                           const float power = s + cy * dx * dy;
                           const float e = gs_expf_libm(power, s_exptab);
                           const bool flows = upd && (e0.w * e <= 0.99f);  // alpha is the product, not the clamp (NaN: false)
                           const double a = bwd_a(g, e1.z, e1.w, s_rec[2][k].x);
                           const double aw = a * wd;
                           if (upd) prefix = prefix + aw;
                           const double R = R_tot - prefix;
                           const double galpha = (double)T * a - (R - gaTf) / (double)(1 - alpha);
                           const double gp = galpha * (double)alpha;
                           const double dxd = (double)dx, dyd = (double)dy;
                           const double c00 = (double)e0.x, c01 = (double)e0.y, c11 = (double)e0.z;
                           double t[4] = {galpha * (double)e, gp * (-0.5 * (dxd * dxd)), gp * -(dxd * dyd), gp * (-0.5 * (dyd * dyd))};
                           double u0 = gp * -(c00 * dxd + c01 * dyd), u1 = gp * -(c01 * dxd + c11 * dyd);
#pragma unroll
                           for (int j = 0; j < 4; ++j) t[j] = flows ? t[j] : 0.0;  // selected, never multiplied
                           u0 = flows ? u0 : 0.0;
                           u1 = flows ? u1 : 0.0;
                           if (d_opacity || d_conic) {
                               const double sum = row_reduce4_f64(t, lane);
                               if ((lane & 12) == 0) atomicAdd(&s_acc[k][4 + c_mine], sum);  // (a row's quads hold the same sums)
                           }
                           if (d_uv) {
                               const double sum = row_reduce2_f64(u0, u1, lane);
                               if ((lane & 14) == 0) atomicAdd(&s_acc[k][8 + (lane & 1)], sum);
                           }
                           if (__builtin_amdgcn_ballot_w64(flows) != 0) flag = 3;
                       }
                       if (upd) T = test_T;  // :88
                       if (d_colour) {
                           const double sum = lift_reduce<4>(v, upd ? wd : 0.0, upd);  // channel c_mine over this lane's row of 16
                           if ((lane & 12) == 0) atomicAdd(&s_acc[k][c_mine], sum);
                       }
                       if (lane == 0) atomicOr(&s_flag[k], flag);
                   });
        __syncthreads();  // the four waves' partials have met in the slots
#pragma unroll
        for (int j = 0; j < (WAVE * kBwdSlots) / BLOCK; ++j) {
            const int i = j * BLOCK + tid, e = i / kBwdSlots, c = i % kBwdSlots;
            const uint32_t flag = s_flag[e];  // (read by the entry's 16 lanes at once, before lane c == 0 clears it below)
            if (flag != 0 && c < 10) {
                const size_t gid = s_gid[par][e];
                double* dst = nullptr;
                if (c < 3) dst = d_colour ? d_colour + gid * 3 + c : nullptr;
                else if ((flag & 2) == 0 || c == 3) dst = nullptr;
                else if (c == 4) dst = d_opacity ? d_opacity + gid : nullptr;
                else if (c < 8) dst = d_conic ? d_conic + gid * 3 + (c - 5) : nullptr;
                else dst = d_uv ? d_uv + gid * 2 + (c - 8) : nullptr;
                if (dst) atomicAdd(dst, s_acc[e][c]);
                s_acc[e][c] = 0.0;
                if (c == 0) s_flag[e] = 0;
            }
        }
        if (s_done[1] == BLOCK / WAVE) break;  // (uniform: gs_tile_walk.h, Barriers)
    }
}

void launch_blend_backward(const TileLists& t, const float* grad_rgb, const float* grad_alpha, double* d_colour, double* d_opacity,
                           double* d_conic, double* d_uv, hipStream_t s) {
    const uint32_t width = t.width, height = t.height;
    if (width == 0 || height == 0) return;
    const bool geom = d_opacity || d_conic || d_uv;
    if (!geom && !d_colour) return;
    const uint32_t tx = (width + kTile - 1) / kTile, ty = (height + kTile - 1) / kTile;
    const uint2* rg = reinterpret_cast<const uint2*>(t.ranges);
    if (geom)
        hipLaunchKernelGGL((k_blend_backward<true>), dim3(tx * ty), dim3(BLOCK), 0, s, rg, t.sorted_gid, t.tile_order, t.rec, width, height,
                           tx, grad_rgb, grad_alpha, d_colour, d_opacity, d_conic, d_uv);
    else
        hipLaunchKernelGGL((k_blend_backward<false>), dim3(tx * ty), dim3(BLOCK), 0, s, rg, t.sorted_gid, t.tile_order, t.rec, width, height,
                           tx, grad_rgb, nullptr, d_colour, nullptr, nullptr, nullptr);
}

}  // namespace gs
