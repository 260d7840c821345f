// gs_wave_f64.h -- binary64 sums across a wave, shared by k_lift (gs_lift.hip) and k_blend_backward (gs_backward.hip): the DPP
// moves of a double, the wave sum, and the transpose-reduces that leave every lane with ONE channel's sum over its row of 16 lanes.
//
// Device code, included by those two translation units; built with -ffp-contract=off like them.  Every function here needs every
// lane of the wave active (the DPP reads and v_readlane take what an inactive lane last held).
#pragma once
#include "gs_device.h"

namespace gs {

template <int CTRL>
__device__ __forceinline__ double dpp_f64(double x) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), CTRL, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double readlane_f64(double x, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), l), __builtin_amdgcn_readlane(__double2loint(x), l));
}

// Sum of x over the wave's 64 lanes in binary64, wave-uniform; every lane must be active.  wave_sum's pattern (gs_contrib.hip) on
// both halves of the double: four DPP steps make each row of 16 lanes hold its own sum (each step adds two values that the two
// partner lanes add in either order: the same bits), four lanes are read and joined with three adds.
__device__ __forceinline__ double wave_sum_f64(double x) {
    x = x + dpp_f64<0xB1>(x);   // quad_perm [1, 0, 3, 2]
    x = x + dpp_f64<0x4E>(x);   // quad_perm [2, 3, 0, 1]
    x = x + dpp_f64<0x141>(x);  // row_half_mirror
    x = x + dpp_f64<0x140>(x);  // row_mirror
    return (readlane_f64(x, 0) + readlane_f64(x, 16)) + (readlane_f64(x, 32) + readlane_f64(x, 48));
}

// The transpose-reduce of a group.  Position j of a lane's registers holds the channel lift_channel<G>(j, lane): the lane's
// channels in an order that depends on the lane, chosen so that every step below moves whole registers and needs no select.
// With b0, b1 the lane's two low bits and Q = (lane >> 2) & 3 its quad within the row of 16:
//   step A  (lane ^ 1)  a lane keeps the first half of its positions and adds the partner's second half: the partner holds the
//                       two halves swapped (the top bit of the channel is the top bit of the position ^ b0);
//   step B  (lane ^ 2)  the same on what is left (the next bit of the channel is the next bit of the position ^ b1);
//   step C  G = 16: four positions are left, the same four channels in the four quads of the row, position p of quad Q holding
//                       the low channel bits (Q + p) & 3: a lane keeps position 0, i.e. Q, and takes position 1 of the quad one
//                       rotation behind, 2 of the quad two behind, 3 of the quad three behind (row_ror:4, 8, 12), each of which
//                       is its own Q again;
//           G = 4:  one position is left, the same channel in the four quads: the same three rotations sum them.
// After A, B, C a lane holds ONE channel, lift_final<G>(lane), summed in binary64 over its row of 16 lanes: G/2 + G/4 + 3 adds
// for G channels, where a DPP sum per channel takes 4 G and 8 G v_readlane.  The wave's four rows meet in the LDS slot.
template <int G>
__device__ __forceinline__ uint32_t lift_channel(int j, int lane) {
    const uint32_t b0 = lane & 1, b1 = (lane >> 1) & 1, q = (lane >> 2) & 3;
    uint32_t c = ((((uint32_t)j / (G / 2)) & 1) ^ b0) * (G / 2) + ((((uint32_t)j / (G / 4)) & 1) ^ b1) * (G / 4);
    if (G == 16) c += (q + ((uint32_t)j & 3)) & 3;
    return c;
}

template <int G>
__device__ __forceinline__ uint32_t lift_final(int lane) {
    const uint32_t b0 = lane & 1, b1 = (lane >> 1) & 1, q = (lane >> 2) & 3;
    return b0 * (G / 2) + b1 * (G / 4) + (G == 16 ? q : 0);
}

// v: the lane's values in lift_channel's order.  w: (double)fl32(alpha T) where the lane blends the entry, 0 elsewhere; `upd`
// says which.  A lane that does not blend takes 0 * 0: its values -- a NaN among them -- are selected away, never multiplied.
template <int G>
__device__ __forceinline__ double lift_reduce(const float (&v)[G], double w, bool upd) {
    static_assert(G == 4 || G == 16, "steps A and B halve twice, step C takes four positions or one");
    double x[G / 2];
#pragma unroll
    for (int j = 0; j < G / 2; ++j) {
        // (the values are converted HERE, per entry: hoisted out of the walk, the doubles would cost G more registers)
        float lo = upd ? v[j] : 0.0f, hi = upd ? v[j + G / 2] : 0.0f;
        asm volatile("" : "+v"(lo), "+v"(hi));
        x[j] = w * (double)lo + dpp_f64<0xB1>(w * (double)hi);  // A: quad_perm [1, 0, 3, 2]
    }
#pragma unroll
    for (int j = 0; j < G / 4; ++j) x[j] = x[j] + dpp_f64<0x4E>(x[j + G / 4]);  // B: quad_perm [2, 3, 0, 1]
    constexpr int R = G / 4;  // C: row_ror:4, 8, 12
    return (x[0] + dpp_f64<0x124>(x[1 % R])) + (dpp_f64<0x128>(x[2 % R]) + dpp_f64<0x12C>(x[3 % R]));
}

// The same steps for terms that are binary64 already and are formed per entry, in NATURAL order t[0 .. 3] (gs_backward.hip: they
// are no product with a value that could be put in lift_channel's order once, before the walk).  The order is made here: position
// j of a lane is channel j ^ (2 b0 + b1), two levels of whole-register selects.  Returns channel lift_final<4>(lane) = 2 b0 + b1
// summed over the lane's row of 16; the four quads of a row hold the same four sums.
__device__ __forceinline__ double row_reduce4_f64(const double (&t)[4], int lane) {
    const bool b0 = lane & 1, b1 = lane & 2;
    const double s0 = b1 ? t[1] : t[0], s1 = b1 ? t[0] : t[1], s2 = b1 ? t[3] : t[2], s3 = b1 ? t[2] : t[3];
    const double p0 = b0 ? s2 : s0, p1 = b0 ? s3 : s1, p2 = b0 ? s0 : s2, p3 = b0 ? s1 : s3;
    const double a0 = p0 + dpp_f64<0xB1>(p2), a1 = p1 + dpp_f64<0xB1>(p3);  // A
    const double b = a0 + dpp_f64<0x4E>(a1);                                // B
    return (b + dpp_f64<0x124>(b)) + (dpp_f64<0x128>(b) + dpp_f64<0x12C>(b));  // C
}

// Two terms: a lane keeps t[b0] and adds the partner's (lane ^ 1), then lane ^ 2 and the three rotations, which all keep b0.
// Returns channel b0 = lane & 1 summed over the lane's row of 16.
__device__ __forceinline__ double row_reduce2_f64(double t0, double t1, int lane) {
    const bool b0 = lane & 1;
    double x = (b0 ? t1 : t0) + dpp_f64<0xB1>(b0 ? t0 : t1);
    x = x + dpp_f64<0x4E>(x);
    return (x + dpp_f64<0x124>(x)) + (dpp_f64<0x128>(x) + dpp_f64<0x12C>(x));
}

}  // namespace gs
