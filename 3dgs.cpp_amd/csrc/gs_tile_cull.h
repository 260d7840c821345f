// gs_tile_cull.h -- the alpha-cut tile box: which tiles of a Gaussian's reference tile box can hold a pixel that keeps it.
//
// Plain C++, host and device: k_preprocess (gs_preprocess.hip) takes the box per visible Gaussian, where conic, centre and cut
// sit in registers; the CPU tests compile this header alone with g++ (tests/test_tile_cull.py).  Built with -ffp-contract=off like
// everything around it; nothing here depends on a contraction either way (the slack covers both).
//
// The rule.  render.comp:61-89 keeps entry g at pixel p only if  cut <= power <= 0  (:68, :78 with the record's alpha cut, as
// every blend mode decides it), power = -q(d) as the shader rounds it, q(d) = 0.5 (a dx^2 + c dy^2) + b dx dy, d = uv - pixel
// (walk_pixel's convention: a pixel IS its integer coordinates, gs_tile_walk.h).  With L = -cut, a pixel whose EXACT q exceeds
// L + E is dropped by every mode as long as the shader's rounded power is within E of -q.  For a positive-definite conic the
// minimum of q over dy at a fixed dx is dx^2 det / (2 c), det = a c - b^2 (and dy^2 det / (2 a) the other way), so every pixel with
//     |dx| > hx = sqrt(2 (L + E) c / det)    or    |dy| > hy = sqrt(2 (L + E) a / det)
// is dropped: the axis-aligned bound of the ellipse q = L + E.  The tight box is the tiles of the reference box that hold a pixel
// column inside [u - hx, u + hx] and a pixel row inside [v - hy, v + hy].
//
// The slack, derived as quadrant_keep's (gs_tile_walk.h).
//  * E.  The rounding error of the shader's power is relative to its TERMS a dx^2 / 2, c dy^2 / 2, b dx dy, not to their sum (a
//    thin diagonal splat has terms ~1e5 cancelling to q ~ 5): at most 16 roundings of 2^-24 each, generously (dx, dy, two
//    products and the sums per term, with or without the three contractions), i.e. 9.6e-7 x the terms.  Only pixels of the
//    REFERENCE box are ever asked about, so the terms are bounded by their value at the box's pixel farthest from the centre:
//        E = 9.6e-7 (0.5 |a| Dx^2 + 0.5 |c| Dy^2 + |b| Dx Dy),   Dx, Dy = the largest |dx|, |dy| over the reference box's pixels.
//  * det.  a c - b b cancels for a thin diagonal splat.  Two products and a difference: the computed value is within
//    3 x 2^-24 (a c + b b) of the exact one; the rule divides by det_lo = det - 1.8e-7 (a c + b b) <= the exact det, and hands
//    back the reference box when det_lo <= 0 (or a <= 0, c <= 0, anything not finite): below that the conic is not known to be
//    positive definite and the bound above does not hold.
//  * hx, hy.  A sum, two products, a quotient and a square root, each within 2^-24: the factor 1 + 4e-6 covers them 16 times over;
//    the differences u -+ hx round by at most 2^-24 max(|u|, hx) and the scaling by 1 / 16 is exact: (|u| + hx + 1) 2.4e-7 is
//    added on top.  Every slack ENLARGES the box.
// cut = +inf (or any cut > 0): no power <= 0 is kept -- the box is empty.  cut = -inf: never culled -- the reference box.  NaN
// anywhere: the reference box.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GS_CULL_HD __host__ __device__ inline
#else
#define GS_CULL_HD inline
#endif

namespace gs {

struct TileBox {  // tiles [x0, x1) x [y0, y1); empty: x0 == x1 == y0 == y1 == 0
    int x0, y0, x1, y1;
};

constexpr int kCullTile = 16;  // render.comp's tile (gs_device.h: kTile), restated so that the header stands alone
constexpr float kCullTermSlack = 9.6e-7f, kCullDetSlack = 1.8e-7f, kCullRelSlack = 4e-6f, kCullAbsSlack = 2.4e-7f;

// one axis: the tiles of [t0, t1) that hold an integer pixel coordinate in [u - h, u + h]; false: none
GS_CULL_HD bool tile_cull_axis(float u, float h, int t0, int t1, int& o0, int& o1) {
    const float first = (float)(t0 * kCullTile), last = (float)(t1 * kCullTile - 1);  // the reference box's pixels (exact: < 2^24)
    // pixels are integers: the first that can keep the entry is ceil(u - h), the last floor(u + h) (a sixteenth of the bounds fall
    // in the last pixel's width before a tile edge: without this the rule keeps 0.674 of config B's instances instead of 0.647)
    const float lo = ceilf(fmaxf(u - h, first)), hi = floorf(fminf(u + h, last));     // NaN -> the reference's
    if (lo > hi) return false;
    // floor(x / 16) is monotone and the division by a power of two exact: a pixel in [lo, hi] lies in a tile in [o0, o1)
    o0 = (int)floorf(lo * (1.0f / kCullTile));
    o1 = (int)floorf(hi * (1.0f / kCullTile)) + 1;
    return true;
}

// conic (a, b, c), centre (u, v), `cut` as the record carries it, the reference tile box (non-empty) -> the tight box
GS_CULL_HD TileBox tile_cull_box(float a, float b, float c, float u, float v, float cut, TileBox ref) {
    const TileBox none{0, 0, 0, 0};
    if (cut > 0.0f) return none;                // +inf: never kept
    if (!(cut > -INFINITY)) return ref;         // -inf: always kept; NaN
    const float ac = a * c, bb = b * b;
    const float det_lo = (ac - bb) - kCullDetSlack * (ac + bb);
    if (!(det_lo > 0.0f) || !(a > 0.0f) || !(c > 0.0f) || !(det_lo < INFINITY)) return ref;  // degenerate or not finite
    // the reference box's pixel farthest from the centre, per axis
    const float Dx = fmaxf(fabsf(u - (float)(ref.x0 * kCullTile)), fabsf(u - (float)(ref.x1 * kCullTile - 1)));
    const float Dy = fmaxf(fabsf(v - (float)(ref.y0 * kCullTile)), fabsf(v - (float)(ref.y1 * kCullTile - 1)));
    const float mag = 0.5f * a * Dx * Dx + 0.5f * c * Dy * Dy + fabsf(b) * Dx * Dy;
    const float lim = 2.0f * (kCullTermSlack * mag - cut);  // 2 (L + E)
    const float sx = sqrtf(lim * c / det_lo), sy = sqrtf(lim * a / det_lo);
    const float hx = sx * (1.0f + kCullRelSlack) + (fabsf(u) + sx + 1.0f) * kCullAbsSlack;
    const float hy = sy * (1.0f + kCullRelSlack) + (fabsf(v) + sy + 1.0f) * kCullAbsSlack;
    TileBox t;
    if (!tile_cull_axis(u, hx, ref.x0, ref.x1, t.x0, t.x1) || !tile_cull_axis(v, hy, ref.y0, ref.y1, t.y0, t.y1)) return none;
    return t;
}

}  // namespace gs
