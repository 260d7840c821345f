// gs_knn_rules.h -- the arithmetic of gs_knn_dist2 (gs3d_hip.h): the Morton cell and code of a point, the squared distance d2,
// the two lower bounds that let the search pass a box over, the insertion into a lane's sorted `best` and the final mean.
// Plain inline functions, __host__ __device__ under hipcc and ordinary C++ otherwise, without a device in sight: the kernels
// (gs_knn.hip) and the CPU simulation of the whole search (tests/native/knn_rules_sim.cpp) compile this one text.
// Every operation is binary32 and rounded on its own, in the order written (-ffp-contract=off on both sides).
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define GS_KNN_HD __host__ __device__ __forceinline__
#else
#define GS_KNN_HD inline
#endif

namespace gs_knn {

constexpr uint32_t kCells = 1024;  // per axis: 10 bits, 30 in the code

// The cell of coordinate x on an axis of the bounding box [lo, lo + extent].  ANY bit pattern of x, lo and extent -- NaN and
// infinities included -- gives a cell in [0, 1023]: both comparisons are written so that a NaN takes the clamped branch, and the
// conversion only ever sees a value in [0, 1023].  An axis without extent (extent <= 0, or NaN) is cell 0.
GS_KNN_HD uint32_t morton_cell(float x, float lo, float extent) {
    if (!(extent > 0.0f)) return 0u;
    float t = ((x - lo) / extent) * 1024.0f;
    if (!(t >= 0.0f)) t = 0.0f;
    if (t > 1023.0f) t = 1023.0f;
    return (uint32_t)t;
}

// bits 0..9 of v to bits 0, 3, 6, ..., 27
GS_KNN_HD uint32_t morton_spread(uint32_t v) {
    v &= 0x3FFu;
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

// 30 bits: x in bit 0 of every triple, y in bit 1, z in bit 2
GS_KNN_HD uint32_t morton_code(uint32_t cx, uint32_t cy, uint32_t cz) {
    return morton_spread(cx) | (morton_spread(cy) << 1) | (morton_spread(cz) << 2);
}

// fl(fl(fl(ax ax) + fl(ay ay)) + fl(az az)): the one sum of three squares that d2 and both bounds share
GS_KNN_HD float sum_squares(float ax, float ay, float az) { return ((ax * ax) + (ay * ay)) + (az * az); }

// d2(i, j) of gs3d_hip.h
GS_KNN_HD float dist2(float xi, float yi, float zi, float xj, float yj, float zj) {
    return sum_squares(xi - xj, yi - yj, zi - zj);
}

// THE BOUND.  Per axis, between the intervals [loA, hiA] and [loB, hiB]:  g = max(fl(loB - hiA), 0, fl(loA - hiB)).
// For a in [loA, hiA] and b in [loB, hiB]:  where loB > hiA,  b - a >= loB - hiA > 0  as real numbers, and rounding to nearest
// is monotonic, so  |fl(a - b)| = fl(b - a) >= fl(loB - hiA) = g;  the other side alike;  where the intervals meet, g = 0 <=
// |fl(a - b)|.  So 0 <= g <= |fl(a - b)| on every axis.  A product of two equal non-negative factors is monotonic in the factor
// and so is its rounding; a sum of non-negatives is monotonic in each term and so is its rounding.  sum_squares(g) therefore
// never exceeds sum_squares of the member pair's differences, which is d2 -- the same operations in the same order, term by term.
// (A NaN cannot arise from finite coordinates: the differences are finite or +-inf, the squares and sums >= 0 or +inf.)
GS_KNN_HD float axis_gap(float loA, float hiA, float loB, float hiB) {
    float g = loB - hiA;
    const float h = loA - hiB;
    if (!(g > 0.0f)) g = 0.0f;
    if (h > g) g = h;
    return g;
}

struct Box {
    float lo[3], hi[3];
};

// <= d2(i, j) for every i in A and every j in B
GS_KNN_HD float box_box_bound(const Box& a, const Box& b) {
    return sum_squares(axis_gap(a.lo[0], a.hi[0], b.lo[0], b.hi[0]), axis_gap(a.lo[1], a.hi[1], b.lo[1], b.hi[1]),
                       axis_gap(a.lo[2], a.hi[2], b.lo[2], b.hi[2]));
}

// <= d2(i, j) for the point i = (x, y, z) and every j in B: the bound above with A the point
GS_KNN_HD float point_box_bound(float x, float y, float z, const Box& b) {
    return sum_squares(axis_gap(x, x, b.lo[0], b.hi[0]), axis_gap(y, y, b.lo[1], b.hi[1]), axis_gap(z, z, b.lo[2], b.hi[2]));
}

// best[0] <= ... <= best[K - 1], +inf where nothing is kept yet.  A candidate replaces a kept value only where d2 < kept: a NaN
// and a +inf are never kept, and equal values are kept as often as they occur.
template <int K>
GS_KNN_HD void insert(float (&best)[K], float d2) {
    if (!(d2 < best[K - 1])) return;
    best[K - 1] = d2;
#pragma unroll
    for (int i = K - 1; i > 0; --i) {
        const float a = best[i - 1], b = best[i];
        if (b < a) best[i - 1] = b, best[i] = a;
    }
}

// fl(fl(... fl(best[0] + best[1]) + ... + best[ke - 1]) / (float)ke), +0.0 where ke == 0
template <int K>
GS_KNN_HD float mean_of(const float (&best)[K], int ke) {
    if (ke <= 0) return 0.0f;
    float s = best[0];
#pragma unroll
    for (int i = 1; i < K; ++i)
        if (i < ke) s = s + best[i];
    return s / (float)ke;
}

// THE WALK of query box b over the other boxes of `boxes`, nearest in the sorted order first: position p = 0, 1, 2, ... is box
// b - (p / 2 + 1) for even p and b + (p / 2 + 1) for odd p; positions that fall outside [0, boxes) are passed over.
GS_KNN_HD uint32_t walk_positions(uint32_t b, uint32_t boxes) {
    const uint32_t left = b, right = boxes - 1u - b;
    return 2u * (left > right ? left : right);
}
GS_KNN_HD bool walk_box(uint32_t b, uint32_t boxes, uint32_t p, uint32_t* c) {
    const uint32_t d = p / 2u + 1u;
    if ((p & 1u) == 0u) {
        if (d > b) return false;
        *c = b - d;
        return true;
    }
    if (d > boxes - 1u - b) return false;
    *c = b + d;
    return true;
}

}  // namespace gs_knn
