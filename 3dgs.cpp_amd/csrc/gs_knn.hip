// gs_knn.hip -- the mean squared distance of every point of a cloud to its k nearest neighbours, on the device (gs3d_hip.h:
// gs_knn_dist2): what a trainer derives its initial scales from.  No reference counterpart.
//
// Part of libgs3d_hip.so (gfx950 only).  Built with -ffp-contract=off: every operation is rounded on its own, in the order
// gs_knn_rules.h writes it -- the arithmetic (cell, code, d2, the two bounds, the insertion, the mean) lives THERE, so that the
// CPU simulation (tests/native/knn_rules_sim.cpp) runs the same text.  The contract is a bit pattern: the brute force over all
// pairs, restated in tests/knn_reference.py.  What is here is the order of the work, none of which can change a value:
//   * k_knn_bound_parts / k_knn_bound_final: min / max per axis in two stages, at most kKnnBoundParts partial rows, no atomics
//     (min and max of finite values have one value in any order); the final stage also leaves n where the radix passes read it;
//   * k_knn_codes: a 30-bit Morton code per point, (code, id) pairs for launch_radix_pass (gs_radix.hip: four stable passes of
//     8, 8, 8 and 6 bits, ties stay in id order);
//   * k_knn_gather: the points into ONE array in sorted order, 16 bytes each (x, y, z, the id's bits), so that the search reads
//     rows and not through an index; the same workgroup reduces the min / max of its GS_KNN_BOX points into the box table.  An id
//     is clamped to n - 1 before it is used: a scratch overwritten in flight gives wrong values, never an access outside `points`;
//   * k_knn_search<K>: a workgroup per query box, a lane per query point, best[K] in registers.  The own box first; then the
//     other boxes outward in the sorted order (gs_knn_rules.h: walk_box), GS_KNN_BOX walk positions per turn: every lane takes
//     the bound of ONE candidate box against the workgroup's radius R as it stands, a ballot per wave goes to LDS, and the
//     workgroup then visits the surviving positions IN ORDER, testing each again against R as it stands by then.  R only
//     falls, so a position dropped in the turn's first test would be dropped by the second too: the decisions are those of a
//     one-by-one walk, which is what the simulation runs and what box_visits is compared with.  An accepted box is staged once
//     in LDS (4 KB) and every lane that its own point-to-box bound does not excuse scans it: all lanes read the same 16 bytes,
//     a broadcast.  Every branch that guards a barrier is on workgroup-uniform values (R, the masks and the bounds come out of
//     LDS and are made scalar with readfirstlane); the lanes past n in the last box are masked, take every barrier, and count 0
//     towards R.
// Cost: a query box scans O(boxes / GS_KNN_BOX) turns plus the boxes it accepts; all points coincident accepts everything (n^2).
// No atomics, no scratch memory; registers and LDS: profiles/knn_resource_usage.txt.
#include "gs_device.h"
#include "gs_knn_rules.h"

namespace gs {

constexpr uint32_t kKnnBox = GS_KNN_BOX, kKnnWaves = kKnnBox / WAVE;
static_assert(kKnnBox % WAVE == 0 && kKnnBox >= WAVE && kKnnBox <= 1024, "a box is a whole number of waves and one workgroup");

__device__ __forceinline__ float knn_min(float a, float b) { return b < a ? b : a; }
__device__ __forceinline__ float knn_max(float a, float b) { return b > a ? b : a; }
__device__ __forceinline__ float knn_uniform(float v) { return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(v))); }

// lo[3], hi[3] reduced over the workgroup of WAVES waves into lane 0's copies; s_red: 6 * WAVES floats of LDS.
template <uint32_t WAVES>
__device__ __forceinline__ void knn_reduce_bounds(float (&lo)[3], float (&hi)[3], float* s_red) {
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int d = WAVE / 2; d > 0; d >>= 1) {
            lo[a] = knn_min(lo[a], __shfl_xor(lo[a], d, WAVE));
            hi[a] = knn_max(hi[a], __shfl_xor(hi[a], d, WAVE));
        }
    const uint32_t w = threadIdx.x / WAVE;
    if ((threadIdx.x & (WAVE - 1)) == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) s_red[6 * w + a] = lo[a], s_red[6 * w + 3 + a] = hi[a];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t k = 1; k < WAVES; ++k)
#pragma unroll
            for (int a = 0; a < 3; ++a) lo[a] = knn_min(lo[a], s_red[6 * k + a]), hi[a] = knn_max(hi[a], s_red[6 * k + 3 + a]);
    }
}

constexpr float kKnnInf = __builtin_huge_valf();

// ---------------------------------------------------------------------------------------------------------------- bounding box
__global__ __launch_bounds__(BLOCK) void k_knn_bound_parts(const float* __restrict__ points, uint32_t n, float* __restrict__ parts) {
    __shared__ float s_red[6 * (BLOCK / WAVE)];
    float lo[3] = {kKnnInf, kKnnInf, kKnnInf}, hi[3] = {-kKnnInf, -kKnnInf, -kKnnInf};
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * BLOCK) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float v = points[3 * i + a];
            lo[a] = knn_min(lo[a], v), hi[a] = knn_max(hi[a], v);
        }
    }
    knn_reduce_bounds<BLOCK / WAVE>(lo, hi, s_red);
    if (threadIdx.x == 0) {
        float* row = parts + 8 * (size_t)blockIdx.x;
#pragma unroll
        for (int a = 0; a < 3; ++a) row[a] = lo[a], row[4 + a] = hi[a];
    }
}

__global__ __launch_bounds__(BLOCK) void k_knn_bound_final(const float* __restrict__ parts, uint32_t rows, float* __restrict__ bbox,
                                                           uint32_t* __restrict__ count, uint32_t n) {
    __shared__ float s_red[6 * (BLOCK / WAVE)];
    float lo[3] = {kKnnInf, kKnnInf, kKnnInf}, hi[3] = {-kKnnInf, -kKnnInf, -kKnnInf};
    for (uint32_t r = threadIdx.x; r < rows; r += BLOCK) {
#pragma unroll
        for (int a = 0; a < 3; ++a) lo[a] = knn_min(lo[a], parts[8 * (size_t)r + a]), hi[a] = knn_max(hi[a], parts[8 * (size_t)r + 4 + a]);
    }
    knn_reduce_bounds<BLOCK / WAVE>(lo, hi, s_red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) bbox[a] = lo[a], bbox[4 + a] = hi[a];
        bbox[3] = 0.0f, bbox[7] = 0.0f;
        *count = n;
    }
}

// ---------------------------------------------------------------------------------------------------------------- Morton order
__global__ __launch_bounds__(BLOCK) void k_knn_codes(const float* __restrict__ points, uint32_t n, const float* __restrict__ bbox,
                                                     uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    uint32_t cell[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float lo = bbox[a];
        cell[a] = gs_knn::morton_cell(points[3 * i + a], lo, bbox[4 + a] - lo);
    }
    keys[i] = gs_knn::morton_code(cell[0], cell[1], cell[2]);
    vals[i] = (uint32_t)i;
}

__global__ __launch_bounds__(kKnnBox) void k_knn_gather(const float* __restrict__ points, uint32_t n, const uint32_t* __restrict__ order,
                                                        float4* __restrict__ sorted, float4* __restrict__ boxes) {
    __shared__ float s_red[6 * kKnnWaves];
    const uint64_t j = (uint64_t)blockIdx.x * kKnnBox + threadIdx.x;
    float lo[3] = {kKnnInf, kKnnInf, kKnnInf}, hi[3] = {-kKnnInf, -kKnnInf, -kKnnInf};
    if (j < n) {
        const uint32_t id = min(order[j], n - 1u);
        const float x = points[3 * (size_t)id], y = points[3 * (size_t)id + 1], z = points[3 * (size_t)id + 2];
        sorted[j] = make_float4(x, y, z, __uint_as_float(id));
        lo[0] = hi[0] = x, lo[1] = hi[1] = y, lo[2] = hi[2] = z;
    }
    knn_reduce_bounds<kKnnWaves>(lo, hi, s_red);
    if (threadIdx.x == 0) {
        boxes[2 * (size_t)blockIdx.x] = make_float4(lo[0], lo[1], lo[2], 0.0f);
        boxes[2 * (size_t)blockIdx.x + 1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
    }
}

// ---------------------------------------------------------------------------------------------------------------- the search
__device__ __forceinline__ gs_knn::Box knn_load_box(const float4* __restrict__ boxes, uint32_t c) {
    const float4 lo = boxes[2 * (size_t)c], hi = boxes[2 * (size_t)c + 1];
    gs_knn::Box b;
    b.lo[0] = lo.x, b.lo[1] = lo.y, b.lo[2] = lo.z;
    b.hi[0] = hi.x, b.hi[1] = hi.y, b.hi[2] = hi.z;
    return b;
}

template <int K>
__global__ __launch_bounds__(kKnnBox) void k_knn_search(const float4* __restrict__ sorted, const float4* __restrict__ boxes, uint32_t n,
                                                        uint32_t nb, int ke, float* __restrict__ mean, float* __restrict__ dist2,
                                                        uint32_t* __restrict__ visits) {
    __shared__ float4 s_pts[kKnnBox];
    __shared__ float s_lb[kKnnBox];
    __shared__ uint64_t s_mask[kKnnWaves];
    __shared__ float s_r[kKnnWaves];
    const uint32_t b = blockIdx.x, t = threadIdx.x, w = t / WAVE, lane = t & (WAVE - 1);
    const uint32_t j = b * kKnnBox + t;  // (b kKnnBox < n < 2^31)
    const bool active = j < n;
    const float4 q = active ? sorted[j] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const uint32_t my_id = __float_as_uint(q.w);
    float best[K];
#pragma unroll
    for (int i = 0; i < K; ++i) best[i] = kKnnInf;
    float R = kKnnInf;  // the largest best[K - 1] of the workgroup's lanes: uniform
    uint32_t staged = 0;

    // Stage box c, let every lane it may matter to scan it, and take the workgroup's radius again.  Called under uniform control.
    auto examine = [&](uint32_t c, const gs_knn::Box& cb) {
        const uint32_t base = c * kKnnBox, cnt = min(kKnnBox, n - base);
        if (t < cnt) s_pts[t] = sorted[base + t];  // (the last scan ended before the barrier that closed the examine before)
        __syncthreads();
        if (active && !(gs_knn::point_box_bound(q.x, q.y, q.z, cb) > best[K - 1])) {
            for (uint32_t e = 0; e < cnt; ++e) {
                const float4 p = s_pts[e];
                if (__float_as_uint(p.w) != my_id) gs_knn::insert<K>(best, gs_knn::dist2(q.x, q.y, q.z, p.x, p.y, p.z));
            }
        }
        float r = active ? best[K - 1] : 0.0f;
#pragma unroll
        for (int d = WAVE / 2; d > 0; d >>= 1) r = knn_max(r, __shfl_xor(r, d, WAVE));
        if (lane == 0) s_r[w] = r;
        __syncthreads();
        r = s_r[0];
#pragma unroll
        for (uint32_t k = 1; k < kKnnWaves; ++k) r = knn_max(r, s_r[k]);
        R = knn_uniform(r);
        ++staged;
    };

    const gs_knn::Box mine = knn_load_box(boxes, b);
    examine(b, mine);

    const uint32_t positions = gs_knn::walk_positions(b, nb);
    for (uint32_t p0 = 0; p0 < positions; p0 += kKnnBox) {  // (uniform)
        __syncthreads();  // s_lb and s_mask of the turn before are read no more
        float lb = kKnnInf;
        bool candidate = false;
        uint32_t c = 0;
        if (p0 + t < positions && gs_knn::walk_box(b, nb, p0 + t, &c)) {
            lb = gs_knn::box_box_bound(mine, knn_load_box(boxes, c));
            candidate = !(lb > R);
        }
        s_lb[t] = lb;
        const uint64_t m = __ballot(candidate);
        if (lane == 0) s_mask[w] = m;
        __syncthreads();
        for (uint32_t k = 0; k < kKnnWaves; ++k) {
            const uint64_t mk = s_mask[k];
            uint64_t left = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(mk >> 32)) << 32) | __builtin_amdgcn_readfirstlane((uint32_t)mk);
            while (left) {
                const uint32_t e = k * WAVE + (uint32_t)(__ffsll((unsigned long long)left) - 1);
                left &= left - 1;
                if (knn_uniform(s_lb[e]) > R) continue;  // R has fallen since the turn's first test
                uint32_t cc = 0;
                (void)gs_knn::walk_box(b, nb, p0 + e, &cc);  // (true: the lane that set the bit found it so)
                examine(cc, knn_load_box(boxes, cc));
            }
        }
    }

    if (visits && t == 0) visits[b] = staged;
    if (!active) return;
    if (mean) mean[my_id] = gs_knn::mean_of<K>(best, ke);
    if (dist2) {
#pragma unroll
        for (int i = 0; i < K; ++i) dist2[(size_t)my_id * K + i] = best[i];
    }
}

// ---------------------------------------------------------------------------------------------------------------- host side
static size_t knn_round16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }
static int knn_radix_blocks(uint32_t n) { return std::max(1, std::min<int>(kSortMaxBlocks, (int)(((uint64_t)n + kSortTileKeys - 1) / kSortTileKeys))); }
static uint32_t knn_bound_rows(uint32_t n) { return std::min<uint32_t>(kKnnBoundParts, (uint32_t)(((uint64_t)n + BLOCK - 1) / BLOCK)); }

// The segments in order; `base` null: only the size is wanted.
static size_t knn_layout(uint8_t* base, uint32_t n, KnnBuffers* out) {
    size_t at = 0;
    auto take = [&](size_t bytes) {
        uint8_t* p = base ? base + at : nullptr;
        at += knn_round16(bytes);
        return p;
    };
    KnnBuffers b;
    b.sorted = reinterpret_cast<float4*>(take((size_t)n * sizeof(float4)));
    b.boxes = reinterpret_cast<float4*>(take(2 * (size_t)knn_boxes(n) * sizeof(float4)));
    for (int k = 0; k < 2; ++k) b.keys[k] = reinterpret_cast<uint32_t*>(take((size_t)n * sizeof(uint32_t)));
    for (int k = 0; k < 2; ++k) b.vals[k] = reinterpret_cast<uint32_t*>(take((size_t)n * sizeof(uint32_t)));
    b.block_hist = reinterpret_cast<uint32_t*>(take(256 * (size_t)knn_radix_blocks(n) * sizeof(uint32_t)));
    b.digit_total = reinterpret_cast<uint32_t*>(take(256 * sizeof(uint32_t)));
    b.bbox_parts = reinterpret_cast<float*>(take(8 * (size_t)knn_bound_rows(n) * sizeof(float)));
    b.bbox = reinterpret_cast<float*>(take(8 * sizeof(float)));
    b.count = reinterpret_cast<uint32_t*>(take(sizeof(uint32_t)));
    if (out) *out = b;
    return at;
}

size_t knn_scratch_bytes(uint64_t n) { return n == 0 ? 0 : knn_layout(nullptr, (uint32_t)n, nullptr) + 16; }

KnnBuffers knn_buffers(void* scratch, uint32_t n) {
    KnnBuffers b;
    uint8_t* base = reinterpret_cast<uint8_t*>((reinterpret_cast<uintptr_t>(scratch) + 15) & ~(uintptr_t)15);
    knn_layout(base, n, &b);
    return b;
}

template <int K>
static void knn_launch_search(const KnnBuffers& b, uint32_t n, int ke, float* mean, float* dist2, uint32_t* visits, hipStream_t s) {
    hipLaunchKernelGGL(k_knn_search<K>, dim3(knn_boxes(n)), dim3(kKnnBox), 0, s, b.sorted, b.boxes, n, knn_boxes(n), ke, mean, dist2, visits);
}

void launch_knn(const float* points, uint32_t n, int k, float* mean, float* dist2, uint32_t* visits, const KnnBuffers& b, hipStream_t s) {
    if (n == 0) return;
    const uint32_t rows = knn_bound_rows(n);
    hipLaunchKernelGGL(k_knn_bound_parts, dim3(rows), dim3(BLOCK), 0, s, points, n, b.bbox_parts);
    hipLaunchKernelGGL(k_knn_bound_final, dim3(1), dim3(BLOCK), 0, s, b.bbox_parts, rows, b.bbox, b.count, n);
    hipLaunchKernelGGL(k_knn_codes, dim3((uint32_t)(((uint64_t)n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, points, n, b.bbox, b.keys[0], b.vals[0]);
    static const int kBits[4] = {8, 8, 8, 6};  // 30 bits of code
    for (int pass = 0; pass < 4; ++pass) {
        RadixPass p{};
        p.keys_in = b.keys[pass & 1], p.vals_in = b.vals[pass & 1];
        p.keys_out = b.keys[(pass & 1) ^ 1], p.vals_out = b.vals[(pass & 1) ^ 1];
        p.n_in = b.count;
        p.n_static = n;
        p.block_hist = b.block_hist, p.digit_total = b.digit_total;
        p.shift = 8 * pass, p.bits = kBits[pass];
        p.blocks = knn_radix_blocks(n);
        p.first = 0;
        launch_radix_pass(p, s);
    }
    hipLaunchKernelGGL(k_knn_gather, dim3(knn_boxes(n)), dim3(kKnnBox), 0, s, points, n, b.vals[0], b.sorted, b.boxes);
    const int ke = (int)std::min<uint64_t>((uint64_t)k, (uint64_t)n - 1);
    switch (k) {
        case 1: knn_launch_search<1>(b, n, ke, mean, dist2, visits, s); break;
        case 2: knn_launch_search<2>(b, n, ke, mean, dist2, visits, s); break;
        case 3: knn_launch_search<3>(b, n, ke, mean, dist2, visits, s); break;
        case 4: knn_launch_search<4>(b, n, ke, mean, dist2, visits, s); break;
        case 5: knn_launch_search<5>(b, n, ke, mean, dist2, visits, s); break;
        case 6: knn_launch_search<6>(b, n, ke, mean, dist2, visits, s); break;
        case 7: knn_launch_search<7>(b, n, ke, mean, dist2, visits, s); break;
        default: knn_launch_search<8>(b, n, ke, mean, dist2, visits, s); break;
    }
}

}  // namespace gs
