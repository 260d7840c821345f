// gs_densify.hip -- adaptive density control on the device (gs3d_hip.h: gs_accumulate_densify_stats, gs_densify_plan,
// gs_densify_apply): k_densify_stats keeps the statistic that decides, k_densify_yield / k_densify_scan_parts / k_densify_offsets
// make the decision and its two prefix sums, k_densify_apply compacts the model and its Adam moments.  No reference counterpart.
//
// Part of libgs3d_hip.so (gfx950 only).  Built with -ffp-contract=off: every operation below is rounded on its own, in the order
// written; the decision and the split children are binary64 on exact conversions of the stored binary32 values, the activation is
// k_ingest_arrays's binary32 (gs_scene.hip), so the contract of all of it is a bit pattern (gs3d_hip.h states the order;
// tests/densify_reference.py restates it).
//
// THE PLAN is the reduce / scan / scatter of k_l1_scan's pattern over integers:
//   * k_densify_yield: a workgroup of BLOCK lanes takes GS_DENSIFY_PARTITION = 8 BLOCK consecutive parents, lane-contiguous (parent
//     g0 + k BLOCK + t in turn k), decides each one ONCE -- its yield (0, 1, 2 rows) goes to row_offset[i], "a split parent whose
//     children survive" to noise_offset[i] -- and leaves the partition's two sums in parts[];
//   * k_densify_scan_parts: ONE workgroup turns the partitions' sums into their exclusive prefixes, BLOCK at a time with a carry
//     (a model of 1 M parents has 489 partitions: two turns; 2^31 parents: 4096 turns), and writes the two totals to slot n;
//   * k_densify_offsets: the same grid reads the yields back, scans them inside the workgroup turn by turn from the partition's
//     base and overwrites them with the offsets -- each lane writes the slots it read.
// Integer sums: the result has one value whatever the order, so "deterministic" is free.  Sums are uint32: at most 2 (2^31 - 1),
// no wrap; the host refuses a total beyond 2^31 - 1.
//
// THE APPLY is memory-bound: per output row 59 parameters and up to 118 moments, each read once and written once.  The shape
// chosen -- the one the issue suggested, kept because nothing in it costs more than the traffic:
//   * a workgroup takes BLOCK consecutive parents; their output rows are ONE contiguous range [row_offset[g0], row_offset[g0 +
//     in_block]) of at most 2 BLOCK rows;
//   * phase 1, one lane per parent: the lane reads its two pairs of offsets and files (parent, role) for each of its rows in
//     s_tab, a dword per output row (a walk's 32 lanes read at most 32 consecutive dwords or one broadcast: no bank conflict; 2 KB).
//     role 0 = the original (moments carried), 1 = a clone's copy, 2 / 3 = split child 0 / 1.  A yield of 1 is the original unless
//     the screen-radius rule pruned it: then the parent was a clone and the row is its copy (the only way to lose one of two; the
//     lane re-reads max_radius for that).  A split parent's lane also computes both children's means and the shared log-scales
//     into s_means / s_ls BY OUTPUT ROW (stride 3 dwords per row; the 10 strided floats it reads cost uncoalesced requests, for the
//     few per cent of parents that split);
//   * phase 2: every output array is walked BY ELEMENT, lane-contiguous, as k_adam_step's adam_rows does: element j of the
//     workgroup's output range belongs to output row j / R, whose source the lane looks up in s_tab.  Stores are whole coalesced
//     requests; loads are the same rows at a non-decreasing offset (a run of kept rows is a straight copy);
//   * no atomics, no scratch memory, one writer per element.  Registers, LDS: profiles/densify_resource_usage.txt.
// Every index that comes from the offsets is clamped to the arrays' extents, so a scratch that was overwritten between plan and
// apply gives wrong rows, never a write outside the outputs.
#include "gs_device.h"

namespace gs {

static_assert(GS_DENSIFY_BLOCK == BLOCK && GS_DENSIFY_PARTITION % BLOCK == 0, "the plan's and the apply's tiles are multiples of the workgroup");
constexpr uint32_t kPlanTurns = GS_DENSIFY_PARTITION / BLOCK;

// ---------------------------------------------------------------------------------------------------------------- the statistic
__global__ __launch_bounds__(BLOCK) void k_densify_stats(const uint32_t* __restrict__ tiles, const AttrRecord* __restrict__ rec,
                                                         gs_densify_stats st, uint32_t n, double half_w, double half_h) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n || tiles[i] == 0u) return;
    const double gx = st.d_uv[2 * (size_t)i], gy = st.d_uv[2 * (size_t)i + 1];
    const double a = gx * half_w, b = gy * half_h;
    st.grad_sum[i] = st.grad_sum[i] + sqrt((a * a) + (b * b));
    st.count[i] = st.count[i] + 1u;
    const float radius = rec[i].depth_radius.y, was = st.max_radius[i];
    if (radius > was) st.max_radius[i] = radius;
}

void launch_densify_stats(const uint32_t* tiles, const AttrRecord* rec, const gs_densify_stats& st, uint32_t n, uint32_t width,
                          uint32_t height, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_densify_stats, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, tiles, rec, st, n, (double)width / 2.0,
                       (double)height / 2.0);
}

// ---------------------------------------------------------------------------------------------------------------- the decision
// s of three binary32 scales, as gs3d_hip.h writes it (a NaN in the first stays, one in the others is passed over)
__device__ __forceinline__ float largest_scale(float s0, float s1, float s2) {
    float s = s0;
    if (s1 > s) s = s1;
    if (s2 > s) s = s2;
    return s;
}

// Parent i: its yield in bits 0..1, "a split parent whose children survive" in bit 2.
__device__ __forceinline__ uint32_t densify_decide(const gs_densify_input& in, size_t i, const uint2* tab) {
    const gs_densify_rule& r = in.rule;
    const uint32_t cnt = in.count[i];
    const double avg = cnt != 0u ? in.grad_sum[i] / (double)cnt : 0.0;
    const float ls0 = in.params.log_scales[3 * i], ls1 = in.params.log_scales[3 * i + 1], ls2 = in.params.log_scales[3 * i + 2];
    const double s = (double)largest_scale(gs_expf_libm_domain(ls0, tab), gs_expf_libm_domain(ls1, tab), gs_expf_libm_domain(ls2, tab));
    const double o = (double)(1.0f / (1.0f + gs_expf_libm_domain(-in.params.opacity_logits[i], tab)));
    const bool grow = avg >= r.grad_threshold;
    const bool clone = grow && s <= r.dense_extent, split = grow && s > r.dense_extent;
    const bool faint = o < r.min_opacity;
    if (split) {
        const float c0 = (float)((double)ls0 - GS_DENSIFY_LOG_1_6), c1 = (float)((double)ls1 - GS_DENSIFY_LOG_1_6),
                    c2 = (float)((double)ls2 - GS_DENSIFY_LOG_1_6);
        const double sc = (double)largest_scale(gs_expf_libm_domain(c0, tab), gs_expf_libm_domain(c1, tab), gs_expf_libm_domain(c2, tab));
        const bool pruned = faint || (r.max_world_scale > 0.0 && sc > r.max_world_scale);
        return pruned ? 0u : (2u | 4u);
    }
    const bool both = faint || (r.max_world_scale > 0.0 && s > r.max_world_scale);  // what the original and its copy share
    const bool original = both || (r.max_screen_radius > 0.0 && (double)in.max_radius[i] > r.max_screen_radius);
    return (original ? 0u : 1u) + (clone && !both ? 1u : 0u);
}

// The workgroup's sum of v (every lane gets it); s_red: 4 uints of LDS.
__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t* s_red) {
#pragma unroll
    for (int d = WAVE / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, WAVE);
    __syncthreads();  // (s_red reuse)
    if ((threadIdx.x & (WAVE - 1)) == 0) s_red[threadIdx.x / WAVE] = v;
    __syncthreads();
    return (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

__global__ __launch_bounds__(BLOCK) void k_densify_yield(gs_densify_input in, uint32_t n, uint32_t* __restrict__ parts) {
    __shared__ uint32_t s_red[BLOCK / WAVE];
    const uint2* tab = reinterpret_cast<const uint2*>(kExpfTab);
    uint32_t* row_offset = in.scratch;
    uint32_t* noise_offset = in.scratch + (size_t)n + 1;
    const size_t g0 = (size_t)blockIdx.x * GS_DENSIFY_PARTITION;
    uint32_t rows = 0, noise = 0;
    for (uint32_t k = 0; k < kPlanTurns; ++k) {
        const size_t i = g0 + (size_t)k * BLOCK + threadIdx.x;
        if (i < n) {
            const uint32_t d = densify_decide(in, i, tab);
            row_offset[i] = d & 3u;
            noise_offset[i] = d >> 2;
            rows += d & 3u;
            noise += d >> 2;
        }
    }
    rows = block_sum(rows, s_red);
    noise = block_sum(noise, s_red);
    if (threadIdx.x == 0) parts[2 * (size_t)blockIdx.x] = rows, parts[2 * (size_t)blockIdx.x + 1] = noise;
}

// parts[2 p], parts[2 p + 1] <- the exclusive prefixes over the partitions; the totals to slot n of the two offset arrays.
__global__ __launch_bounds__(BLOCK) void k_densify_scan_parts(uint32_t* __restrict__ parts, uint32_t count, uint32_t* __restrict__ scratch, uint32_t n) {
    __shared__ uint32_t s_scan[8];
    uint32_t carry_rows = 0, carry_noise = 0;
    for (uint32_t p0 = 0; p0 < count; p0 += BLOCK) {  // (uniform: every lane takes every turn)
        const uint32_t p = p0 + threadIdx.x;
        const uint32_t rows = p < count ? parts[2 * (size_t)p] : 0u, noise = p < count ? parts[2 * (size_t)p + 1] : 0u;
        uint32_t total_rows, total_noise;
        const uint32_t before_rows = block_excl_scan<BLOCK>(rows, s_scan, &total_rows);
        const uint32_t before_noise = block_excl_scan<BLOCK>(noise, s_scan, &total_noise);
        if (p < count) parts[2 * (size_t)p] = carry_rows + before_rows, parts[2 * (size_t)p + 1] = carry_noise + before_noise;
        carry_rows += total_rows;
        carry_noise += total_noise;
    }
    if (threadIdx.x == 0) scratch[n] = carry_rows, scratch[2 * (size_t)n + 1] = carry_noise;
}

__global__ __launch_bounds__(BLOCK) void k_densify_offsets(uint32_t* __restrict__ scratch, uint32_t n, const uint32_t* __restrict__ parts) {
    __shared__ uint32_t s_scan[8];
    uint32_t* row_offset = scratch;
    uint32_t* noise_offset = scratch + (size_t)n + 1;
    const size_t g0 = (size_t)blockIdx.x * GS_DENSIFY_PARTITION;
    uint32_t base_rows = parts[2 * (size_t)blockIdx.x], base_noise = parts[2 * (size_t)blockIdx.x + 1];
    for (uint32_t k = 0; k < kPlanTurns; ++k) {  // (uniform)
        const size_t i = g0 + (size_t)k * BLOCK + threadIdx.x;
        const uint32_t rows = i < n ? row_offset[i] : 0u, noise = i < n ? noise_offset[i] : 0u;
        uint32_t total_rows, total_noise;
        const uint32_t before_rows = block_excl_scan<BLOCK>(rows, s_scan, &total_rows);
        const uint32_t before_noise = block_excl_scan<BLOCK>(noise, s_scan, &total_noise);
        if (i < n) row_offset[i] = base_rows + before_rows, noise_offset[i] = base_noise + before_noise;
        base_rows += total_rows;
        base_noise += total_noise;
    }
}

size_t densify_partitions(uint32_t n) { return ((size_t)n + GS_DENSIFY_PARTITION - 1) / GS_DENSIFY_PARTITION; }

void launch_densify_plan(const gs_densify_input& in, uint32_t n, uint32_t* parts, hipStream_t s) {
    if (n == 0) return;
    const uint32_t count = (uint32_t)densify_partitions(n);
    hipLaunchKernelGGL(k_densify_yield, dim3(count), dim3(BLOCK), 0, s, in, n, parts);
    hipLaunchKernelGGL(k_densify_scan_parts, dim3(1), dim3(BLOCK), 0, s, parts, count, in.scratch, n);
    hipLaunchKernelGGL(k_densify_offsets, dim3(count), dim3(BLOCK), 0, s, in.scratch, n, parts);
}

// ---------------------------------------------------------------------------------------------------------------- the compaction
struct DensifyTile {
    uint32_t g0, in_block;  // the workgroup's parents
    uint32_t r0, rows;      // its output rows [r0, r0 + rows), inside [0, n_out)
};

// The tile's elements of one [.][R] array, lane-contiguous.  moments: a row that is not an original gets +0.0.  s_new (R == 3 only;
// nullptr: every row is a copy): what a split child gets instead of its parent's row, in LDS by output row.
template <uint32_t R>
__device__ __forceinline__ void densify_rows(const float* __restrict__ src, float* __restrict__ dst, const DensifyTile& t,
                                             const uint32_t* s_tab, bool moments, const float* s_new) {
    const uint32_t* in = reinterpret_cast<const uint32_t*>(src) + (size_t)t.g0 * R;
    uint32_t* out = reinterpret_cast<uint32_t*>(dst) + (size_t)t.r0 * R;
    for (uint32_t j = threadIdx.x; j < R * t.rows; j += BLOCK) {
        const uint32_t c = j / R, e = j - c * R;
        const uint32_t entry = s_tab[c], role = entry & 3u, parent = entry >> 2;
        uint32_t v;
        if (moments && role != 0u) v = 0u;                                 // +0.0
        else if (s_new && role >= 2u) v = __float_as_uint(s_new[j]);       // (R == 3: the arrays by output row ARE by element)
        else v = in[(size_t)parent * R + e];
        out[j] = v;
    }
}

template <uint32_t R>
__device__ __forceinline__ void densify_group(const float* param, float* out_param, const gs_densify_output& o, int g, const DensifyTile& t,
                                              const uint32_t* s_tab, const float* s_new) {
    densify_rows<R>(param, out_param, t, s_tab, false, s_new);
    if (o.exp_avg[g]) {  // (uniform: a group's pair is given or not)
        densify_rows<R>(o.exp_avg[g], o.out_exp_avg[g], t, s_tab, true, nullptr);
        densify_rows<R>(o.exp_avg_sq[g], o.out_exp_avg_sq[g], t, s_tab, true, nullptr);
    }
}

__global__ __launch_bounds__(BLOCK) void k_densify_apply(gs_densify_input in, uint32_t n, gs_densify_output o) {
    __shared__ uint32_t s_tab[2 * BLOCK];
    __shared__ float s_means[3 * 2 * BLOCK], s_ls[3 * 2 * BLOCK];
    const uint2* tab = reinterpret_cast<const uint2*>(kExpfTab);
    const uint32_t* row_offset = in.scratch;
    const uint32_t* noise_offset = in.scratch + (size_t)n + 1;
    const uint32_t n_out = (uint32_t)o.n_out, n_noise = (uint32_t)o.n_noise;
    DensifyTile t;
    t.g0 = blockIdx.x * BLOCK;  // < n: the grid covers the parents
    t.in_block = min((uint32_t)BLOCK, n - t.g0);
    t.r0 = min(row_offset[t.g0], n_out);
    const uint32_t r1 = min(row_offset[t.g0 + t.in_block], n_out);
    t.rows = r1 > t.r0 ? min(r1 - t.r0, 2u * t.in_block) : 0u;
    if (t.rows == 0) return;  // (uniform)
    s_tab[threadIdx.x] = 0u, s_tab[BLOCK + threadIdx.x] = 0u;  // (parent 0 of the tile, the original: a legal source whatever follows)
    __syncthreads();

    if (threadIdx.x < t.in_block) {
        const size_t i = (size_t)t.g0 + threadIdx.x;
        const uint32_t at = row_offset[i], yield = row_offset[i + 1] - at;
        const uint32_t j = noise_offset[i], split = noise_offset[i + 1] - j;
        const uint32_t c = at - t.r0;  // (wraps where at < r0: the range test below then fails)
        if (yield == 2u && split == 1u && j < n_noise && c < t.rows && c + 1u < t.rows) {
            s_tab[c] = (threadIdx.x << 2) | 2u;
            s_tab[c + 1] = (threadIdx.x << 2) | 3u;
            const float* ls = in.params.log_scales + 3 * i;
            const float* q = in.params.quats + 4 * i;
            const float* m = in.params.means + 3 * i;
            double d[2][3];  // sigma o noise, per child
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float l = ls[k];
                const double sg = (double)gs_expf_libm_domain(l, tab);
                d[0][k] = sg * (double)o.noise[6 * (size_t)j + k];
                d[1][k] = sg * (double)o.noise[6 * (size_t)j + 3 + k];
                const float child = (float)((double)l - GS_DENSIFY_LOG_1_6);
                s_ls[3 * c + k] = child, s_ls[3 * (c + 1) + k] = child;
            }
            const float q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
            // the ingest's normalisation (k_ingest_arrays): v * (1 / sqrtf(dot)), dot = (e0 e0 + e1 e1) + (e2 e2 + e3 e3)
            const float dot = (q0 * q0 + q1 * q1) + (q2 * q2 + q3 * q3);
            const float inv = 1.0f / sqrtf(dot);
            const double w = (double)(q0 * inv), x = (double)(q1 * inv), y = (double)(q2 * inv), z = (double)(q3 * inv);
            const double R[3][3] = {{1.0 - 2.0 * ((y * y) + (z * z)), 2.0 * ((x * y) - (w * z)), 2.0 * ((x * z) + (w * y))},
                                    {2.0 * ((x * y) + (w * z)), 1.0 - 2.0 * ((x * x) + (z * z)), 2.0 * ((y * z) - (w * x))},
                                    {2.0 * ((x * z) - (w * y)), 2.0 * ((y * z) + (w * x)), 1.0 - 2.0 * ((x * x) + (y * y))}};
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const double mean = (double)m[r];
#pragma unroll
                for (int child = 0; child < 2; ++child)
                    s_means[3 * (c + child) + r] = (float)(mean + (((R[r][0] * d[child][0]) + (R[r][1] * d[child][1])) + (R[r][2] * d[child][2])));
            }
        } else if (yield == 2u && c < t.rows && c + 1u < t.rows) {
            s_tab[c] = threadIdx.x << 2;
            s_tab[c + 1] = (threadIdx.x << 2) | 1u;
        } else if (yield == 1u && c < t.rows) {
            // one row of a parent: the original, unless the screen-radius rule pruned it -- then the parent was cloned and this is the copy
            const bool copy = in.rule.max_screen_radius > 0.0 && (double)in.max_radius[i] > in.rule.max_screen_radius;
            s_tab[c] = (threadIdx.x << 2) | (copy ? 1u : 0u);
        }
    }
    __syncthreads();

    const gs_device_arrays& p = in.params;
    densify_group<3>(p.means, o.params.means, o, 0, t, s_tab, s_means);
    densify_group<3>(p.log_scales, o.params.log_scales, o, 1, t, s_tab, s_ls);
    densify_group<4>(p.quats, o.params.quats, o, 2, t, s_tab, nullptr);
    densify_group<1>(p.opacity_logits, o.params.opacity_logits, o, 3, t, s_tab, nullptr);
    densify_group<3>(p.sh_dc, o.params.sh_dc, o, 4, t, s_tab, nullptr);
    if (p.sh_rest_coeffs == 15u) densify_group<45>(p.sh_rest, o.params.sh_rest, o, 5, t, s_tab, nullptr);
    else if (p.sh_rest_coeffs == 8u) densify_group<24>(p.sh_rest, o.params.sh_rest, o, 5, t, s_tab, nullptr);
    else if (p.sh_rest_coeffs == 3u) densify_group<9>(p.sh_rest, o.params.sh_rest, o, 5, t, s_tab, nullptr);
}

void launch_densify_apply(const gs_densify_input& in, uint32_t n, const gs_densify_output& out, hipStream_t s) {
    if (n == 0 || out.n_out == 0) return;
    hipLaunchKernelGGL(k_densify_apply, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, in, n, out);
}

}  // namespace gs
