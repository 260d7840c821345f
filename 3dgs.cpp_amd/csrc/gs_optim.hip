// gs_optim.hip -- k_adam_step: the sparse Adam step of a trainer on this rasteriser (gs_scene_adam_step, gs3d_hip.h), and
// k_visible_mask: the last frame's visibility as the mask such a step takes (gs_visible_mask).  No reference counterpart.
//
// Part of libgs3d_hip.so (gfx950 only).  Built with -ffp-contract=off: every operation below is rounded on its own, in the order
// written; the update is binary64 on exact conversions of the stored binary32 values, the activation is k_ingest_arrays's binary32
// (gs_scene.hip), so the contract of both is a bit pattern (gs3d_hip.h states the order; tests/adam_step_reference.py restates it).
//
// k_adam_step is memory-bound: per masked Gaussian 59 elements x (8 B gradient in, 8 B out when zeroing, 4 B in + 4 B out for each
// of parameter, exp_avg, exp_avg_sq) = 2.4 KB, plus the blob's 236 B; against that about a hundred binary64 operations per element
// (one square root, two divisions).  The shape chosen -- the one the issue suggested, kept because nothing in it costs more than the
// traffic:
//   * a workgroup of BLOCK lanes takes BLOCK consecutive Gaussians, by SCENE ID (the step writes the canonical blob; the copy in
//     spatial order is redone by launch_permute_blob afterwards);
//   * it reads its BLOCK mask bytes first and leaves on __syncthreads_or() == 0 before touching anything else: in a scene whose ids
//     are spatially coherent whole runs are culled together;
//   * every [N][R] array is walked BY ELEMENT, lane-contiguous, as k_ingest_arrays reads its sources (they are 4-byte / 8-byte
//     aligned and no more): element j of the workgroup's run belongs to Gaussian j / R, whose mask byte the lane looks up in LDS.
//     A masked Gaussian's rows therefore cost whole coalesced accesses; an unmasked Gaussian's elements are neither read nor
//     written (its lanes sit out);
//   * the new means, log-scales and quaternions go to LDS (3 + 3 + 4 floats per Gaussian, 10 KB) and a second phase, one lane per
//     Gaussian, activates them into the planes exactly as k_ingest_arrays does -- the quaternion's norm needs its four components
//     together; a stride of 3 dwords is conflict-free on 32 banks, the quaternion is one 16-byte ds_read_b128 per lane;
//   * the opacity (R = 1: the lane IS the Gaussian) is activated where it is updated; SH elements go from the update straight to
//     their place in the blob's 48-float row (consecutive lanes, consecutive floats of a row);
//   * no atomics, no scratch: one writer per element.  Registers, LDS: profiles/adam_step_resource_usage.txt.
// A group whose pointers are null (uniform branch) is not stepped and its planes keep their bits; so do the SH bands beyond
// sh_rest_coeffs (gs_scene_update_from_device_arrays zeroes them: stated in gs3d_hip.h).
#include "gs_device.h"

namespace gs {

// One element: exp_avg, exp_avg_sq and param of G at e are replaced, the gradient is consumed; returns the new binary32 parameter.
//     m' = (beta1 m) + ((1 - beta1) g)        v' = (beta2 v) + (((1 - beta2) g) g)
//     d  = (sqrt(v') / sqrt(bc2)) + eps       p' = p - ((lr / bc1) (m' / d))            one rounding each; three at the stores
__device__ __forceinline__ float adam_element(const AdamGroup& G, const AdamStep& a, size_t e) {
    const double g = G.grad[e];
    const double m = (a.beta1 * (double)G.exp_avg[e]) + (a.one_minus_beta1 * g);
    const double v = (a.beta2 * (double)G.exp_avg_sq[e]) + ((a.one_minus_beta2 * g) * g);
    const double d = (sqrt(v) / a.sqrt_bc2) + a.eps;  // sqrt and / are IEEE (no fast-math in this build)
    const double p = (double)G.param[e] - (G.step * (m / d));
    const float pf = (float)p;
    G.exp_avg[e] = (float)m;
    G.exp_avg_sq[e] = (float)v;
    G.param[e] = pf;
    if (a.zero_grads) G.grad[e] = 0.0;
    return pf;
}

// The run's elements of one group of row width R, lane-contiguous: put(Gaussian of the run, element of its row, new value).
template <uint32_t R, class Put>
__device__ __forceinline__ void adam_rows(const AdamGroup& G, const AdamStep& a, const uint8_t* s_mask, uint32_t g0, uint32_t in_block,
                                          Put&& put) {
    const size_t base = (size_t)g0 * R;
    for (uint32_t j = threadIdx.x; j < R * in_block; j += BLOCK) {
        const uint32_t gl = j / R;
        if (!s_mask[gl]) continue;
        put(gl, j - gl * R, adam_element(G, a, base + j));
    }
}

__global__ __launch_bounds__(BLOCK) void k_adam_step(AdamStep a, float* __restrict__ blob, uint32_t stride, uint32_t n) {
    __shared__ float s_pos[3 * BLOCK], s_scale[3 * BLOCK];
    __shared__ __attribute__((aligned(16))) float s_rot[4 * BLOCK];
    __shared__ uint8_t s_mask[BLOCK];
    const uint32_t g0 = blockIdx.x * BLOCK, t = threadIdx.x, i = g0 + t;  // g0 < n: the grid covers the scene
    const uint32_t in_block = min((uint32_t)BLOCK, n - g0);
    const uint8_t mine = i < n && (!a.mask || a.mask[i] != 0) ? 1 : 0;
    s_mask[t] = mine;
    if (!__syncthreads_or(mine)) return;  // (also the barrier that publishes s_mask)

    const size_t N = stride;
    const uint2* tab = reinterpret_cast<const uint2*>(kExpfTab);
    float* sh_rows = blob + (size_t)P_SH * N + (size_t)g0 * 48u;
    if (a.means.param) adam_rows<3>(a.means, a, s_mask, g0, in_block, [&](uint32_t gl, uint32_t c, float p) { s_pos[3 * gl + c] = p; });
    if (a.log_scales.param) adam_rows<3>(a.log_scales, a, s_mask, g0, in_block, [&](uint32_t gl, uint32_t c, float p) { s_scale[3 * gl + c] = p; });
    if (a.quats.param) adam_rows<4>(a.quats, a, s_mask, g0, in_block, [&](uint32_t gl, uint32_t c, float p) { s_rot[4 * gl + c] = p; });
    if (a.opacity_logits.param)
        adam_rows<1>(a.opacity_logits, a, s_mask, g0, in_block, [&](uint32_t gl, uint32_t, float p) {
            blob[P_OPACITY * N + g0 + gl] = 1.0f / (1.0f + gs_expf_libm_domain(-p, tab));
        });
    if (a.sh_dc.param) adam_rows<3>(a.sh_dc, a, s_mask, g0, in_block, [&](uint32_t gl, uint32_t c, float p) { sh_rows[gl * 48u + c] = p; });
    if (a.sh_rest.param) {
        auto put = [&](uint32_t gl, uint32_t c, float p) { sh_rows[gl * 48u + 3u + c] = p; };
        if (a.sh_rest_coeffs == 15u) adam_rows<45>(a.sh_rest, a, s_mask, g0, in_block, put);
        else if (a.sh_rest_coeffs == 8u) adam_rows<24>(a.sh_rest, a, s_mask, g0, in_block, put);
        else adam_rows<9>(a.sh_rest, a, s_mask, g0, in_block, put);
    }
    __syncthreads();
    if (!mine) return;
    float* out = blob + i;
    if (a.means.param) {
        for (int k = 0; k < 3; ++k) out[(P_POS + k) * N] = s_pos[3 * t + k];
    }
    if (a.log_scales.param) {
        for (int k = 0; k < 3; ++k) out[(P_SCALE + k) * N] = gs_expf_libm_domain(s_scale[3 * t + k], tab);
    }
    if (a.quats.param) {
        const float4 q = reinterpret_cast<const float4*>(s_rot)[t];
        // glm::normalize(vec4) as k_ingest_arrays writes it: v * inversesqrt(dot(v, v)), dot<4> = (x*x + y*y) + (z*z + w*w)
        const float dot = (q.x * q.x + q.y * q.y) + (q.z * q.z + q.w * q.w);
        const float inv = 1.0f / sqrtf(dot);
        out[(P_ROT + 0) * N] = q.x * inv;
        out[(P_ROT + 1) * N] = q.y * inv;
        out[(P_ROT + 2) * N] = q.z * inv;
        out[(P_ROT + 3) * N] = q.w * inv;
    }
}

void launch_adam_step(const AdamStep& a, float* blob, uint32_t stride, uint32_t n, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_adam_step, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, a, blob, stride, n);
}

// mask[id] = the frame saw Gaussian id (its tiles_overlap is not 0), or that ORed into what mask[id] holds.
__global__ __launch_bounds__(BLOCK) void k_visible_mask(const uint32_t* __restrict__ tiles, uint8_t* __restrict__ mask, uint32_t n,
                                                        bool accumulate) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint8_t seen = tiles[i] != 0u ? 1 : 0;
    mask[i] = accumulate ? (uint8_t)(mask[i] | seen) : seen;
}

void launch_visible_mask(const uint32_t* tiles, uint8_t* mask, uint32_t n, bool accumulate, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_visible_mask, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, tiles, mask, n, accumulate);
}

}  // namespace gs
