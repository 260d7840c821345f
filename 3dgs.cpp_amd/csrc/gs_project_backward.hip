// gs_project_backward.hip -- k_project_backward: the projection half of the backward (gs_project_backward, gs3d_hip.h): from the
// float64 gradients with respect to a visible Gaussian's screen-space record (colour, opacity, conic, uv: what gs_blend_backward
// sums) to the gradients with respect to the six tensors Scene.to_tensors() returns -- means, log-scales, quaternions, opacity
// logits, SH DC and rest -- by the chain rule over the record function F the header writes down.  No reference counterpart.
//
// Part of libgs3d_hip.so (gfx950 only).  Built with -ffp-contract=off like every other unit.  The per-Gaussian chain -- the ONE
// binary32 computation that decides which branch of the Jacobian's clamp the frame took, and everything else in binary64 on exact
// conversions of the stored binary32 values and the frame's uniforms -- is gs_project_chain.h's project_chain and
// sh_direction_gradient, shared with k_camera_backward (gs_camera_backward.hip); the association is free (the contract is the
// bound tests/project_backward_reference.py derives), the formulas are that module's, node for node.
//
// SHAPE.  One lane per Gaussian in the order the frame read the scene: lane j reads slot j of the blob the frame rendered from (the
// copy in spatial order where there is one), and reads its inputs and writes its outputs under the scene id perm[j].  A lane whose
// Gaussian the frame culled (tiles_overlap == 0: the tap's answer) reads nothing more and writes nothing.
//   * The 48 SH coefficients are streamed once, never held: term j forms its basis value and the three partials with respect to the
//     view direction, reads its three coefficients, adds (dB_j/dd) * (sh_j . g_rgb) to the direction's gradient and puts
//     B_j * g_rgb down as d_sh[j].
//   * The outputs are rows of 8 to 360 bytes per Gaussian, strided by lane: each lane puts its 59 doubles (3 means, 3 log-scales,
//     4 quaternion, 1 logit, 48 SH) into LDS, and the wave then walks its visible Gaussians: for each, lane e reads element e of
//     the row and adds it to its place -- one read-modify-write of up to 59 consecutive doubles per output row instead of 59
//     strided ones per lane.  One writer per element: no atomics.  An exact zero is not added (a row element no gradient reaches
//     keeps its bits); a NaN is.
// Workgroup = one wave: 64 x 59 doubles = 30 208 bytes of LDS, five workgroups per CU.
// RESOURCES (tools/resource_usage.sh, profiles/camera_backward_resource_usage.txt): no scratch in either instantiation; the VGPR count
// is written down there and was not tuned for.
#include "gs_device.h"
#include "gs_project_chain.h"

namespace gs {

constexpr int kPbRow = 59;  // doubles per Gaussian in the stage: means 0..2, log-scales 3..5, quaternion 6..9, logit 10, SH 11..58

struct ProjectBackward {
    const float* blob;        // the blob the frame read (spatial copy or canonical), `stride` floats per plane
    const uint16_t* sh16;     // SH16 only: the binary16 SH block
    const uint32_t* perm;     // nullable: scene id of slot j
    const uint32_t* tiles;    // [n] by scene id: tiles_overlap of the frame
    const AttrRecord* rec;    // [n] by scene id: the frame's records (r > 0 decides whether channel 0 flows)
    uint32_t n, stride;
    int antialiased;
    gs_uniforms u;
    gs_project_grads g;
};

template <bool SH16>
__global__ __launch_bounds__(WAVE) void k_project_backward(ProjectBackward a) {
    __shared__ double s_row[WAVE * kPbRow];
    const uint32_t lane = threadIdx.x;
    const uint32_t j = blockIdx.x * WAVE + lane;
    const bool valid = j < a.n;
    const uint32_t oid = valid ? (a.perm ? a.perm[j] : j) : 0u;
    const bool vis = valid && a.tiles[oid] != 0u;
    const gs_uniforms& u = a.u;
    const gs_project_grads& g = a.g;

    if (vis) {
        ProjectChain k;
        project_chain(a.blob, a.stride, j, oid, u, a.antialiased, a.rec, g.d_colour, g.d_opacity, g.d_conic, g.d_uv, k);
        double* const row = s_row + lane * kPbRow;
#pragma unroll
        for (int c = 0; c < 3; ++c) row[3 + c] = k.d_ls[c];
#pragma unroll
        for (int c = 0; c < 4; ++c) row[6 + c] = k.d_q[c];
        row[10] = k.d_logit;
        // ---- rgb -> sh (row 11..58), and -> d -> p
        const float* const sh32 = a.blob + (size_t)P_SH * a.stride + (size_t)j * 48;
        const uint16_t* const sh_half = SH16 ? a.sh16 + (size_t)j * 48 : nullptr;
        double g_d[3];
        sh_direction_gradient<SH16, true>(sh32, sh_half, k.d, k.gcol, row + 11, g_d);
        const double dg = (k.d[0] * g_d[0] + k.d[1] * g_d[1]) + k.d[2] * g_d[2];
#pragma unroll
        for (int c = 0; c < 3; ++c) row[c] = k.g_p[c] + (g_d[c] - k.d[c] * dg) / k.len;
    }
    __syncthreads();  // (one wave: the rows are in LDS)

    // ---- the wave walks its visible Gaussians; lane e adds element e of the row to its place
    const uint32_t k3 = g.d_sh_rest ? 3u * g.sh_rest_coeffs : 0u;
    const uint32_t e = lane;
    for (uint64_t m = __ballot(vis); m != 0; m &= m - 1) {
        const int src = __ffsll((unsigned long long)m) - 1;
        const size_t id = (size_t)(uint32_t)__shfl((int)oid, src, WAVE);
        double* dst = nullptr;
        if (e < 3u) dst = g.d_means ? g.d_means + id * 3 + e : nullptr;
        else if (e < 6u) dst = g.d_log_scales ? g.d_log_scales + id * 3 + (e - 3u) : nullptr;
        else if (e < 10u) dst = g.d_quats ? g.d_quats + id * 4 + (e - 6u) : nullptr;
        else if (e == 10u) dst = g.d_opacity_logits ? g.d_opacity_logits + id : nullptr;
        else if (e < 14u) dst = g.d_sh_dc ? g.d_sh_dc + id * 3 + (e - 11u) : nullptr;
        else if (e - 14u < k3) dst = g.d_sh_rest + id * k3 + (e - 14u);  // (e <= 58: inside the row)
        if (dst) {
            const double v = s_row[src * kPbRow + e];
            if (v != 0.0) *dst = *dst + v;  // (true for a NaN)
        }
    }
}

void launch_project_backward(const SceneView& sv, const uint32_t* tiles, const AttrRecord* rec, const gs_uniforms& u, bool antialiased,
                             const gs_project_grads& g, hipStream_t s) {
    if (sv.n == 0) return;
    ProjectBackward a;
    a.blob = sv.blob, a.sh16 = sv.sh16, a.perm = sv.perm, a.tiles = tiles, a.rec = rec;
    a.n = sv.n, a.stride = sv.stride, a.antialiased = antialiased ? 1 : 0;
    a.u = u, a.g = g;
    const dim3 grid((sv.n + WAVE - 1) / WAVE);
    if (sv.sh16) hipLaunchKernelGGL((k_project_backward<true>), grid, dim3(WAVE), 0, s, a);
    else hipLaunchKernelGGL((k_project_backward<false>), grid, dim3(WAVE), 0, s, a);
}

}  // namespace gs
