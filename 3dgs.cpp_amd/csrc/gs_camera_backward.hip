// gs_camera_backward.hip -- k_camera_backward, k_camera_backward_finish: the camera half of the backward (gs_camera_backward,
// gs3d_hip.h): from the float64 gradients with respect to every visible Gaussian's screen-space record (what gs_blend_backward
// sums) to the gradients with respect to the frame's uniforms -- rows 0..2 of the view matrix, rows 0, 1, 3 of the projection
// matrix, the camera position: 27 sums over the visible Gaussians of the last frame.  No reference counterpart.
//
// Part of libgs3d_hip.so (gfx950 only), built with -ffp-contract=off.  The per-Gaussian chain is gs_project_chain.h's, the one
// k_project_backward evaluates; what is added here are the 27 terms a lane hangs off its nodes,
//     dV[r][c] = g_t[r] (p, 1)[c] + (r < 2 ? jaa[r] gA[r][c] : ja2[0] gA[0][c] + ja2[1] gA[1][c])   c < 3;    dV[r][3] = g_t[r]
//     dP[r][c] = g_h[r] (p, 1)[c]                                                                    r in 0, 1, 3
//     dc       = -(g_d - d (d . g_d)) / len
// and their reduction.  The SH coefficients are streamed for g_d alone: no d_sh is written.
//
// SHAPE.  kCamGroups workgroups of kCamThreads lanes at most, one lane per Gaussian in the order the frame read the scene (slot j of
// the blob, inputs under the scene id perm[j]), striding by the grid where the scene has more Gaussians than the launch has lanes
// (GS_CAMERA_BACKWARD_LANES).  A lane whose Gaussian the frame culled reads nothing more and adds nothing.
//   * a lane adds its visible Gaussians' terms into 27 binary64 registers, in the order it meets them;
//   * the wave sums each register over its lanes (wave_sum_f64: DPP within rows of 16, four lanes joined), the workgroup's waves
//     meet in 4 x 27 doubles of LDS and are added in wave order;
//   * the workgroup writes its row of 27 partials into a buffer the renderer owns, with ordinary vector stores;
//   * k_camera_backward_finish, one wave, lane e < 27: adds the rows in index order and adds the sum to its place in the caller's
//     arrays.  An exact zero is not added (the element keeps its bits); a NaN is.
// No atomics anywhere: the association is fixed by n and the launch geometry, so two calls give the same bits.
// RESOURCES (tools/resource_usage.sh, profiles/camera_backward_resource_usage.txt): no scratch; the VGPR count is written down there.
#include "gs_device.h"
#include "gs_project_chain.h"
#include "gs_wave_f64.h"

namespace gs {

constexpr int kCamTerms = 27;                                  // 12 of V (rows 0..2), 12 of P (rows 0, 1, 3), 3 of the position
constexpr int kCamThreads = 256;                               // four waves
constexpr int kCamGroups = GS_CAMERA_BACKWARD_LANES / kCamThreads;
static_assert(kCamGroups * kCamThreads == GS_CAMERA_BACKWARD_LANES, "the header states the launch's lanes");

size_t camera_backward_partials() { return (size_t)kCamGroups * kCamTerms; }

struct CameraBackward {
    const float* blob;        // the blob the frame read (spatial copy or canonical), `stride` floats per plane
    const uint16_t* sh16;     // SH16 only: the binary16 SH block
    const uint32_t* perm;     // nullable: scene id of slot j
    const uint32_t* tiles;    // [n] by scene id: tiles_overlap of the frame
    const AttrRecord* rec;    // [n] by scene id: the frame's records (r > 0 decides whether channel 0 flows)
    uint32_t n, stride;
    int antialiased;
    gs_uniforms u;
    const double *d_colour, *d_opacity, *d_conic, *d_uv;
    double* partials;         // [gridDim.x][kCamTerms]
};

template <bool SH16>
__global__ __launch_bounds__(kCamThreads) void k_camera_backward(CameraBackward a) {
    __shared__ double s_wave[kCamThreads / WAVE][kCamTerms];
    double acc[kCamTerms];
#pragma unroll
    for (int e = 0; e < kCamTerms; ++e) acc[e] = 0.0;

    for (uint32_t j = blockIdx.x * kCamThreads + threadIdx.x; j < a.n; j += gridDim.x * kCamThreads) {
        const uint32_t oid = a.perm ? a.perm[j] : j;
        if (a.tiles[oid] == 0u) continue;
        ProjectChain k;
        project_chain(a.blob, a.stride, j, oid, a.u, a.antialiased, a.rec, a.d_colour, a.d_opacity, a.d_conic, a.d_uv, k);
        const float* const sh32 = a.blob + (size_t)P_SH * a.stride + (size_t)j * 48;
        const uint16_t* const sh_half = SH16 ? a.sh16 + (size_t)j * 48 : nullptr;
        double g_d[3];
        sh_direction_gradient<SH16, false>(sh32, sh_half, k.d, k.gcol, nullptr, g_d);
        const double dg = (k.d[0] * g_d[0] + k.d[1] * g_d[1]) + k.d[2] * g_d[2];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            acc[0 * 4 + c] = acc[0 * 4 + c] + (k.g_t[0] * k.p[c] + k.jaa[0] * k.gA[0][c]);
            acc[1 * 4 + c] = acc[1 * 4 + c] + (k.g_t[1] * k.p[c] + k.jaa[1] * k.gA[1][c]);
            acc[2 * 4 + c] = acc[2 * 4 + c] + (k.g_t[2] * k.p[c] + (k.ja2[0] * k.gA[0][c] + k.ja2[1] * k.gA[1][c]));
#pragma unroll
            for (int r = 0; r < 3; ++r) acc[12 + r * 4 + c] = acc[12 + r * 4 + c] + k.g_h[r] * k.p[c];
            acc[24 + c] = acc[24 + c] + -((g_d[c] - k.d[c] * dg) / k.len);
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            acc[r * 4 + 3] = acc[r * 4 + 3] + k.g_t[r];
            acc[12 + r * 4 + 3] = acc[12 + r * 4 + 3] + k.g_h[r];
        }
    }
    // (the loop's lanes have met again: every lane of the wave is active for the DPP moves)
    const uint32_t wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
#pragma unroll
    for (int e = 0; e < kCamTerms; ++e) {
        const double s = wave_sum_f64(acc[e]);
        if (lane == 0) s_wave[wave][e] = s;
    }
    __syncthreads();
    if (threadIdx.x < kCamTerms) {
        const uint32_t e = threadIdx.x;
        a.partials[(size_t)blockIdx.x * kCamTerms + e] = ((s_wave[0][e] + s_wave[1][e]) + s_wave[2][e]) + s_wave[3][e];
    }
}

// Lane e adds rows 0 .. rows-1 of the partials in index order and adds the sum to its element: e < 12 is V[e / 4][e % 4],
// e < 24 is P[(0, 1, 3)[(e - 12) / 4]][e % 4], both stored column-major as the uniforms are; the last three are the position.
__global__ __launch_bounds__(WAVE) void k_camera_backward_finish(const double* __restrict__ partials, uint32_t rows, double* d_view_mat,
                                                                 double* d_proj_mat, double* d_camera_position) {
    const uint32_t e = threadIdx.x;
    if (e >= (uint32_t)kCamTerms) return;
    double sum = 0.0;
#pragma unroll 16
    for (uint32_t r = 0; r < rows; ++r) sum = sum + partials[(size_t)r * kCamTerms + e];
    double* dst;
    if (e < 12u) dst = d_view_mat ? d_view_mat + (e % 4u) * 4u + e / 4u : nullptr;
    else if (e < 24u) dst = d_proj_mat ? d_proj_mat + (e % 4u) * 4u + ((e - 12u) / 4u == 2u ? 3u : (e - 12u) / 4u) : nullptr;
    else dst = d_camera_position ? d_camera_position + (e - 24u) : nullptr;
    if (dst && sum != 0.0) *dst = *dst + sum;  // (true for a NaN)
}

void launch_camera_backward(const SceneView& sv, const uint32_t* tiles, const AttrRecord* rec, const gs_uniforms& u, bool antialiased,
                            const gs_camera_grads& g, double* partials, hipStream_t s) {
    if (sv.n == 0) return;
    CameraBackward a;
    a.blob = sv.blob, a.sh16 = sv.sh16, a.perm = sv.perm, a.tiles = tiles, a.rec = rec;
    a.n = sv.n, a.stride = sv.stride, a.antialiased = antialiased ? 1 : 0;
    a.u = u;
    a.d_colour = g.d_colour, a.d_opacity = g.d_opacity, a.d_conic = g.d_conic, a.d_uv = g.d_uv;
    a.partials = partials;
    const uint32_t groups = (uint32_t)std::min<uint64_t>(((uint64_t)sv.n + kCamThreads - 1) / kCamThreads, (uint64_t)kCamGroups);
    if (sv.sh16) hipLaunchKernelGGL((k_camera_backward<true>), dim3(groups), dim3(kCamThreads), 0, s, a);
    else hipLaunchKernelGGL((k_camera_backward<false>), dim3(groups), dim3(kCamThreads), 0, s, a);
    hipLaunchKernelGGL(k_camera_backward_finish, dim3(1), dim3(WAVE), 0, s, partials, groups, g.d_view_mat, g.d_proj_mat, g.d_camera_position);
}

}  // namespace gs
