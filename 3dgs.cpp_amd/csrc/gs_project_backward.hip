// gs_project_backward.hip -- k_project_backward: the projection half of the backward (gs_project_backward, gs3d_hip.h): from the
// float64 gradients with respect to a visible Gaussian's screen-space record (colour, opacity, conic, uv: what gs_blend_backward
// sums) to the gradients with respect to the six tensors Scene.to_tensors() returns -- means, log-scales, quaternions, opacity
// logits, SH DC and rest -- by the chain rule over the record function F the header writes down.  No reference counterpart.
//
// Part of libgs3d_hip.so (gfx950 only).  Built with -ffp-contract=off like every other unit: the ONE binary32 computation in here
// -- the p_view rows and the division that decide which branch of the Jacobian's clamp the frame took -- restates
// gs_preprocess.hip:137-166 with the same operations in the same order, so the decision is the frame's.  Everything else is
// binary64 on exact conversions of the stored binary32 values and the frame's uniforms; the association is free (the contract is
// the bound tests/project_backward_reference.py derives), the formulas are that module's, node for node.
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
// RESOURCES (tools/resource_usage.sh, profiles/r22_kernel_resource_usage.txt): no scratch in either instantiation; the VGPR count
// is written down there and was not tuned for.
#include "gs_device.h"

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
        const size_t N = a.stride;
        const float* __restrict__ blob = a.blob;
        const float pxf = blob[(P_POS + 0) * N + j], pyf = blob[(P_POS + 1) * N + j], pzf = blob[(P_POS + 2) * N + j];
        // ---- the clamp's branch, in binary32 as the frame took it (gs_preprocess.hip:137-166)
        float p_view[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            float s = u.view_mat[0 * 4 + r] * pxf;
            s = s + u.view_mat[1 * 4 + r] * pyf;
            s = s + u.view_mat[2 * 4 + r] * pzf;
            s = s + u.view_mat[3 * 4 + r] * 1.0f;
            p_view[r] = s;
        }
        const float limx = 1.3f * u.tan_fovx;
        const float limy = 1.3f * u.tan_fovy;
        const float txtz = p_view[0] / p_view[2];
        const float tytz = p_view[1] / p_view[2];
        const float cxf = fminf(limx, fmaxf(-limx, txtz));
        const float cyf = fminf(limy, fmaxf(-limy, tytz));
        const bool bind[2] = {!(cxf == txtz), !(cyf == tytz)};
        const double cc[2] = {(double)cxf, (double)cyf};

        // ---- inputs (a NULL array = zeros); channel 0 flows iff the record holds r > 0
        double gcol[3] = {0.0, 0.0, 0.0}, gop = 0.0, gcon[3] = {0.0, 0.0, 0.0}, guv[2] = {0.0, 0.0};
        if (g.d_colour) {
#pragma unroll
            for (int k = 0; k < 3; ++k) gcol[k] = g.d_colour[(size_t)oid * 3 + k];
        }
        if (g.d_opacity) gop = g.d_opacity[oid];
        if (g.d_conic) {
#pragma unroll
            for (int k = 0; k < 3; ++k) gcon[k] = g.d_conic[(size_t)oid * 3 + k];
        }
        if (g.d_uv) {
            guv[0] = g.d_uv[(size_t)oid * 2 + 0];
            guv[1] = g.d_uv[(size_t)oid * 2 + 1];
        }
        if (!(a.rec[oid].uv_rg.z > 0.0f)) gcol[0] = 0.0;  // selected, never multiplied by zero

        const double p[3] = {(double)pxf, (double)pyf, (double)pzf};
        double s[3], q[4];
#pragma unroll
        for (int k = 0; k < 3; ++k) s[k] = (double)blob[(P_SCALE + k) * N + j];
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = (double)blob[(P_ROT + k) * N + j];
        const double o = (double)blob[(size_t)P_OPACITY * N + j];
#define GS_P(r, c) ((double)u.proj_mat[(c) * 4 + (r)])
#define GS_V(r, c) ((double)u.view_mat[(c) * 4 + (r)])
        const double W = (double)u.width, H = (double)u.height;

        // ---- forward
        double h[4], t[3];
#pragma unroll
        for (int r = 0; r < 4; ++r) h[r] = ((p[0] * GS_P(r, 0) + p[1] * GS_P(r, 1)) + p[2] * GS_P(r, 2)) + GS_P(r, 3);
#pragma unroll
        for (int r = 0; r < 3; ++r) t[r] = ((p[0] * GS_V(r, 0) + p[1] * GS_V(r, 1)) + p[2] * GS_V(r, 2)) + GS_V(r, 3);
        const double f[2] = {W / (2.0 * (double)u.tan_fovx), H / (2.0 * (double)u.tan_fovy)};
        const double t2sq = t[2] * t[2];
        double jaa[2], ja2[2], A[2][3];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            jaa[i] = f[i] / t[2];
            ja2[i] = bind[i] ? -(f[i] * cc[i]) / t[2] : -(f[i] * t[i]) / t2sq;
#pragma unroll
            for (int c = 0; c < 3; ++c) A[i][c] = jaa[i] * GS_V(i, c) + ja2[i] * GS_V(2, c);
        }
        const double nrm = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
        const double qw = q[0] / nrm, qx = q[1] / nrm, qy = q[2] / nrm, qz = q[3] / nrm;
        double R[3][3];
        R[0][0] = 1.0 - 2.0 * (qy * qy + qz * qz);
        R[0][1] = 2.0 * (qx * qy - qz * qw);
        R[0][2] = 2.0 * (qx * qz + qy * qw);
        R[1][0] = 2.0 * (qx * qy + qz * qw);
        R[1][1] = 1.0 - 2.0 * (qx * qx + qz * qz);
        R[1][2] = 2.0 * (qy * qz - qx * qw);
        R[2][0] = 2.0 * (qx * qz - qy * qw);
        R[2][1] = 2.0 * (qy * qz + qx * qw);
        R[2][2] = 1.0 - 2.0 * (qx * qx + qy * qy);
        double M[2][3], s2[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            s2[k] = s[k] * s[k];
#pragma unroll
            for (int i = 0; i < 2; ++i) M[i][k] = (A[i][0] * R[0][k] + A[i][1] * R[1][k]) + A[i][2] * R[2][k];
        }
        const double cov00 = (M[0][0] * M[0][0] * s2[0] + M[0][1] * M[0][1] * s2[1]) + M[0][2] * M[0][2] * s2[2];
        const double cov01 = (M[0][0] * M[1][0] * s2[0] + M[0][1] * M[1][1] * s2[1]) + M[0][2] * M[1][2] * s2[2];
        const double cov11 = (M[1][0] * M[1][0] * s2[0] + M[1][1] * M[1][1] * s2[1]) + M[1][2] * M[1][2] * s2[2];
        const double dil = (double)0.3f;
        const double m00 = cov00 + dil, m11 = cov11 + dil, m01 = cov01;
        const double det = m00 * m11 - m01 * m01;
        const double c00 = m11 / det, c01 = -m01 / det, c11 = m00 / det;

        // ---- conic (and comp, antialiased frames) -> cov
        double g_det = -(((gcon[0] * c00 + gcon[1] * c01) + gcon[2] * c11) / det);
        double g_o = gop, g_detraw = 0.0;
        bool comp_flows = false;
        if (a.antialiased) {
            const double det_raw = cov00 * cov11 - cov01 * cov01;
            comp_flows = det_raw > 0.0;
            g_o = 0.0;  // det_raw <= 0: comp is the constant 0
            if (comp_flows) {
                const double comp = sqrt(det_raw / det);
                const double g_comp = gop * o;
                g_o = gop * comp;
                g_detraw = (0.5 * g_comp) / (comp * det);
                g_det = g_det + -(0.5 * (g_comp * comp)) / det;
            }
        }
        double g_m00 = gcon[2] / det + g_det * m11;
        double g_m11 = gcon[0] / det + g_det * m00;
        double g_m01 = -(gcon[1] / det) - 2.0 * (g_det * m01);
        if (comp_flows) {
            g_m00 = g_m00 + g_detraw * cov11;
            g_m11 = g_m11 + g_detraw * cov00;
            g_m01 = g_m01 - 2.0 * (g_detraw * cov01);
        }
        // ---- cov -> M, s^2;  M = A R -> A, R
        double gM[2][3], d_ls[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            gM[0][k] = (2.0 * (g_m00 * M[0][k]) + g_m01 * M[1][k]) * s2[k];
            gM[1][k] = (2.0 * (g_m11 * M[1][k]) + g_m01 * M[0][k]) * s2[k];
            const double g_s2 = (g_m00 * (M[0][k] * M[0][k]) + g_m01 * (M[0][k] * M[1][k])) + g_m11 * (M[1][k] * M[1][k]);
            d_ls[k] = 2.0 * (g_s2 * s2[k]);
        }
        double gA[2][3], gR[3][3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
            for (int i = 0; i < 2; ++i) gA[i][c] = (gM[i][0] * R[c][0] + gM[i][1] * R[c][1]) + gM[i][2] * R[c][2];
#pragma unroll
            for (int k = 0; k < 3; ++k) gR[c][k] = A[0][c] * gM[0][k] + A[1][c] * gM[1][k];
        }
        // ---- A = J V -> J -> t -> p
        const double t2cu = t2sq * t[2];
        double g_t[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const double g_jaa = (gA[i][0] * GS_V(i, 0) + gA[i][1] * GS_V(i, 1)) + gA[i][2] * GS_V(i, 2);
            const double g_ja2 = (gA[i][0] * GS_V(2, 0) + gA[i][1] * GS_V(2, 1)) + gA[i][2] * GS_V(2, 2);
            g_t[i] = bind[i] ? 0.0 : -(g_ja2 * f[i]) / t2sq;
            // where the clamp binds tx = c t2 is still a function of t2: J02 = -f c / t2
            const double through = bind[i] ? ((g_ja2 * f[i]) * cc[i]) / t2sq : (2.0 * ((g_ja2 * f[i]) * t[i])) / t2cu;
            g_t[2] = (g_t[2] + -(g_jaa * f[i]) / t2sq) + through;
        }
        double g_p[3];
        const double h3sq = h[3] * h[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            g_p[c] = (g_t[0] * GS_V(0, c) + g_t[1] * GS_V(1, c)) + g_t[2] * GS_V(2, c);
            const double du = (GS_P(0, c) / h[3] - (h[0] * GS_P(3, c)) / h3sq) * (W / 2.0);
            const double dv = (GS_P(1, c) / h[3] - (h[1] * GS_P(3, c)) / h3sq) * (H / 2.0);
            g_p[c] = (g_p[c] + guv[0] * du) + guv[1] * dv;
        }
        // ---- R -> q^ -> q: the tangent projection, over the stored quaternion's own norm
        double g_qh[4];
        g_qh[0] = 2.0 * (((((-(qz * gR[0][1]) + qy * gR[0][2]) + qz * gR[1][0]) - qx * gR[1][2]) - qy * gR[2][0]) + qx * gR[2][1]);
        g_qh[1] = 2.0 * (((((((-2.0 * (qx * gR[1][1]) - 2.0 * (qx * gR[2][2])) + qy * gR[0][1]) + qz * gR[0][2]) + qy * gR[1][0]) - qw * gR[1][2]) +
                          qz * gR[2][0]) + qw * gR[2][1]);
        g_qh[2] = 2.0 * (((((((-2.0 * (qy * gR[0][0]) - 2.0 * (qy * gR[2][2])) + qx * gR[0][1]) + qw * gR[0][2]) + qx * gR[1][0]) + qz * gR[1][2]) -
                          qw * gR[2][0]) + qz * gR[2][1]);
        g_qh[3] = 2.0 * (((((((-2.0 * (qz * gR[0][0]) - 2.0 * (qz * gR[1][1])) - qw * gR[0][1]) + qx * gR[0][2]) + qw * gR[1][0]) + qy * gR[1][2]) +
                          qx * gR[2][0]) + qy * gR[2][1]);
        const double qh[4] = {qw, qx, qy, qz};
        const double qdot = ((qh[0] * g_qh[0] + qh[1] * g_qh[1]) + qh[2] * g_qh[2]) + qh[3] * g_qh[3];

        double* const row = s_row + lane * kPbRow;
#pragma unroll
        for (int k = 0; k < 3; ++k) row[3 + k] = d_ls[k];
#pragma unroll
        for (int k = 0; k < 4; ++k) row[6 + k] = (g_qh[k] - qh[k] * qdot) / nrm;
        row[10] = g_o * (o * (1.0 - o));

        // ---- rgb -> sh, and -> d -> p.  The basis polynomials and constants of sh_to_rgb (gs_preprocess.hip), the constants
        // converted exactly; x, y, z independent variables, the normalisation behind them.
        const double rel[3] = {p[0] - (double)u.camera_position[0], p[1] - (double)u.camera_position[1], p[2] - (double)u.camera_position[2]};
        const double len = sqrt((rel[0] * rel[0] + rel[1] * rel[1]) + rel[2] * rel[2]);
        const double x = rel[0] / len, y = rel[1] / len, z = rel[2] / len;
        const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
        const double C0 = (double)0.28209479177387814f, C1 = (double)0.4886025119029199f;
        const double C2_0 = (double)1.0925484305920792f, C2_1 = (double)-1.0925484305920792f, C2_2 = (double)0.31539156525252005f,
                     C2_3 = (double)-1.0925484305920792f, C2_4 = (double)0.5462742152960396f;
        const double C3_0 = (double)-0.5900435899266435f, C3_1 = (double)2.890611442640554f, C3_2 = (double)-0.4570457994644658f,
                     C3_3 = (double)0.3731763325901154f, C3_4 = (double)-0.4570457994644658f, C3_5 = (double)1.445305721320277f,
                     C3_6 = (double)-0.5900435899266435f;
        const float* const sh32 = blob + (size_t)P_SH * N + (size_t)j * 48;
        const uint16_t* const sh_half = SH16 ? a.sh16 + (size_t)j * 48 : nullptr;
        double g_d[3] = {0.0, 0.0, 0.0};
        // term J: its basis value B and partials (BX, BY, BZ); the three coefficients are read here and nowhere else
#define GS_SH_TERM(J, B, BX, BY, BZ)                                                                                              \
    {                                                                                                                             \
        const double b_ = (B);                                                                                                    \
        double c_[3];                                                                                                             \
        _Pragma("unroll") for (int k = 0; k < 3; ++k) {                                                                           \
            c_[k] = SH16 ? (double)__half2float(__ushort_as_half(sh_half[(J) * 3 + k])) : (double)sh32[(J) * 3 + k];              \
            row[11 + (J) * 3 + k] = b_ * gcol[k];                                                                                 \
        }                                                                                                                         \
        const double S_ = (c_[0] * gcol[0] + c_[1] * gcol[1]) + c_[2] * gcol[2];                                                  \
        g_d[0] = g_d[0] + (BX) * S_;                                                                                              \
        g_d[1] = g_d[1] + (BY) * S_;                                                                                              \
        g_d[2] = g_d[2] + (BZ) * S_;                                                                                              \
    }
        GS_SH_TERM(0, C0, 0.0, 0.0, 0.0)
        GS_SH_TERM(1, -C1 * y, 0.0, -C1, 0.0)
        GS_SH_TERM(2, C1 * z, 0.0, 0.0, C1)
        GS_SH_TERM(3, -C1 * x, -C1, 0.0, 0.0)
        GS_SH_TERM(4, C2_0 * xy, C2_0 * y, C2_0 * x, 0.0)
        GS_SH_TERM(5, C2_1 * yz, 0.0, C2_1 * z, C2_1 * y)
        GS_SH_TERM(6, C2_2 * ((2.0 * zz - xx) - yy), -2.0 * (C2_2 * x), -2.0 * (C2_2 * y), 4.0 * (C2_2 * z))
        GS_SH_TERM(7, C2_3 * xz, C2_3 * z, 0.0, C2_3 * x)
        GS_SH_TERM(8, C2_4 * (xx - yy), 2.0 * (C2_4 * x), -2.0 * (C2_4 * y), 0.0)
        GS_SH_TERM(9, C3_0 * ((3.0 * xx - yy) * y), (6.0 * C3_0) * xy, C3_0 * (3.0 * xx - 3.0 * yy), 0.0)
        GS_SH_TERM(10, C3_1 * (xy * z), C3_1 * yz, C3_1 * xz, C3_1 * xy)
        GS_SH_TERM(11, C3_2 * (((4.0 * zz - xx) - yy) * y), -2.0 * (C3_2 * xy), C3_2 * ((4.0 * zz - xx) - 3.0 * yy), 8.0 * (C3_2 * yz))
        GS_SH_TERM(12, C3_3 * (z * ((2.0 * zz - 3.0 * xx) - 3.0 * yy)), (-6.0 * C3_3) * xz, (-6.0 * C3_3) * yz, C3_3 * ((6.0 * zz - 3.0 * xx) - 3.0 * yy))
        GS_SH_TERM(13, C3_4 * (x * ((4.0 * zz - xx) - yy)), C3_4 * ((4.0 * zz - 3.0 * xx) - yy), -2.0 * (C3_4 * xy), 8.0 * (C3_4 * xz))
        GS_SH_TERM(14, C3_5 * ((xx - yy) * z), 2.0 * (C3_5 * xz), -2.0 * (C3_5 * yz), C3_5 * (xx - yy))
        GS_SH_TERM(15, C3_6 * (x * (xx - 3.0 * yy)), C3_6 * (3.0 * xx - 3.0 * yy), (-6.0 * C3_6) * xy, 0.0)
#undef GS_SH_TERM
        const double d[3] = {x, y, z};
        const double dg = (d[0] * g_d[0] + d[1] * g_d[1]) + d[2] * g_d[2];
#pragma unroll
        for (int c = 0; c < 3; ++c) row[c] = g_p[c] + (g_d[c] - d[c] * dg) / len;
#undef GS_P
#undef GS_V
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
