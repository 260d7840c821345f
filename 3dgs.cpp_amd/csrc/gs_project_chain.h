// gs_project_chain.h -- the per-Gaussian chain of the projection's backward, shared by k_project_backward (gs_project_backward.hip)
// and k_camera_backward (gs_camera_backward.hip): from the four input gradients of one visible Gaussian (colour, opacity, conic, uv)
// through the record function F of gs3d_hip.h, node by node, to everything either kernel hangs its outputs off -- g_t, gA, the
// Jacobian's entries, g_p, the log-scales', the quaternion's and the logit's gradients, the view direction -- and the one stream
// over the SH coefficients (sh_direction_gradient: the GS_SH_TERM table, its row store optional).  The mathematics is stated HERE
// and nowhere else; the formulas are tests/project_backward_reference.py's, node for node.
//
// Device code, built with -ffp-contract=off like every unit that includes it: the ONE binary32 computation -- the p_view rows and
// the division that decide which branch of the Jacobian's clamp the frame took -- restates gs_preprocess.hip:137-166 with the same
// operations in the same order, so the decision is the frame's.  Everything else is binary64 on exact conversions of the stored
// binary32 values and the frame's uniforms.  Both functions are forced inline: what a kernel does not read of the struct is never
// computed.
#pragma once
#include "gs_device.h"

namespace gs {

struct ProjectChain {
    double p[3];          // the stored position, converted exactly
    double gcol[3];       // the colour's input gradient, channel 0 selected away where the record holds r == 0
    double jaa[2], ja2[2];  // J[i][i] and J[i][2] as the frame's clamp branches give them
    double gA[2][3];      // dL/dA, A = J V(3x3)
    double g_t[3];        // dL/dt through the covariance (uv does not pass t)
    double g_h[3];        // dL/dh rows 0, 1, 3 through uv
    double g_p[3];        // dL/dp through t and h (the view direction's part is added by the caller, behind the SH stream)
    double d_ls[3];       // dL/d(log s)
    double d_q[4];        // dL/dq: the tangent projection over the stored quaternion's own norm
    double d_logit;       // dL/d(opacity logit)
    double d[3], len;     // the view direction (p - camera_position) / len
};

#define GS_P(r, c) ((double)u.proj_mat[(c) * 4 + (r)])
#define GS_V(r, c) ((double)u.view_mat[(c) * 4 + (r)])

// Slot j of `blob` (stride N floats per plane), scene id oid; the four input arrays are gs_project_grads' (a NULL array = zeros).
__device__ __forceinline__ void project_chain(const float* __restrict__ blob, size_t N, uint32_t j, uint32_t oid, const gs_uniforms& u,
                                              int antialiased, const AttrRecord* rec, const double* d_colour, const double* d_opacity,
                                              const double* d_conic, const double* d_uv, ProjectChain& k) {
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
    if (d_colour) {
#pragma unroll
        for (int c = 0; c < 3; ++c) gcol[c] = d_colour[(size_t)oid * 3 + c];
    }
    if (d_opacity) gop = d_opacity[oid];
    if (d_conic) {
#pragma unroll
        for (int c = 0; c < 3; ++c) gcon[c] = d_conic[(size_t)oid * 3 + c];
    }
    if (d_uv) {
        guv[0] = d_uv[(size_t)oid * 2 + 0];
        guv[1] = d_uv[(size_t)oid * 2 + 1];
    }
    if (!(rec[oid].uv_rg.z > 0.0f)) gcol[0] = 0.0;  // selected, never multiplied by zero
#pragma unroll
    for (int c = 0; c < 3; ++c) k.gcol[c] = gcol[c];

    const double p[3] = {(double)pxf, (double)pyf, (double)pzf};
    double s[3], q[4];
#pragma unroll
    for (int c = 0; c < 3; ++c) s[c] = (double)blob[(P_SCALE + c) * N + j];
#pragma unroll
    for (int c = 0; c < 4; ++c) q[c] = (double)blob[(P_ROT + c) * N + j];
    const double o = (double)blob[(size_t)P_OPACITY * N + j];
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
    for (int c = 0; c < 3; ++c) {
        s2[c] = s[c] * s[c];
#pragma unroll
        for (int i = 0; i < 2; ++i) M[i][c] = (A[i][0] * R[0][c] + A[i][1] * R[1][c]) + A[i][2] * R[2][c];
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
    if (antialiased) {
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
    double gM[2][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        gM[0][c] = (2.0 * (g_m00 * M[0][c]) + g_m01 * M[1][c]) * s2[c];
        gM[1][c] = (2.0 * (g_m11 * M[1][c]) + g_m01 * M[0][c]) * s2[c];
        const double g_s2 = (g_m00 * (M[0][c] * M[0][c]) + g_m01 * (M[0][c] * M[1][c])) + g_m11 * (M[1][c] * M[1][c]);
        k.d_ls[c] = 2.0 * (g_s2 * s2[c]);
    }
    double gA[2][3], gR[3][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int i = 0; i < 2; ++i) gA[i][c] = (gM[i][0] * R[c][0] + gM[i][1] * R[c][1]) + gM[i][2] * R[c][2];
#pragma unroll
        for (int e = 0; e < 3; ++e) gR[c][e] = A[0][c] * gM[0][e] + A[1][c] * gM[1][e];
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
    const double h3sq = h[3] * h[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double g_p = (g_t[0] * GS_V(0, c) + g_t[1] * GS_V(1, c)) + g_t[2] * GS_V(2, c);
        const double du = (GS_P(0, c) / h[3] - (h[0] * GS_P(3, c)) / h3sq) * (W / 2.0);
        const double dv = (GS_P(1, c) / h[3] - (h[1] * GS_P(3, c)) / h3sq) * (H / 2.0);
        k.g_p[c] = (g_p + guv[0] * du) + guv[1] * dv;
    }
    // the same two rows of d(u, v)/dh, contracted with the input instead of with P: dL/dh
    k.g_h[0] = (guv[0] * (W / 2.0)) / h[3];
    k.g_h[1] = (guv[1] * (H / 2.0)) / h[3];
    k.g_h[2] = -(((guv[0] * (W / 2.0)) * h[0] + (guv[1] * (H / 2.0)) * h[1]) / h3sq);
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
#pragma unroll
    for (int c = 0; c < 4; ++c) k.d_q[c] = (g_qh[c] - qh[c] * qdot) / nrm;
    k.d_logit = g_o * (o * (1.0 - o));

    // ---- the view direction
    const double rel[3] = {p[0] - (double)u.camera_position[0], p[1] - (double)u.camera_position[1], p[2] - (double)u.camera_position[2]};
    k.len = sqrt((rel[0] * rel[0] + rel[1] * rel[1]) + rel[2] * rel[2]);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        k.d[c] = rel[c] / k.len;
        k.p[c] = p[c];
        k.g_t[c] = g_t[c];
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        k.jaa[i] = jaa[i];
        k.ja2[i] = ja2[i];
#pragma unroll
        for (int c = 0; c < 3; ++c) k.gA[i][c] = gA[i][c];
    }
}

#undef GS_P
#undef GS_V

// rgb -> sh, and -> d.  The basis polynomials and constants of sh_to_rgb (gs_preprocess.hip), the constants converted exactly;
// x, y, z independent variables, the normalisation behind them.  The 48 coefficients of slot j are streamed once, never held:
// term J forms its basis value and the three partials with respect to the view direction, reads its three coefficients and adds
// (dB_J/dd) * (sh_J . gcol) to g_d.  STORE: B_J * gcol is put down as d_sh[J] at sh_row[3 J + channel] (k_project_backward's LDS
// row); k_camera_backward writes no d_sh and passes nullptr.
template <bool SH16, bool STORE>
__device__ __forceinline__ void sh_direction_gradient(const float* sh32, const uint16_t* sh_half, const double (&dir)[3],
                                                      const double (&gcol)[3], double* sh_row, double (&g_d)[3]) {
    const double x = dir[0], y = dir[1], z = dir[2];
    const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
    const double C0 = (double)0.28209479177387814f, C1 = (double)0.4886025119029199f;
    const double C2_0 = (double)1.0925484305920792f, C2_1 = (double)-1.0925484305920792f, C2_2 = (double)0.31539156525252005f,
                 C2_3 = (double)-1.0925484305920792f, C2_4 = (double)0.5462742152960396f;
    const double C3_0 = (double)-0.5900435899266435f, C3_1 = (double)2.890611442640554f, C3_2 = (double)-0.4570457994644658f,
                 C3_3 = (double)0.3731763325901154f, C3_4 = (double)-0.4570457994644658f, C3_5 = (double)1.445305721320277f,
                 C3_6 = (double)-0.5900435899266435f;
    g_d[0] = g_d[1] = g_d[2] = 0.0;
    // term J: its basis value B and partials (BX, BY, BZ); the three coefficients are read here and nowhere else
#define GS_SH_TERM(J, B, BX, BY, BZ)                                                                                              \
    {                                                                                                                             \
        const double b_ = (B);                                                                                                    \
        double c_[3];                                                                                                             \
        _Pragma("unroll") for (int k = 0; k < 3; ++k) {                                                                           \
            c_[k] = SH16 ? (double)__half2float(__ushort_as_half(sh_half[(J) * 3 + k])) : (double)sh32[(J) * 3 + k];              \
            if (STORE) sh_row[(J) * 3 + k] = b_ * gcol[k];                                                                        \
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
}

}  // namespace gs
