// gs_sh_rotation.h -- the host arithmetic of gs_scene_transform (include/gs3d_hip.h): from a gs_transform the rotation matrix R,
// the three matrices M_1 (3 x 3), M_2 (5 x 5), M_3 (7 x 7) that rotate the SH bands with it, and the camera that goes with the
// transformed scene.  Everything is evaluated in binary64 and rounded ONCE to binary32.  Plain C++ without a device in sight:
// tests/test_scene_transform_api.py drives it through the C ABI on the CPU, tests/native/sh_rotation_sim.cpp stand-alone.
//
// M_l is DEFINED by the renderer's own basis, not by a textbook's (whose signs and order differ): with Y_j the 2l + 1 functions
// that k_preprocess's sh_to_rgb multiplies the coefficients of band l with (sh_band_basis below restates them, constants as
// the binary32 values the kernel holds), f(d) = sum_j c_j Y_j(d), the rotated colour function is f'(d) = f(R^T d), and
//     sum_j c'_j Y_j(d) = sum_j c_j Y_j(R^T d)  for every unit d      <=>      c' = M_l c,   Y(d)^T M_l = Y(R^T d)^T.
// The band is closed under rotation, so the system has an exact solution; it is solved in the least-squares sense over kDirs
// fixed directions of a Fibonacci spiral (A M = B with A_ij = Y_j(d_i), B_ij = Y_j(R^T d_i), by the normal equations: A^T A is
// K / 4 pi times the identity to a few per cent for these directions, condition number 1.0).  The solve's error is ~1e-15; an
// entry below kNoise in magnitude is that error around an exact zero and is returned as zero, so that a rotation about an axis --
// the identity included -- gives the zeros its matrices have, and the identity gives identity matrices exactly.
#pragma once

#include <cmath>
#include <cstdint>

#include "../../include/gs3d_hip.h"

namespace gs_host {

constexpr int kShMatrixFloats = 9 + 25 + 49;                 // gs_transform_sh_matrices: M_1, M_2, M_3, row-major, back to back
constexpr int kShMatrixOffset[4] = {0, 0, 9, 9 + 25};        // of band l
constexpr int kShRotationDirs = 64;
constexpr double kShRotationNoise = 1e-12;

// the functions sh_to_rgb (gs_preprocess.hip) multiplies coefficients 1..3, 4..8, 9..15 with, in its order and with its signs
inline void sh_band_basis(int l, double x, double y, double z, double* Y) {
    const double C1 = 0.4886025119029199f;
    const double C2_0 = 1.0925484305920792f, C2_1 = -1.0925484305920792f, C2_2 = 0.31539156525252005f, C2_3 = -1.0925484305920792f,
                 C2_4 = 0.5462742152960396f;
    const double C3_0 = -0.5900435899266435f, C3_1 = 2.890611442640554f, C3_2 = -0.4570457994644658f, C3_3 = 0.3731763325901154f,
                 C3_4 = -0.4570457994644658f, C3_5 = 1.445305721320277f, C3_6 = -0.5900435899266435f;
    if (l == 1) {
        Y[0] = -C1 * y;
        Y[1] = C1 * z;
        Y[2] = -C1 * x;
    } else if (l == 2) {
        Y[0] = C2_0 * x * y;
        Y[1] = C2_1 * y * z;
        Y[2] = C2_2 * (2.0 * z * z - x * x - y * y);
        Y[3] = C2_3 * z * x;
        Y[4] = C2_4 * (x * x - y * y);
    } else {
        Y[0] = C3_0 * (3.0 * x * x - y * y) * y;
        Y[1] = C3_1 * x * y * z;
        Y[2] = C3_2 * (4.0 * z * z - x * x - y * y) * y;
        Y[3] = C3_3 * z * (2.0 * z * z - 3.0 * x * x - 3.0 * y * y);
        Y[4] = C3_4 * x * (4.0 * z * z - x * x - y * y);
        Y[5] = C3_5 * (x * x - y * y) * z;
        Y[6] = C3_6 * x * (x * x - 3.0 * y * y);
    }
}

// What gs_scene_transform / gs_transform_sh_matrices / gs_transform_camera refuse in a transform: the message, or nullptr.
inline const char* transform_fault(const gs_transform* t) {
    if (!t) return "null argument";
    if (!std::isfinite(t->scale) || !(t->scale > 0.0f)) return "transform: scale must be finite and > 0";
    for (float v : t->translation)
        if (!std::isfinite(v)) return "transform: translation is not finite";
    double n2 = 0.0;
    for (float v : t->rotation) {
        if (!std::isfinite(v)) return "transform: rotation quaternion is not finite";
        n2 += static_cast<double>(v) * v;
    }
    if (!(n2 > 0.0)) return "transform: rotation quaternion has zero norm";
    return nullptr;
}

// the quaternion normalised in binary64 (w x y z) and R = the rotation it stands for, row-major: (R v)_i = sum_j R[3 i + j] v_j
inline void rotation_of(const gs_transform& t, double q[4], double R[9]) {
    double n2 = 0.0;
    for (float v : t.rotation) n2 += static_cast<double>(v) * v;
    const double inv = 1.0 / std::sqrt(n2);
    for (int k = 0; k < 4; ++k) q[k] = t.rotation[k] * inv;
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    R[0] = 1 - 2 * (y * y + z * z);
    R[1] = 2 * (x * y - z * w);
    R[2] = 2 * (x * z + y * w);
    R[3] = 2 * (x * y + z * w);
    R[4] = 1 - 2 * (x * x + z * z);
    R[5] = 2 * (y * z - x * w);
    R[6] = 2 * (x * z - y * w);
    R[7] = 2 * (y * z + x * w);
    R[8] = 1 - 2 * (x * x + y * y);
}

// Hamilton product a (x) b, w x y z
inline void quat_mul(const double a[4], const double b[4], double o[4]) {
    o[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
    o[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
    o[2] = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
    o[3] = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
}

// M_l of the rotation R (binary64, row-major m x m with m = 2 l + 1): see the head of this file
inline void sh_band_matrix(int l, const double R[9], double* M) {
    constexpr int K = kShRotationDirs;
    const int m = 2 * l + 1;
    double G[7][7] = {}, H[7][7] = {};  // A^T A, A^T B
    const double golden = 3.14159265358979323846 * (3.0 - std::sqrt(5.0));
    for (int i = 0; i < K; ++i) {
        const double z = 1.0 - (2.0 * i + 1.0) / K, r = std::sqrt(1.0 - z * z), phi = golden * i;
        const double d[3] = {r * std::cos(phi), r * std::sin(phi), z};
        const double e[3] = {R[0] * d[0] + R[3] * d[1] + R[6] * d[2], R[1] * d[0] + R[4] * d[1] + R[7] * d[2],
                             R[2] * d[0] + R[5] * d[1] + R[8] * d[2]};  // R^T d
        double a[7], b[7];
        sh_band_basis(l, d[0], d[1], d[2], a);
        sh_band_basis(l, e[0], e[1], e[2], b);
        for (int p = 0; p < m; ++p)
            for (int q = 0; q < m; ++q) {
                G[p][q] += a[p] * a[q];
                H[p][q] += a[p] * b[q];
            }
    }
    // G M = H: elimination with partial pivoting, all right-hand sides at once
    for (int c = 0; c < m; ++c) {
        int piv = c;
        for (int r = c + 1; r < m; ++r)
            if (std::fabs(G[r][c]) > std::fabs(G[piv][c])) piv = r;
        for (int k = 0; k < m; ++k) {
            const double g = G[c][k], h = H[c][k];
            G[c][k] = G[piv][k];
            G[piv][k] = g;
            H[c][k] = H[piv][k];
            H[piv][k] = h;
        }
        for (int r = c + 1; r < m; ++r) {
            const double f = G[r][c] / G[c][c];
            for (int k = c; k < m; ++k) G[r][k] -= f * G[c][k];
            for (int k = 0; k < m; ++k) H[r][k] -= f * H[c][k];
        }
    }
    for (int r = m - 1; r >= 0; --r)
        for (int k = 0; k < m; ++k) {
            double v = H[r][k];
            for (int c = r + 1; c < m; ++c) v -= G[r][c] * M[c * m + k];
            M[r * m + k] = v / G[r][r];
        }
    for (int k = 0; k < m * m; ++k)
        if (std::fabs(M[k]) < kShRotationNoise) M[k] = 0.0;
}

// Everything k_scene_transform takes from a (valid) transform, rounded once to binary32.
struct ShRotation {
    float q[4];                  // the normalised quaternion, w x y z
    float R[9];                  // row-major
    float M[kShMatrixFloats];    // M_1, M_2, M_3
};
inline ShRotation sh_rotation(const gs_transform& t) {
    double q[4], R[9], M[49];
    rotation_of(t, q, R);
    ShRotation o;
    for (int k = 0; k < 4; ++k) o.q[k] = static_cast<float>(q[k]);
    for (int k = 0; k < 9; ++k) o.R[k] = static_cast<float>(R[k]);
    for (int l = 1; l <= 3; ++l) {
        sh_band_matrix(l, R, M);
        for (int k = 0; k < (2 * l + 1) * (2 * l + 1); ++k) o.M[kShMatrixOffset[l] + k] = static_cast<float>(M[k]);
    }
    return o;
}

// The camera that sees the transformed scene as `in` saw the original.  A camera maps its own space to the world by
// x_w = R_c x_c + p; after x_w -> s R x_w + t that is (R R_c)(s x_c) + (s R p + t): rotation q_R (x) q_c, position s R p + t, and
// every length of camera space -- the planes included -- times s.  in.rotation is taken as it is (not normalised).
inline void transform_camera(const gs_transform& t, const gs_camera& in, gs_camera* out) {
    double q[4], R[9], o[4];
    rotation_of(t, q, R);
    const double c[4] = {in.rotation[0], in.rotation[1], in.rotation[2], in.rotation[3]};
    quat_mul(q, c, o);
    const double s = t.scale, p[3] = {in.position[0], in.position[1], in.position[2]};
    gs_camera r = in;
    for (int k = 0; k < 3; ++k) r.position[k] = static_cast<float>(s * (R[3 * k] * p[0] + R[3 * k + 1] * p[1] + R[3 * k + 2] * p[2]) + t.translation[k]);
    for (int k = 0; k < 4; ++k) r.rotation[k] = static_cast<float>(o[k]);
    r.near_plane = static_cast<float>(s * in.near_plane);
    r.far_plane = static_cast<float>(s * in.far_plane);
    *out = r;
}

}  // namespace gs_host
