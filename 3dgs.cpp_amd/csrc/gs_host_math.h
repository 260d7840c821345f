// gs_host_math.h -- host-side arithmetic of the hot path's callers: PLY record activation
// (GSScene::load, src/GSScene.cpp:36-59) and the camera uniform block
// (Renderer::updateUniforms, src/Renderer.cpp:719-754).  fp32, one rounding per operation,
// glm 1.0.0's operation order (the reference pins glm at CMakeLists.txt:31-35; glm itself is
// not vendored, so its published formulas are restated here).  Column-major 4x4: m[c*4+r].
// Also the order a large scene is read in (spatial_order, at the end; no counterpart in the reference).
// Plain C++ without a device in sight.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <utility>
#include <vector>

#include "../../include/gs3d_hip.h"

namespace gs {
namespace host {

struct Mat4 {
    float m[16];
    float& at(int c, int r) { return m[c * 4 + r]; }
    float at(int c, int r) const { return m[c * 4 + r]; }
    static Mat4 identity() {
        Mat4 o{};
        o.m[0] = o.m[5] = o.m[10] = o.m[15] = 1.0f;
        return o;
    }
};

// glm operator*(mat4, mat4): column c of the result = A.col0*B[c][0] + A.col1*B[c][1] + ...
inline Mat4 mul(const Mat4& a, const Mat4& b) {
    Mat4 o{};
    for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 4; ++r) {
            float s = a.at(0, r) * b.at(c, 0);
            s = s + a.at(1, r) * b.at(c, 1);
            s = s + a.at(2, r) * b.at(c, 2);
            s = s + a.at(3, r) * b.at(c, 3);
            o.at(c, r) = s;
        }
    return o;
}

// glm::mat4_cast(quat{w,x,y,z})
inline Mat4 from_quat(const float q[4]) {
    const float w = q[0], x = q[1], y = q[2], z = q[3];
    const float qxx = x * x, qyy = y * y, qzz = z * z;
    const float qxz = x * z, qxy = x * y, qyz = y * z;
    const float qwx = w * x, qwy = w * y, qwz = w * z;
    Mat4 o = Mat4::identity();
    o.at(0, 0) = 1.0f - 2.0f * (qyy + qzz);
    o.at(0, 1) = 2.0f * (qxy + qwz);
    o.at(0, 2) = 2.0f * (qxz - qwy);
    o.at(1, 0) = 2.0f * (qxy - qwz);
    o.at(1, 1) = 1.0f - 2.0f * (qxx + qzz);
    o.at(1, 2) = 2.0f * (qyz + qwx);
    o.at(2, 0) = 2.0f * (qxz + qwy);
    o.at(2, 1) = 2.0f * (qyz - qwx);
    o.at(2, 2) = 1.0f - 2.0f * (qxx + qyy);
    return o;
}

// glm::inverse(mat4): cofactor expansion, glm/detail/func_matrix.inl compute_inverse<4,4>.
inline Mat4 inverse(const Mat4& m) {
    auto M = [&](int c, int r) { return m.at(c, r); };
    const float c00 = M(2, 2) * M(3, 3) - M(3, 2) * M(2, 3);
    const float c02 = M(1, 2) * M(3, 3) - M(3, 2) * M(1, 3);
    const float c03 = M(1, 2) * M(2, 3) - M(2, 2) * M(1, 3);
    const float c04 = M(2, 1) * M(3, 3) - M(3, 1) * M(2, 3);
    const float c06 = M(1, 1) * M(3, 3) - M(3, 1) * M(1, 3);
    const float c07 = M(1, 1) * M(2, 3) - M(2, 1) * M(1, 3);
    const float c08 = M(2, 1) * M(3, 2) - M(3, 1) * M(2, 2);
    const float c10 = M(1, 1) * M(3, 2) - M(3, 1) * M(1, 2);
    const float c11 = M(1, 1) * M(2, 2) - M(2, 1) * M(1, 2);
    const float c12 = M(2, 0) * M(3, 3) - M(3, 0) * M(2, 3);
    const float c14 = M(1, 0) * M(3, 3) - M(3, 0) * M(1, 3);
    const float c15 = M(1, 0) * M(2, 3) - M(2, 0) * M(1, 3);
    const float c16 = M(2, 0) * M(3, 2) - M(3, 0) * M(2, 2);
    const float c18 = M(1, 0) * M(3, 2) - M(3, 0) * M(1, 2);
    const float c19 = M(1, 0) * M(2, 2) - M(2, 0) * M(1, 2);
    const float c20 = M(2, 0) * M(3, 1) - M(3, 0) * M(2, 1);
    const float c22 = M(1, 0) * M(3, 1) - M(3, 0) * M(1, 1);
    const float c23 = M(1, 0) * M(2, 1) - M(2, 0) * M(1, 1);
    const float fac[6][4] = {{c00, c00, c02, c03}, {c04, c04, c06, c07}, {c08, c08, c10, c11},
                             {c12, c12, c14, c15}, {c16, c16, c18, c19}, {c20, c20, c22, c23}};
    const float vec[4][4] = {{M(1, 0), M(0, 0), M(0, 0), M(0, 0)},
                             {M(1, 1), M(0, 1), M(0, 1), M(0, 1)},
                             {M(1, 2), M(0, 2), M(0, 2), M(0, 2)},
                             {M(1, 3), M(0, 3), M(0, 3), M(0, 3)}};
    Mat4 inv{};
    for (int i = 0; i < 4; ++i) {
        const float sign_a = (i & 1) ? -1.0f : 1.0f, sign_b = -sign_a;
        inv.at(0, i) = ((vec[1][i] * fac[0][i] - vec[2][i] * fac[1][i]) + vec[3][i] * fac[2][i]) * sign_a;
        inv.at(1, i) = ((vec[0][i] * fac[0][i] - vec[2][i] * fac[3][i]) + vec[3][i] * fac[4][i]) * sign_b;
        inv.at(2, i) = ((vec[0][i] * fac[1][i] - vec[1][i] * fac[3][i]) + vec[3][i] * fac[5][i]) * sign_a;
        inv.at(3, i) = ((vec[0][i] * fac[2][i] - vec[1][i] * fac[4][i]) + vec[2][i] * fac[5][i]) * sign_b;
    }
    const float d0 = M(0, 0) * inv.at(0, 0), d1 = M(0, 1) * inv.at(1, 0);
    const float d2 = M(0, 2) * inv.at(2, 0), d3 = M(0, 3) * inv.at(3, 0);
    const float one_over_det = 1.0f / ((d0 + d1) + (d2 + d3));
    for (float& v : inv.m) v = v * one_over_det;
    return inv;
}

// Renderer::updateUniforms, src/Renderer.cpp:719-754.
inline void camera_uniforms(const gs_camera& cam, uint32_t width, uint32_t height, gs_uniforms* out) {
    std::memset(out, 0, sizeof *out);
    out->width = width;
    out->height = height;
    out->camera_position[0] = cam.position[0];
    out->camera_position[1] = cam.position[1];
    out->camera_position[2] = cam.position[2];
    out->camera_position[3] = 1.0f;

    const Mat4 rotation = from_quat(cam.rotation);
    Mat4 translation = Mat4::identity();  // glm::translate(mat4(1), position)
    translation.at(3, 0) = cam.position[0];
    translation.at(3, 1) = cam.position[1];
    translation.at(3, 2) = cam.position[2];
    const Mat4 view = inverse(mul(translation, rotation));

    // :730 std::tan(glm::radians(fov) / 2.0) is evaluated in double and narrowed
    const float radians = cam.fov * 0.01745329251994329576923690768489f;
    const float tan_fovx = static_cast<float>(std::tan(static_cast<double>(radians) / 2.0));
    const float tan_fovy = tan_fovx * static_cast<float>(height) / static_cast<float>(width);

    // glm::perspectiveRH_NO(atan(tan_fovy) * 2, w / h, near, far)
    const float fovy = std::atan(tan_fovy) * 2.0f;
    const float aspect = static_cast<float>(width) / static_cast<float>(height);
    const float tan_half = std::tan(fovy / 2.0f);
    Mat4 persp{};
    persp.at(0, 0) = 1.0f / (aspect * tan_half);
    persp.at(1, 1) = 1.0f / tan_half;
    persp.at(2, 2) = -(cam.far_plane + cam.near_plane) / (cam.far_plane - cam.near_plane);
    persp.at(2, 3) = -1.0f;
    persp.at(3, 2) = -(2.0f * cam.far_plane * cam.near_plane) / (cam.far_plane - cam.near_plane);
    Mat4 proj = mul(persp, view);
    Mat4 v = view;
    for (int c = 0; c < 4; ++c) {  // :738-750 shader space is x right, y down, z forward
        v.at(c, 1) *= -1.0f;
        v.at(c, 2) *= -1.0f;
        proj.at(c, 1) *= -1.0f;
    }
    std::memcpy(out->proj_mat, proj.m, sizeof proj.m);
    std::memcpy(out->view_mat, v.m, sizeof v.m);
    out->tan_fovx = tan_fovx;
    out->tan_fovy = tan_fovy;
}

// gs_camera_uniforms_backward (gs3d_hip.h): the gradient of the exact real function behind camera_uniforms with respect to the
// camera's position and raw quaternion, binary64, at the binary32 camera values.  No reference counterpart.  [row][column] here.
//     M = [R(q) | position; 0 0 0 1],  R = mat4_cast(q), q not normalised;   view = M^-1;   proj = persp view;
//     view rows 1, 2 and proj row 1 negated;   camera_position = position.
// g arrays are laid out as the uniforms' matrices (element 4 c + r); every row of them is taken.
inline void camera_uniforms_backward(const gs_camera& cam, uint32_t width, uint32_t height, const double* g_view_mat, const double* g_proj_mat,
                                     const double* g_camera_position, double* d_position, double* d_rotation) {
    const double w = cam.rotation[0], x = cam.rotation[1], y = cam.rotation[2], z = cam.rotation[3];
    const double R[3][3] = {{1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)},
                            {2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)},
                            {2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)}};
    // M^-1 = [R^-1 | -R^-1 position]: R is orthogonal only for a unit quaternion, so the adjugate over the determinant
    double Ri[3][3];
    const double det = R[0][0] * (R[1][1] * R[2][2] - R[1][2] * R[2][1]) - R[0][1] * (R[1][0] * R[2][2] - R[1][2] * R[2][0]) +
                       R[0][2] * (R[1][0] * R[2][1] - R[1][1] * R[2][0]);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            const int r1 = (c + 1) % 3, r2 = (c + 2) % 3, c1 = (r + 1) % 3, c2 = (r + 2) % 3;  // cofactor of R[c][r]
            Ri[r][c] = (R[r1][c1] * R[r2][c2] - R[r1][c2] * R[r2][c1]) / det;
        }
    double Mi[4][4] = {};
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) Mi[r][c] = Ri[r][c];
        Mi[r][3] = -((Ri[r][0] * (double)cam.position[0] + Ri[r][1] * (double)cam.position[1]) + Ri[r][2] * (double)cam.position[2]);
    }
    Mi[3][3] = 1.0;
    // persp, as the forward's real function: tan(atan(tan_fovy) * 2 / 2) = tan_fovy, aspect * tan_fovy = tan_fovx
    const double tan_fovx = std::tan((double)cam.fov * 0.01745329251994329576923690768489 / 2.0);
    const double tan_fovy = tan_fovx * (double)height / (double)width;
    const double nearp = cam.near_plane, farp = cam.far_plane;
    double persp[4][4] = {};
    persp[0][0] = 1.0 / tan_fovx;
    persp[1][1] = 1.0 / tan_fovy;
    persp[2][2] = -(farp + nearp) / (farp - nearp);
    persp[3][2] = -1.0;
    persp[2][3] = -(2.0 * farp * nearp) / (farp - nearp);
    // the flips undone, then g_view += persp^T g_proj
    double gv[4][4], gp[4][4];
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) {
            gv[r][c] = (r == 1 || r == 2) ? -g_view_mat[c * 4 + r] : g_view_mat[c * 4 + r];
            gp[r][c] = (r == 1) ? -g_proj_mat[c * 4 + r] : g_proj_mat[c * 4 + r];
        }
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c)
            for (int e = 0; e < 4; ++e) gv[r][c] += persp[e][r] * gp[e][c];
    // g_M = -M^-T g_view M^-T
    double tmp[4][4] = {}, gM[4][4] = {};
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c)
            for (int e = 0; e < 4; ++e) tmp[r][c] += Mi[e][r] * gv[e][c];
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) {
            for (int e = 0; e < 4; ++e) gM[r][c] += tmp[r][e] * Mi[c][e];
            gM[r][c] = -gM[r][c];
        }
    for (int c = 0; c < 3; ++c) d_position[c] = gM[c][3] + g_camera_position[c];
    const double(*G)[4] = gM;  // the 3 x 3 block is dL/dR
    d_rotation[0] = 2.0 * (z * G[1][0] - y * G[2][0] - z * G[0][1] + x * G[2][1] + y * G[0][2] - x * G[1][2]);
    d_rotation[1] = 2.0 * (y * G[1][0] + z * G[2][0] + y * G[0][1] - 2.0 * x * G[1][1] + w * G[2][1] + z * G[0][2] - w * G[1][2] - 2.0 * x * G[2][2]);
    d_rotation[2] = 2.0 * (-2.0 * y * G[0][0] + x * G[1][0] - w * G[2][0] + x * G[0][1] + z * G[2][1] + w * G[0][2] + z * G[1][2] - 2.0 * y * G[2][2]);
    d_rotation[3] = 2.0 * (-2.0 * z * G[0][0] + w * G[1][0] + x * G[2][0] - w * G[0][1] - 2.0 * z * G[1][1] + y * G[2][1] + x * G[0][2] + y * G[1][2]);
}

constexpr int kRecordFloats = 62;  // VertexStorage, GSScene.cpp:17-24
constexpr int kVertexFloats = 60;  // GSScene::Vertex, GSScene.h:41-46

// One PLY record -> one activated vertex (position4, scale_opacity4, rotation4, shs48).
inline void activate_record(const float* r, float* v) {
    const float* shs = r + 6;
    const float opacity = r[54];
    const float* scale = r + 55;
    const float* rot = r + 58;
    v[0] = r[0];
    v[1] = r[1];
    v[2] = r[2];
    v[3] = 1.0f;
    v[4] = std::exp(scale[0]);  // glm::exp(vec3) is std::exp per component
    v[5] = std::exp(scale[1]);
    v[6] = std::exp(scale[2]);
    v[7] = 1.0f / (1.0f + std::exp(-opacity));
    // glm::normalize(vec4): v * inversesqrt(dot(v, v)), dot<4> = (x*x + y*y) + (z*z + w*w)
    const float dot = (rot[0] * rot[0] + rot[1] * rot[1]) + (rot[2] * rot[2] + rot[3] * rot[3]);
    const float inv = 1.0f / std::sqrt(dot);
    for (int k = 0; k < 4; ++k) v[8 + k] = rot[k] * inv;
    float* out = v + 12;
    out[0] = shs[0];
    out[1] = shs[1];
    out[2] = shs[2];
    constexpr int SH_N = 16;
    for (int j = 1; j < SH_N; ++j) {  // planar RRR..GGG..BBB -> interleaved RGB per coefficient
        out[j * 3 + 0] = shs[(j - 1) + 3];
        out[j * 3 + 1] = shs[(j - 1) + SH_N + 2];
        out[j * 3 + 2] = shs[(j - 1) + SH_N * 2 + 1];
    }
}

// ---- the inverse of activate_record (gs_deactivate_vertices; on the device: k_scene_export, gs_scene.hip, bit for bit; in
// numpy: tests/export_reference.py).  A stored scale s or opacity o is exported as the binary32 x whose activation is closest
// to it -- on every image of the activation that is the stored bits themselves.  binary64 + - x / only, every operation
// rounded on its own (-ffp-contract=off), no fma, no libm log:
//   log64(v), v = m 2^e, m in [1/2, 1):  m < sqrt(1/2) -> m = 2 m, e = e - 1;  t = (m - 1) / (m + 1);  w = t t;
//       p = 1/17;  p = p w + 1/15;  .. + 1/13, 1/11, 1/9, 1/7, 1/5, 1/3;  p = p w + 1      (each 1/k the binary64 quotient)
//       log64 = (double)e * ln2 + (2 t) p,  ln2 = 0x1.62e42fefa39efp-1
//   first guess x0, rounded once to binary32: log64(s);  log64(o / (1 - o)) with o, 1 - o and the quotient in binary64
//   polish: x0 and its binary32 neighbours at distance 1 .. 4, in the order 0, -1, +1, -2, +2, -3, +3, -4, +4 (stepped across
//       zero as nextafter steps; a non-finite candidate is skipped), each activated as activate_record activates; the first
//       with the strictly smallest |(double)act - (double)stored| is the export, a NaN activation never is.  The search stops
//       at a candidate that reproduces the stored value: distance 0 cannot be beaten, the result is the same.
//   edges, without polish: s == 0 -> -inf, s == +inf -> +inf, s < 0 or NaN -> NaN;  o == 0 -> -inf, o == 1 -> +inf, o outside
//       [0, 1] or NaN -> NaN.
inline double export_log64(double v) {  // v: positive, finite, normal (every binary32 > 0 is, and so is o / (1 - o))
    uint64_t b;
    std::memcpy(&b, &v, sizeof b);
    int e = static_cast<int>((b >> 52) & 0x7FFu) - 1022;
    b = (b & 0x000FFFFFFFFFFFFFull) | 0x3FE0000000000000ull;
    double m;
    std::memcpy(&m, &b, sizeof m);
    if (m < 0x1.6a09e667f3bcdp-1) {
        m = 2.0 * m;
        e = e - 1;
    }
    const double t = (m - 1.0) / (m + 1.0), w = t * t;
    double p = 1.0 / 17.0;
    p = p * w + 1.0 / 15.0;
    p = p * w + 1.0 / 13.0;
    p = p * w + 1.0 / 11.0;
    p = p * w + 1.0 / 9.0;
    p = p * w + 1.0 / 7.0;
    p = p * w + 1.0 / 5.0;
    p = p * w + 1.0 / 3.0;
    p = p * w + 1.0;
    return static_cast<double>(e) * 0x1.62e42fefa39efp-1 + (2.0 * t) * p;
}

// the binary32 value d steps from x in the order of the reals (+-0 is one value; a step from it lands on a subnormal)
inline float export_neighbour(float x, int d) {
    uint32_t b;
    std::memcpy(&b, &x, sizeof b);
    int64_t key = (b & 0x80000000u) ? -static_cast<int64_t>(b & 0x7FFFFFFFu) : static_cast<int64_t>(b);
    key += d;
    b = key < 0 ? (0x80000000u | static_cast<uint32_t>(-key)) : static_cast<uint32_t>(key);
    std::memcpy(&x, &b, sizeof x);
    return x;
}

template <bool OPACITY>
inline float export_polish(float x0, float stored) {
    float best = x0;
    double best_err = std::numeric_limits<double>::infinity();
    for (int k = 0; k < 9; ++k) {
        const float c = export_neighbour(x0, (k & 1) ? -((k + 1) >> 1) : (k >> 1));
        if (!std::isfinite(c)) continue;
        const float act = OPACITY ? 1.0f / (1.0f + std::exp(-c)) : std::exp(c);
        const double diff = static_cast<double>(act) - static_cast<double>(stored);
        const double err = diff < 0.0 ? -diff : diff;
        if (err < best_err) best = c, best_err = err;  // (false for a NaN)
        if (err == 0.0) break;
    }
    return best;
}

inline float export_log_scale(float s) {
    if (!(s > 0.0f)) return s == 0.0f ? -std::numeric_limits<float>::infinity() : std::numeric_limits<float>::quiet_NaN();
    if (s == std::numeric_limits<float>::infinity()) return s;
    return export_polish<false>(static_cast<float>(export_log64(static_cast<double>(s))), s);
}

inline float export_opacity_logit(float o) {
    if (o == 0.0f) return -std::numeric_limits<float>::infinity();
    if (o == 1.0f) return std::numeric_limits<float>::infinity();
    if (!(o > 0.0f && o < 1.0f)) return std::numeric_limits<float>::quiet_NaN();
    const double od = static_cast<double>(o), rest = 1.0 - od;
    return export_polish<true>(static_cast<float>(export_log64(od / rest)), o);
}

// One activated vertex -> one PLY record.  Positions, the rotation AS STORED (normalised: a reload renormalises it, which may
// move each component by a few 2^-24 relative; gs3d_hip.h) and the 48 SH coefficients are copies of bits, the normals are 0.
inline void deactivate_vertex(const float* v, float* r) {
    r[0] = v[0];
    r[1] = v[1];
    r[2] = v[2];
    r[3] = r[4] = r[5] = 0.0f;
    const float* in = v + 12;
    float* shs = r + 6;
    shs[0] = in[0];
    shs[1] = in[1];
    shs[2] = in[2];
    constexpr int SH_N = 16;
    for (int j = 1; j < SH_N; ++j) {  // interleaved RGB per coefficient -> planar RRR..GGG..BBB
        shs[(j - 1) + 3] = in[j * 3 + 0];
        shs[(j - 1) + SH_N + 2] = in[j * 3 + 1];
        shs[(j - 1) + SH_N * 2 + 1] = in[j * 3 + 2];
    }
    r[54] = export_opacity_logit(v[7]);
    for (int k = 0; k < 3; ++k) r[55 + k] = export_log_scale(v[4 + k]);
    for (int k = 0; k < 4; ++k) r[58 + k] = v[8 + k];
}

// ---- the order the per-frame kernels read a large scene in (gs_scene::make_spatial_copy): ascending Morton code of the
// position, ties by id.
//   * per axis the finite coordinates' bounding box [lo, hi] is cut into 2^21 cells: cell = min(2^21 - 1, floor(t 2^21)) with
//     t = (v - lo) / (hi - lo) evaluated in binary64 from the binary32 values;
//   * a degenerate axis (no finite coordinate, or all of them equal) takes hi = lo + 1 in binary32;
//   * a non-finite coordinate (NaN, +-inf) maps to cell 0;
//   * the code interleaves the three cells bit by bit, x lowest: bit 3 b + k of the code is bit b of axis k's cell.
// tests/test_limit_scenes.py drives it on the CPU (tests/native/spatial_order_sim.cpp) against
// tests/limit_scenes.py::morton_order, which restates it in numpy: a change of the rules here changes them there.
inline uint64_t morton_spread21(uint64_t v) {  // 21 bits -> every third bit
    v &= 0x1FFFFFull;
    v = (v | v << 32) & 0x1F00000000FFFFull;
    v = (v | v << 16) & 0x1F0000FF0000FFull;
    v = (v | v << 8) & 0x100F00F00F00F00Full;
    v = (v | v << 4) & 0x10C30C30C30C30C3ull;
    v = (v | v << 2) & 0x1249249249249249ull;
    return v;
}

// pos[k]: the n coordinates of axis k (x, y, z).  Returns the scene ids in the order they are read: order[j] = id of read slot j.
inline std::vector<uint32_t> spatial_order(const float* const pos[3], uint64_t n) {
    float lo[3], hi[3];
    for (int k = 0; k < 3; ++k) {
        lo[k] = std::numeric_limits<float>::infinity();
        hi[k] = -lo[k];
        for (uint64_t i = 0; i < n; ++i) {
            const float v = pos[k][i];
            if (std::isfinite(v)) lo[k] = std::min(lo[k], v), hi[k] = std::max(hi[k], v);
        }
        if (!(hi[k] > lo[k])) hi[k] = lo[k] + 1.0f;
    }
    std::vector<std::pair<uint64_t, uint32_t>> keyed(n);
    for (uint64_t i = 0; i < n; ++i) {
        uint64_t code = 0;
        for (int k = 0; k < 3; ++k) {
            const float v = pos[k][i];
            const double t = std::isfinite(v) ? (static_cast<double>(v) - lo[k]) / (static_cast<double>(hi[k]) - lo[k]) : 0.0;
            code |= morton_spread21(static_cast<uint64_t>(std::min(2097151.0, std::max(0.0, t * 2097152.0)))) << k;
        }
        keyed[i] = {code, static_cast<uint32_t>(i)};
    }
    std::sort(keyed.begin(), keyed.end());
    std::vector<uint32_t> order(n);
    for (uint64_t i = 0; i < n; ++i) order[i] = keyed[i].second;
    return order;
}

}  // namespace host
}  // namespace gs
