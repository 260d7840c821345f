// gs_scene.hip -- load-time kernels: cov3D precompute, SH quantisation, the per-Gaussian alpha cut of render.comp:78.
//
// Part of libgs3d_hip.so (gfx950 only).  Built with -ffp-contract=off: the floating-point contract of this path is "IEEE
// binary32, one rounding per operation, in the order the reference shader writes it" (DESIGN.md section 3); fused
// multiply-adds appear only where written explicitly.
// Reference restated (paths relative to /root/reference/src/shaders): precomp_cov3d.comp:25-47, common.glsl:51-75
#include "gs_device.h"

namespace gs {

// ---------------------------------------------------------------------------------------
// cov3D precompute (load time).  precomp_cov3d.comp:25-47.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ M3 rotation_from_quaternion(float qw, float qx, float qy, float qz) {
    float qx2 = qx * qx, qy2 = qy * qy, qz2 = qz * qz;
    M3 m;
    m.c[0][0] = 1 - 2 * qy2 - 2 * qz2;
    m.c[0][1] = 2 * qx * qy - 2 * qz * qw;
    m.c[0][2] = 2 * qx * qz + 2 * qy * qw;
    m.c[1][0] = 2 * qx * qy + 2 * qz * qw;
    m.c[1][1] = 1 - 2 * qx2 - 2 * qz2;
    m.c[1][2] = 2 * qy * qz - 2 * qx * qw;
    m.c[2][0] = 2 * qx * qz - 2 * qy * qw;
    m.c[2][1] = 2 * qy * qz + 2 * qx * qw;
    m.c[2][2] = 1 - 2 * qx2 - 2 * qy2;
    return m;
}

__global__ __launch_bounds__(BLOCK) void k_cov3d(const float* __restrict__ blob, float* __restrict__ cov3d,
                                                 uint32_t n, uint32_t stride, uint32_t first, uint32_t count) {
    uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= count) return;
    i += first;  // < n: the caller's range lies inside the scene
    const size_t N = stride, NC = n;
    const float scale_factor = 1.0f;  // GSScene.cpp:176
    M3 S = {};
    S.c[0][0] = blob[(P_SCALE + 0) * N + i] * scale_factor;
    S.c[1][1] = blob[(P_SCALE + 1) * N + i] * scale_factor;
    S.c[2][2] = blob[(P_SCALE + 2) * N + i] * scale_factor;
    M3 R = rotation_from_quaternion(blob[(P_ROT + 0) * N + i], blob[(P_ROT + 1) * N + i],
                                    blob[(P_ROT + 2) * N + i], blob[(P_ROT + 3) * N + i]);
    M3 M = m3_mul(S, R);
    M3 C = m3_mul(m3_transpose(M), M);
    cov3d[0 * NC + i] = C.c[0][0];
    cov3d[1 * NC + i] = C.c[0][1];
    cov3d[2 * NC + i] = C.c[0][2];
    cov3d[3 * NC + i] = C.c[1][1];
    cov3d[4 * NC + i] = C.c[1][2];
    cov3d[5 * NC + i] = C.c[2][2];
}

// Opt-in SH quantisation: the fp32 SH block -> binary16, round to nearest even.
__global__ __launch_bounds__(BLOCK) void k_sh_to_half(const float* __restrict__ sh, uint16_t* __restrict__ out, uint64_t count) {
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i < count) out[i] = __half_as_ushort(__float2half_rn(sh[i]));
}
void launch_sh_to_half(const float* blob, uint16_t* sh16, uint32_t stride, uint32_t first, uint32_t count, hipStream_t s) {
    if (count == 0) return;
    const uint64_t values = 48ull * count, at = 48ull * first;
    hipLaunchKernelGGL(k_sh_to_half, dim3((uint32_t)((values + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s,
                       blob + (size_t)P_SH * stride + at, sh16 + at, values);
}

// The alpha cut of every Gaussian (gs_device.h: alpha_cut), a function of its opacity alone: one plane of n floats beside cov3D.
// *beyond_unit (nullable, zeroed by the caller) is set when an opacity exceeds 1: the guarded blend's bound assumes the sigmoid's range.
__global__ __launch_bounds__(BLOCK) void k_alpha_cut(const float* __restrict__ opacity, float* __restrict__ cut, uint32_t n,
                                                     uint32_t* __restrict__ beyond_unit) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const float o = opacity[i];
    cut[i] = alpha_cut(o, reinterpret_cast<const uint2*>(kExpfTab));
    if (beyond_unit && o > 1.0f) *beyond_unit = 1u;  // (racing stores of the same value)
}
void launch_alpha_cut(const float* blob, float* cut, uint32_t n, uint32_t stride, uint32_t* beyond_unit, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_alpha_cut, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, blob + (size_t)P_OPACITY * stride, cut, n, beyond_unit);
}

// ---- test hook: the antialiased mode's per-frame cut (alpha_cut_seeded) against the load-time bisection, pattern by pattern
__global__ __launch_bounds__(BLOCK) void k_alpha_cut_scan(uint32_t first_bits, uint64_t count, unsigned long long* __restrict__ mismatches,
                                                          uint32_t* __restrict__ first_mismatch) {
    const uint2* tab = reinterpret_cast<const uint2*>(kExpfTab);
    unsigned long long bad = 0;
    uint32_t first = 0xFFFFFFFFu;
    for (uint64_t at = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; at < count; at += (uint64_t)gridDim.x * BLOCK) {
        const uint32_t ob = first_bits + (uint32_t)at;
        const float o = __uint_as_float(ob);
        if (__float_as_uint(alpha_cut_seeded(o, tab)) != __float_as_uint(alpha_cut(o, tab))) {
            ++bad;
            first = min(first, ob);
        }
    }
    if (bad) {
        atomicAdd(mismatches, bad);
        atomicMin(first_mismatch, first);
    }
}

extern "C" int gs_debug_alpha_cut_scan(int device, uint32_t first_bits, uint64_t count, uint64_t* mismatches, uint32_t* first_mismatch) {
    if (!mismatches || !first_mismatch || count == 0 || count > (1ull << 32)) return GS_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess) return GS_ERR_DEVICE;
    unsigned long long* d = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&d), 2 * sizeof(unsigned long long)) != hipSuccess) return GS_ERR_NOMEM;
    const unsigned long long init[2] = {0ull, 0xFFFFFFFFull};  // [0] count, [1] low word: the first mismatching pattern
    int rc = GS_OK;
    if (hipMemcpy(d, init, sizeof init, hipMemcpyHostToDevice) != hipSuccess) rc = GS_ERR_DEVICE;
    if (rc == GS_OK) {
        const uint64_t blocks = std::min<uint64_t>(65536, (count + BLOCK - 1) / BLOCK);
        hipLaunchKernelGGL(k_alpha_cut_scan, dim3((uint32_t)blocks), dim3(BLOCK), 0, nullptr, first_bits, count, d,
                           reinterpret_cast<uint32_t*>(d + 1));
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) rc = GS_ERR_DEVICE;
    }
    unsigned long long out[2] = {0, 0};
    if (rc == GS_OK && hipMemcpy(out, d, sizeof out, hipMemcpyDeviceToHost) != hipSuccess) rc = GS_ERR_DEVICE;
    (void)hipFree(d);
    if (rc == GS_OK) {
        *mismatches = out[0];
        *first_mismatch = (uint32_t)(out[1] & 0xFFFFFFFFull);
    }
    return rc;
}

// The scene's second copy in spatial order (gs_scene::make_spatial_copy): one thread per (Gaussian, 16-byte chunk of its 59 floats).
__global__ __launch_bounds__(BLOCK) void k_permute_blob(const float* __restrict__ src, const uint32_t* __restrict__ perm,
                                                        float* __restrict__ dst, uint32_t n, uint32_t stride) {
    const uint64_t t = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t j = (uint32_t)(t / 15u), c = (uint32_t)(t % 15u);  // chunks 0..11: the SH block; 12..14: the 11 planes, four at a time
    if (j >= n) return;
    const uint32_t g = perm[j];
    if (c < 12u) {
        reinterpret_cast<float4*>(dst + (size_t)P_SH * stride)[(size_t)j * 12 + c] =
            reinterpret_cast<const float4*>(src + (size_t)P_SH * stride)[(size_t)g * 12 + c];
    } else {
        for (uint32_t p = (c - 12u) * 4u; p < min((c - 11u) * 4u, (uint32_t)P_SH); ++p) dst[(size_t)p * stride + j] = src[(size_t)p * stride + g];
    }
}
void launch_permute_blob(const float* src, const uint32_t* perm, float* dst, uint32_t n, uint32_t stride, hipStream_t s) {
    if (n == 0) return;
    const uint64_t threads = 15ull * n;
    hipLaunchKernelGGL(k_permute_blob, dim3((uint32_t)((threads + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, src, perm, dst, n, stride);
}

// Checksum of a scene replica (gs_dist_verify): the sum of the blob's bit patterns.
__global__ __launch_bounds__(BLOCK) void k_blob_checksum(const uint32_t* __restrict__ words, uint64_t count, unsigned long long* __restrict__ out) {
    unsigned long long sum = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < count; i += (uint64_t)gridDim.x * BLOCK) sum += words[i];
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, WAVE);
    if ((threadIdx.x & (WAVE - 1)) == 0 && sum != 0) atomicAdd(out, sum);
}
void launch_blob_checksum(const float* blob, uint64_t floats, uint64_t* out, hipStream_t s) {
    (void)hipMemsetAsync(out, 0, sizeof(uint64_t), s);
    if (floats == 0) return;
    hipLaunchKernelGGL(k_blob_checksum, dim3(2048), dim3(BLOCK), 0, s, reinterpret_cast<const uint32_t*>(blob), floats,
                       reinterpret_cast<unsigned long long*>(out));
}

void launch_cov3d(const float* blob, float* cov3d, uint32_t n, uint32_t stride, uint32_t first, uint32_t count, hipStream_t s) {
    if (count == 0) return;
    hipLaunchKernelGGL(k_cov3d, dim3((count + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, blob, cov3d, n, stride, first, count);
}

// ---------------------------------------------------------------------------------------
// A trainer's device arrays -> the blob (gs_scene_from_device_arrays / gs_scene_update_from_device_arrays): GSScene::load's
// per-record conversion (GSScene.cpp:42-55, gs_host_math.h: activate_record) on the device, bit for bit.
// ---------------------------------------------------------------------------------------
// (exp is gs_expf_libm_domain, gs_device.h: libm's expf on the whole domain.)
// One workgroup takes BLOCK consecutive Gaussians of the range: Gaussian i of the arrays is Gaussian first + i of the scene.
//   * the [n][3] / [n][4] arrays are read as the runs of floats they are (lane-contiguous: the sources are only 4-byte
//     aligned) into LDS and picked up per Gaussian -- a stride of 3 dwords is conflict-free on 32 banks, the quaternion is one
//     16-byte ds_read_b128 per lane (contiguous, conflict-free; four ds_read_b32 at stride 4 would be 4-way);
//   * the planes are written lane-contiguous;
//   * the SH rows (192 bytes, 16-byte aligned in the blob) are written as whole 16-byte stores from scalar loads: float f of
//     row g is dc[g][f] for f < 3, rest[g][f - 3] for f < 3 + 3 k, 0 beyond.  A member that is absent (DC / REST false: an
//     update that keeps it) is read back from the row itself; without REST only the row's first 16 bytes are touched.
//     REST with sh_rest_coeffs == 0 writes zeros and never reads sh_rest (degree 0: the pointer may be null).
// A null plane member (uniform branch) leaves its planes alone.
template <bool DC, bool REST>
__device__ __forceinline__ void ingest_sh_rows(const gs_device_arrays& a, float* __restrict__ sh_rows, uint32_t g0, uint32_t count) {
    const uint32_t in_block = min((uint32_t)BLOCK, count - g0);
    const uint32_t k3 = 3u * a.sh_rest_coeffs;
    const uint32_t chunks = REST ? 12u : 1u;  // 16-byte chunks of a row that change
    for (uint32_t q = threadIdx.x; q < in_block * chunks; q += BLOCK) {
        const uint32_t gl = q / chunks, c = q - gl * chunks;
        const size_t g = (size_t)g0 + gl;
        float* row = sh_rows + g * 48u;
        float v[4];
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) {
            const uint32_t f = 4u * c + i;
            if (f < 3u) v[i] = DC ? a.sh_dc[g * 3u + f] : row[f];
            else if (REST) v[i] = f - 3u < k3 ? a.sh_rest[g * k3 + (f - 3u)] : 0.0f;
            else v[i] = row[f];
        }
        reinterpret_cast<float4*>(row)[c] = make_float4(v[0], v[1], v[2], v[3]);
    }
}

template <bool DC, bool REST>
__global__ __launch_bounds__(BLOCK) void k_ingest_arrays(gs_device_arrays a, float* __restrict__ blob, uint32_t stride, uint32_t first,
                                                         uint32_t count) {
    __shared__ float s_pos[3 * BLOCK], s_scale[3 * BLOCK];
    __shared__ __attribute__((aligned(16))) float s_rot[4 * BLOCK];
    const uint32_t g0 = blockIdx.x * BLOCK, t = threadIdx.x, i = g0 + t;  // g0 < count: the grid covers the range
    const size_t N = stride;
    const uint32_t left = count - g0;  // Gaussians from g0 on; the block holds min(BLOCK, left) of them
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t j = k * BLOCK + t;
        if (k < 3 && a.means && j < 3ull * left) s_pos[j] = a.means[(size_t)g0 * 3 + j];
        if (k < 3 && a.log_scales && j < 3ull * left) s_scale[j] = a.log_scales[(size_t)g0 * 3 + j];
        if (a.quats && j < 4ull * left) s_rot[j] = a.quats[(size_t)g0 * 4 + j];
    }
    __syncthreads();
    if (i < count) {
        const uint2* tab = reinterpret_cast<const uint2*>(kExpfTab);
        float* out = blob + first + i;
        if (a.means) {
            for (int k = 0; k < 3; ++k) out[(P_POS + k) * N] = s_pos[3 * t + k];
        }
        if (a.log_scales) {
            for (int k = 0; k < 3; ++k) out[(P_SCALE + k) * N] = gs_expf_libm_domain(s_scale[3 * t + k], tab);
        }
        if (a.quats) {
            const float4 q = reinterpret_cast<const float4*>(s_rot)[t];
            // glm::normalize(vec4): v * inversesqrt(dot(v, v)), dot<4> = (x*x + y*y) + (z*z + w*w)  (activate_record)
            const float dot = (q.x * q.x + q.y * q.y) + (q.z * q.z + q.w * q.w);
            const float inv = 1.0f / sqrtf(dot);  // both correctly rounded (hipcc's default; no fast-math in this build)
            out[(P_ROT + 0) * N] = q.x * inv;
            out[(P_ROT + 1) * N] = q.y * inv;
            out[(P_ROT + 2) * N] = q.z * inv;
            out[(P_ROT + 3) * N] = q.w * inv;
        }
        if (a.opacity_logits) out[P_OPACITY * N] = 1.0f / (1.0f + gs_expf_libm_domain(-a.opacity_logits[i], tab));
    }
    if (DC || REST) ingest_sh_rows<DC, REST>(a, blob + (size_t)P_SH * N + (size_t)first * 48u, g0, count);
}

void launch_ingest_arrays(const gs_device_arrays& a, float* blob, uint32_t stride, uint32_t first, uint32_t count, bool replace_rest,
                          hipStream_t s) {
    if (count == 0) return;
    const dim3 grid((count + BLOCK - 1) / BLOCK), block(BLOCK);
    if (a.sh_dc && replace_rest) hipLaunchKernelGGL((k_ingest_arrays<true, true>), grid, block, 0, s, a, blob, stride, first, count);
    else if (a.sh_dc) hipLaunchKernelGGL((k_ingest_arrays<true, false>), grid, block, 0, s, a, blob, stride, first, count);
    else if (replace_rest) hipLaunchKernelGGL((k_ingest_arrays<false, true>), grid, block, 0, s, a, blob, stride, first, count);
    else hipLaunchKernelGGL((k_ingest_arrays<false, false>), grid, block, 0, s, a, blob, stride, first, count);
}

// ---------------------------------------------------------------------------------------
// gs_scene_transform: Gaussians [first, first + count) moved by x -> s R x + t, in place (gs3d_hip.h).  No reference counterpart.
// ---------------------------------------------------------------------------------------
// A memory-bound pass: 55 floats in and 55 out per Gaussian (440 B) against ~330 multiply-adds.  One workgroup takes BLOCK
// consecutive Gaussians of the range; Gaussian i of it is Gaussian first + i of the scene.
//   * the ten planes (position, scale, rotation) are read and written lane-contiguous; the opacity plane is not touched;
//   * the SH rows (192 bytes each; the range's first one is 16-byte aligned: 192 first) go through LDS: the workgroup's rows
//     are ONE run of bytes, copied in and out as whole 16-byte accesses, lane-contiguous, while each lane picks up and puts back
//     its own row as twelve 16-byte LDS accesses.  The LDS row stride is 52 dwords, not 48: at 48 the lanes of a 16-byte
//     access's group start on only four different bank slots (48 l mod 64 is a multiple of 16), at 52 = 4 x 13 the 16
//     lanes of a read group (banks mod 64) and the 8 of a write group (banks mod 32) each start on a slot of their own.
//     The DC term (the row's first three floats) travels through unchanged.  The lane's accesses are volatile so that they STAY
//     16-byte instructions (the binary holds 13 ds_read_b128 and 13 ds_write_b128: twelve per row, one per copy loop, and no other
//     LDS instruction).  What conflicts remain are the copy loops' (measured: SQ_LDS_BANK_CONFLICT 80 of SQ_LDS_IDX_ACTIVE's 368
//     cycles per wave): of consecutive 16-byte pieces, the one that starts a new row lies 4 dwords further on and meets a
//     neighbour's banks.
//   * R, s, t, q and the 83 entries of M are kernel arguments, wave-uniform.
// ARITHMETIC (binary32, -ffp-contract=off: every product and sum below rounded on its own, in this order; the tolerances of
// tests/test_gpu_scene_transform.py are derived from it):
//     position'_k = s * ((R_k0 x + R_k1 y) + R_k2 z) + t_k
//     scale'_k    = s * scale_k
//     rotation'   = v * (1 / sqrt((v.w v.w + v.x v.x) + (v.y v.y + v.z v.z))),  v = q (x) rotation with each component's four
//                   products added left to right in the order w x y z of q's components (division and square root IEEE)
//     c'_i        = (..((M_i0 c_0 + M_i1 c_1) + M_i2 c_2) + ..) + M_i,2l c_2l     per band l and colour channel
constexpr uint32_t kShRowLds = 52;  // dwords between two Gaussians' SH rows in LDS
typedef float ShChunk __attribute__((ext_vector_type(4)));  // 16 bytes of a row, as one LDS access
typedef volatile __attribute__((address_space(3))) ShChunk LdsShChunk;

template <int M_DIM>
__device__ __forceinline__ void sh_band_rotate(const float* __restrict__ M, const float* in, float* out, int j0) {
    // coefficients j0 .. j0 + M_DIM - 1 of the three channels: in/out are a Gaussian's 48 floats, sh[3 j + channel]
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
#pragma unroll
        for (int i = 0; i < M_DIM; ++i) {
            float acc = M[i * M_DIM] * in[3 * j0 + ch];
#pragma unroll
            for (int j = 1; j < M_DIM; ++j) acc = acc + M[i * M_DIM + j] * in[3 * (j0 + j) + ch];
            out[3 * (j0 + i) + ch] = acc;
        }
}

__global__ __launch_bounds__(BLOCK) void k_scene_transform(SceneTransform x, float* blob, uint32_t stride, uint32_t first, uint32_t count) {
    __shared__ __attribute__((aligned(16))) float s_sh[BLOCK * kShRowLds];
    const uint32_t g0 = blockIdx.x * BLOCK, t = threadIdx.x, i = g0 + t;  // g0 < count: the grid covers the range
    const size_t N = stride;
    const uint32_t chunks = min((uint32_t)BLOCK, count - g0) * 12u;  // 16-byte pieces of the workgroup's rows
    float4* rows = reinterpret_cast<float4*>(blob + (size_t)P_SH * N + ((size_t)first + g0) * 48u);
    for (uint32_t q = t; q < chunks; q += BLOCK) {
        const uint32_t r = q / 12u, c = q - r * 12u;
        reinterpret_cast<float4*>(s_sh + r * kShRowLds)[c] = rows[q];
    }
    if (i < count) {
        float* p = blob + first + i;
        const float px = p[(P_POS + 0) * N], py = p[(P_POS + 1) * N], pz = p[(P_POS + 2) * N];
        const float sx = p[(P_SCALE + 0) * N], sy = p[(P_SCALE + 1) * N], sz = p[(P_SCALE + 2) * N];
        const float bw = p[(P_ROT + 0) * N], bx = p[(P_ROT + 1) * N], by = p[(P_ROT + 2) * N], bz = p[(P_ROT + 3) * N];
#pragma unroll
        for (int k = 0; k < 3; ++k) p[(P_POS + k) * N] = x.s * ((x.R[3 * k] * px + x.R[3 * k + 1] * py) + x.R[3 * k + 2] * pz) + x.t[k];
        p[(P_SCALE + 0) * N] = x.s * sx;
        p[(P_SCALE + 1) * N] = x.s * sy;
        p[(P_SCALE + 2) * N] = x.s * sz;
        const float aw = x.q[0], ax = x.q[1], ay = x.q[2], az = x.q[3];
        const float vw = ((aw * bw - ax * bx) - ay * by) - az * bz;
        const float vx = ((aw * bx + ax * bw) + ay * bz) - az * by;
        const float vy = ((aw * by - ax * bz) + ay * bw) + az * bx;
        const float vz = ((aw * bz + ax * by) - ay * bx) + az * bw;
        const float dot = (vw * vw + vx * vx) + (vy * vy + vz * vz);
        const float inv = 1.0f / sqrtf(dot);  // both correctly rounded (hipcc's default; no fast-math in this build)
        p[(P_ROT + 0) * N] = vw * inv;
        p[(P_ROT + 1) * N] = vx * inv;
        p[(P_ROT + 2) * N] = vy * inv;
        p[(P_ROT + 3) * N] = vz * inv;
    }
    __syncthreads();
    if (i < count) {
        // volatile: each access stays ONE 16-byte ds_read_b128 / ds_write_b128.  Left to itself the compiler drops the DC term's
        // round trip, starts at dword 3 and emits 45 dwords as ds_read2_b32 / ds_write2_b32 pairs, whose 32-lane groups (banks
        // mod 32) are 4-way conflicted at this stride.
        // (the pointer carries the LDS address space itself: a volatile access through a generic pointer is a flat_load)
        LdsShChunk* row = (LdsShChunk*)(s_sh + t * kShRowLds);
        float in[48], out[48];
#pragma unroll
        for (int c = 0; c < 12; ++c) {
            const ShChunk v = row[c];
            in[4 * c] = v.x, in[4 * c + 1] = v.y, in[4 * c + 2] = v.z, in[4 * c + 3] = v.w;
        }
        out[0] = in[0], out[1] = in[1], out[2] = in[2];
        sh_band_rotate<3>(x.M, in, out, 1);
        sh_band_rotate<5>(x.M + 9, in, out, 4);
        sh_band_rotate<7>(x.M + 34, in, out, 9);
#pragma unroll
        for (int c = 0; c < 12; ++c) {
            ShChunk v;
            v.x = out[4 * c], v.y = out[4 * c + 1], v.z = out[4 * c + 2], v.w = out[4 * c + 3];
            row[c] = v;
        }
    }
    __syncthreads();
    for (uint32_t q = t; q < chunks; q += BLOCK) {
        const uint32_t r = q / 12u, c = q - r * 12u;
        rows[q] = reinterpret_cast<const float4*>(s_sh + r * kShRowLds)[c];
    }
}

void launch_scene_transform(const SceneTransform& x, float* blob, uint32_t stride, uint32_t first, uint32_t count, hipStream_t s) {
    if (count == 0) return;
    hipLaunchKernelGGL(k_scene_transform, dim3((count + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, x, blob, stride, first, count);
}

// ---------------------------------------------------------------------------------------
// Export (gs_scene_to_device_arrays, gs_scene_download_records, gs_scene_save_ply): the blob -> PLY-domain values, the inverse
// of k_ingest_arrays.  No reference counterpart (GSScene only loads).
// ---------------------------------------------------------------------------------------
// THE INVERSE ACTIVATION, bit for bit gs_host_math.h's export_log_scale / export_opacity_logit (tests/export_reference.py
// restates it in numpy).  ARITHMETIC (binary64 + - x /, -ffp-contract=off: every operation below rounded on its own, in this
// order; no fma, no library log):
//     log64(v), v = m 2^e with m in [1/2, 1):   if m < 0x1.6a09e667f3bcdp-1:  m = 2 m, e = e - 1
//         t = (m - 1) / (m + 1);   w = t t
//         p = 1/17;  p = p w + 1/15;  p = p w + 1/13;  .. 1/11, 1/9, 1/7, 1/5, 1/3;  p = p w + 1    (1/k: the binary64 quotient)
//         log64 = (double)e * 0x1.62e42fefa39efp-1 + (2 t) p
//     x0 = (float)log64(s)   |   x0 = (float)log64(o / (1 - o)),  o, 1 - o and the quotient in binary64
//     candidates x0 and its binary32 neighbours in the order 0, -1, +1, -2, +2, -3, +3, -4, +4 (non-finite ones skipped), each
//         activated exactly as k_ingest_arrays activates (gs_expf_libm_domain; 1.0f / (1.0f + exp(-x)));  the export is the first
//         with the strictly smallest |(double)act - (double)stored|;  a NaN activation never wins.
//     The loop stops at a candidate whose activation IS the stored value: distance 0 cannot be beaten, so the result is the one
//     the full window gives, and on images of the activation (every scene that was loaded, not transformed) a scale costs one
//     exp and an opacity at most five instead of nine each.
//     s == 0 -> -inf;  s == +inf -> +inf;  s < 0 or NaN -> NaN;   o == 0 -> -inf;  o == 1 -> +inf;  o outside [0, 1] or NaN -> NaN.
__device__ __forceinline__ double export_log64(double v) {  // v: positive, finite, normal
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    int e = (int)((b >> 52) & 0x7FFu) - 1022;
    double m = __longlong_as_double((long long)((b & 0x000FFFFFFFFFFFFFull) | 0x3FE0000000000000ull));
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
    return (double)e * 0x1.62e42fefa39efp-1 + (2.0 * t) * p;
}

// the binary32 value d steps from x in the order of the reals (+-0 is one value; a step from it lands on a subnormal)
__device__ __forceinline__ float export_neighbour(float x, int d) {
    const uint32_t b = __float_as_uint(x);
    const int64_t key = ((b & 0x80000000u) ? -(int64_t)(b & 0x7FFFFFFFu) : (int64_t)b) + d;
    return __uint_as_float(key < 0 ? (0x80000000u | (uint32_t)(-key)) : (uint32_t)key);
}

template <bool OPACITY>
__device__ __forceinline__ float export_polish(float x0, float stored, const uint2* __restrict__ tab) {
    float best = x0;
    double best_err = __longlong_as_double(0x7FF0000000000000ll);
    for (int k = 0; k < 9; ++k) {
        const float c = export_neighbour(x0, (k & 1) ? -((k + 1) >> 1) : (k >> 1));
        if ((__float_as_uint(c) & 0x7F800000u) == 0x7F800000u) continue;
        const float act = OPACITY ? 1.0f / (1.0f + gs_expf_libm_domain(-c, tab)) : gs_expf_libm_domain(c, tab);
        const double diff = (double)act - (double)stored;
        const double err = diff < 0.0 ? -diff : diff;
        if (err < best_err) best = c, best_err = err;  // (false for a NaN)
        if (err == 0.0) break;
    }
    return best;
}

__device__ __forceinline__ float export_log_scale(float s, const uint2* __restrict__ tab) {
    if (!(s > 0.0f)) return __uint_as_float(s == 0.0f ? 0xFF800000u : 0x7FC00000u);
    if (s == __uint_as_float(0x7F800000u)) return s;
    return export_polish<false>((float)export_log64((double)s), s, tab);
}

__device__ __forceinline__ float export_opacity_logit(float o, const uint2* __restrict__ tab) {
    if (o == 0.0f) return __uint_as_float(0xFF800000u);
    if (o == 1.0f) return __uint_as_float(0x7F800000u);
    if (!(o > 0.0f && o < 1.0f)) return __uint_as_float(0x7FC00000u);
    const double od = (double)o, rest = 1.0 - od;
    return export_polish<true>((float)export_log64(od / rest), o, tab);
}

// k_scene_export, the mirror of k_ingest_arrays: one workgroup takes BLOCK consecutive Gaussians of the range; Gaussian i of the
// output is Gaussian first + i of the scene.  Two output forms over ONE body: the trainer's six arrays (RECORDS false; a null
// member is a wave-uniform branch that skips its loads and its arithmetic) and 62-float PLY records (RECORDS true).
//   * the planes are read lane-contiguous; each lane inverts its own Gaussian's three scales and its opacity;
//   * every packed output -- [n][3], [n][4], [n][k][3], the 62-float rows -- is a run of floats whose start is only 4-byte
//     aligned: the values are assembled in LDS and the run is written dword by dword, lane-contiguous.  Position and scale sit
//     at a stride of 3 dwords (conflict-free on 32 banks), the quaternion is put down as one 16-byte ds_write_b128 per lane
//     (contiguous), as the ingest picks it up;
//   * the SH rows (192 bytes, 16-byte aligned in the blob; the workgroup's rows are one run of bytes) are read as whole
//     16-byte loads into LDS at kShRowLds dwords per row (k_scene_transform: why 52 and not 48).  sh_rest takes floats
//     3 .. 3 + 3 k of each row, consecutive lanes consecutive dwords; a record's planar f_rest takes float 3 + 3 j + channel
//     for consecutive j, a stride of 3 dwords.  When only the DC term is wanted only the rows' first 16 bytes are read.
// It writes nothing but the outputs and reads the fp32 SH block whatever the scene renders from.
// COST: DESIGN.md section 3b (tools/scene_export_rate.py, profiles/r13_scene_export.txt).
struct SceneExport {
    gs_device_arrays_out a;  // RECORDS false
    float* records;          // RECORDS true: [count][62]
};

template <bool RECORDS>
__global__ __launch_bounds__(BLOCK) void k_scene_export(SceneExport x, const float* __restrict__ blob, uint32_t stride, uint32_t first,
                                                        uint32_t count) {
    __shared__ float s_pos[3 * BLOCK], s_scale[3 * BLOCK], s_op[BLOCK];
    __shared__ __attribute__((aligned(16))) float s_rot[4 * BLOCK];
    __shared__ __attribute__((aligned(16))) float s_sh[BLOCK * kShRowLds];
    const gs_device_arrays_out& a = x.a;
    const uint32_t g0 = blockIdx.x * BLOCK, t = threadIdx.x, i = g0 + t;  // g0 < count: the grid covers the range
    const size_t N = stride;
    const uint32_t left = count - g0, in_block = min((uint32_t)BLOCK, left);  // Gaussians from g0 on; those of this workgroup
    const uint32_t k3 = RECORDS ? 45u : (a.sh_rest ? 3u * a.sh_rest_coeffs : 0u);
    const bool want_pos = RECORDS || a.means, want_scale = RECORDS || a.log_scales, want_rot = RECORDS || a.quats;
    const bool want_op = RECORDS || a.opacity_logits, want_sh = RECORDS || a.sh_dc || k3 != 0u;

    if (want_sh) {
        // whole rows (12 pieces of 16 bytes each, one run of bytes over the workgroup), or each row's first piece alone; the
        // loads are issued together and put down once they have arrived
        const bool whole = k3 != 0u;
        const uint32_t pieces = in_block * (whole ? 12u : 1u);
        const float4* rows = reinterpret_cast<const float4*>(blob + (size_t)P_SH * N + ((size_t)first + g0) * 48u);
        // (q is clamped: a lane beyond the end repeats the last piece, load and store, so that neither is conditional -- under
        // a condition the compiler sinks each load to its store and the twelve wait for one another)
        float4 v[12];
#pragma unroll
        for (uint32_t k = 0; k < 12; ++k) {
            const uint32_t q = min(k * BLOCK + t, pieces - 1u);
            v[k] = rows[whole ? q : 12u * q];
        }
#pragma unroll
        for (uint32_t k = 0; k < 12; ++k) {
            const uint32_t q = min(k * BLOCK + t, pieces - 1u), r = whole ? q / 12u : q, c = whole ? q - r * 12u : 0u;
            reinterpret_cast<float4*>(s_sh + r * kShRowLds)[c] = v[k];
        }
    }
    if (i < count) {
        const uint2* tab = reinterpret_cast<const uint2*>(kExpfTab);
        const float* p = blob + first + i;
        // every plane's load is issued before the first inversion waits for one
        float sc[3] = {0.0f, 0.0f, 0.0f}, o = 0.0f;
        if (want_scale) {
#pragma unroll
            for (int k = 0; k < 3; ++k) sc[k] = p[(P_SCALE + k) * N];
        }
        if (want_op) o = p[P_OPACITY * N];
        if (want_pos) {
#pragma unroll
            for (int k = 0; k < 3; ++k) s_pos[3 * t + k] = p[(P_POS + k) * N];
        }
        if (want_rot)
            reinterpret_cast<float4*>(s_rot)[t] = make_float4(p[(P_ROT + 0) * N], p[(P_ROT + 1) * N], p[(P_ROT + 2) * N], p[(P_ROT + 3) * N]);
        if (want_scale) {
            for (int k = 0; k < 3; ++k) s_scale[3 * t + k] = export_log_scale(sc[k], tab);
        }
        if (want_op) {
            const float logit = export_opacity_logit(o, tab);
            if (RECORDS) s_op[t] = logit;
            else a.opacity_logits[i] = logit;
        }
    }
    __syncthreads();
    if (RECORDS) {
        float* out = x.records + (size_t)g0 * 62u;
#pragma unroll 2
        for (uint32_t j = t; j < in_block * 62u; j += BLOCK) {
            const uint32_t g = j / 62u, f = j - g * 62u;
            float v;
            if (f < 3u) v = s_pos[3u * g + f];
            else if (f < 6u) v = 0.0f;  // normals
            else if (f < 9u) v = s_sh[g * kShRowLds + (f - 6u)];
            else if (f < 54u) {  // planar f_rest: 15 R, 15 G, 15 B  <-  sh[3 j + channel]  (activate_record, inverted)
                const uint32_t ch = (f - 9u) / 15u, c = (f - 9u) - ch * 15u;
                v = s_sh[g * kShRowLds + 3u + 3u * c + ch];
            } else if (f == 54u) v = s_op[g];
            else if (f < 58u) v = s_scale[3u * g + (f - 55u)];
            else v = s_rot[4u * g + (f - 58u)];
            out[j] = v;
        }
        return;
    }
    for (uint32_t j = t; j < in_block * 4u; j += BLOCK) {
        if (a.means && j < in_block * 3u) a.means[(size_t)g0 * 3u + j] = s_pos[j];
        if (a.log_scales && j < in_block * 3u) a.log_scales[(size_t)g0 * 3u + j] = s_scale[j];
        if (a.quats) a.quats[(size_t)g0 * 4u + j] = s_rot[j];
        if (a.sh_dc && j < in_block * 3u) a.sh_dc[(size_t)g0 * 3u + j] = s_sh[(j / 3u) * kShRowLds + (j - (j / 3u) * 3u)];
    }
#pragma unroll 3
    for (uint32_t j = t; j < in_block * k3; j += BLOCK) {
        const uint32_t g = j / k3;
        a.sh_rest[(size_t)g0 * k3 + j] = s_sh[g * kShRowLds + 3u + (j - g * k3)];
    }
}

void launch_scene_export(const gs_device_arrays_out& a, const float* blob, uint32_t stride, uint32_t first, uint32_t count, hipStream_t s) {
    if (count == 0) return;
    SceneExport x = {a, nullptr};
    hipLaunchKernelGGL(k_scene_export<false>, dim3((count + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, x, blob, stride, first, count);
}
void launch_scene_export_records(float* records, const float* blob, uint32_t stride, uint32_t first, uint32_t count, hipStream_t s) {
    if (count == 0) return;
    SceneExport x = {};
    x.records = records;
    hipLaunchKernelGGL(k_scene_export<true>, dim3((count + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, x, blob, stride, first, count);
}

// ---- test hook: gs_expf_libm_domain over ranges of binary32 bit patterns, checksummed per block of 2^20 exactly as
// gs_debug_expf_scan does for the blend's function (tests/test_gpu_device_arrays.py)
__global__ __launch_bounds__(BLOCK) void k_activation_expf_scan(uint32_t first_bits, uint64_t count, unsigned long long* __restrict__ block_sums) {
    const uint64_t base = (uint64_t)blockIdx.x << 20;
    unsigned long long sum = 0;
    for (uint32_t j = threadIdx.x; j < (1u << 20); j += BLOCK) {
        const uint64_t at = base + j;
        if (at >= count) break;
        const uint32_t xb = first_bits + (uint32_t)at;
        const float y = gs_expf_libm_domain(__uint_as_float(xb), reinterpret_cast<const uint2*>(kExpfTab));
        sum += (unsigned long long)__float_as_uint(y) * (unsigned long long)((xb * 0x9E3779B1u) | 1u);
    }
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, WAVE);
    if ((threadIdx.x & (WAVE - 1)) == 0) atomicAdd(&block_sums[blockIdx.x], sum);
}

extern "C" int gs_debug_activation_expf_scan(int device, uint32_t first_bits, uint64_t count, uint64_t* block_sums, uint64_t blocks_capacity) {
    const uint64_t blocks = (count + (1u << 20) - 1) >> 20;
    if (blocks == 0 || blocks > blocks_capacity || !block_sums || blocks > 0x7FFFFFFFull) return GS_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess) return GS_ERR_DEVICE;
    unsigned long long* d = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&d), blocks * sizeof(unsigned long long)) != hipSuccess) return GS_ERR_NOMEM;
    int rc = GS_OK;
    if (hipMemset(d, 0, blocks * sizeof(unsigned long long)) != hipSuccess) rc = GS_ERR_DEVICE;
    if (rc == GS_OK) {
        hipLaunchKernelGGL(k_activation_expf_scan, dim3((uint32_t)blocks), dim3(BLOCK), 0, nullptr, first_bits, count, d);
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) rc = GS_ERR_DEVICE;
    }
    if (rc == GS_OK && hipMemcpy(block_sums, d, blocks * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) rc = GS_ERR_DEVICE;
    (void)hipFree(d);
    return rc;
}
}  // namespace gs
