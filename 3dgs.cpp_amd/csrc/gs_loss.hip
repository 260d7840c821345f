// gs_loss.hip -- k_loss_ssim, k_loss_grad, k_loss_l1, k_loss_finish: the photometric loss of a trainer's step
// (gs_photometric_loss, gs3d_hip.h):  loss = (1 - lambda) L1 + lambda (1 - SSIM)  of an image against a target, 11 x 11 Gaussian
// window (sigma 1.5), zeros outside the image, and d loss / d image as the [height][width][3] binary32 map gs_blend_backward takes.
// No reference counterpart.
//
// Part of libgs3d_hip.so (gfx950 only), built with -ffp-contract=off: every fused multiply-add below is written out
// (__builtin_fma), every other operation rounds on its own.  Binary64 throughout, on exact conversions of the binary32 pixels; a
// product of two pixels is exact in binary64.
//
// SHAPE.  A workgroup of kLossThreads = 256 lanes owns a tile of kLossTile x kLossTile pixels, all three channels: a tile row is
// 48 consecutive values of an interleaved image, and a window tap one pixel to the right is 3 values on.
//   k_loss_ssim<MAPS>   loads the tile and a halo of 5 pixels of BOTH images as binary32 into LDS (26 rows x 78 values each; a
//                       value outside the image is the zero of the padding and is never read from memory), runs the horizontal
//                       11-tap pass of the five maps x, y, x^2, y^2, xy over the 26 rows into LDS (binary64), the vertical pass
//                       for the lane's three outputs, and forms S, P1, P2, P3.  MAPS: the three P maps go to the renderer's
//                       scratch as planes of binary64 (form (a) of DESIGN.md 3j).  The lane's |x - y|, S and (x - y)^2 are summed
//                       over the wave (wave_sum_f64), the four waves meet in LDS in wave order, and the workgroup writes ONE ROW
//                       of three partial sums with ordinary vector stores.
//   k_loss_grad         per map in turn: loads the P map's tile and halo from the scratch (zero outside the image), horizontal
//                       then vertical pass; then  grad = c_l1 sign(x - y) - c_ssim (P1* + 2 x P2* + y P3*)  rounded once to binary32.
//   k_loss_l1<GRAD>     lambda = 0: no window is evaluated.  One strided pass: the L1 and squared-error partial sums and, GRAD,
//                       grad = c_l1 sign(x - y).
//   k_loss_finish       one workgroup: lane t adds rows t, t + 256, ... of the partial sums in index order, the wave sums its
//                       lanes, the waves are added in wave order, lane 0 forms the four terms.
// No atomics anywhere: the association is fixed by the image size, so two calls give the same bits.
// RESOURCES (tools/resource_usage.sh, profiles/photometric_loss_resource_usage.txt): no scratch memory (no spills).
#include "gs_device.h"
#include "gs_wave_f64.h"

namespace gs {

constexpr int kLossTile = 16;                           // pixels per side of a workgroup's tile
constexpr int kLossRadius = 5;                          // the window is 11 x 11
constexpr int kLossTaps = 2 * kLossRadius + 1;
constexpr int kLossRows = kLossTile + 2 * kLossRadius;  // 26 rows of the tile and its halo
constexpr int kLossCols = kLossTile * 3;                // 48 channel values of a tile row
constexpr int kLossHaloCols = kLossRows * 3;            // 78 channel values of a row with its halo
constexpr int kLossThreads = 256;
constexpr int kLossOutputs = kLossTile * kLossCols / kLossThreads;  // 3 outputs per lane
constexpr int kLossTerms = 3;                           // partial sums of a row: sum |x - y|, sum S, sum (x - y)^2
constexpr uint32_t kLossL1Groups = 2048;                // k_loss_l1's grid is at most this many workgroups, striding
static_assert(kLossOutputs * kLossThreads == kLossTile * kLossCols, "every lane forms the same number of outputs");

// g[k] = exp(-(k - 5)^2 / 4.5) / sum, the binary64 rounding of the exact value; g[10 - k] = g[k].
__device__ __forceinline__ double loss_tap(int k) {
    constexpr double g[6] = {0x1.0d956b52a1d6fp-10, 0x1.f1fe01ae5a5b7p-8, 0x1.26eb175d83f66p-5,
                             0x1.bff0fe8e98418p-4,  0x1.b43c3f52b19f2p-3, 0x1.106560aa892c0p-2};
    return g[k <= kLossRadius ? k : 2 * kLossRadius - k];
}

size_t photo_loss_groups(int width, int height) {
    return (size_t)((width + kLossTile - 1) / kLossTile) * (size_t)((height + kLossTile - 1) / kLossTile);
}
size_t photo_loss_partials(int width, int height) { return std::max<size_t>(photo_loss_groups(width, height), kLossL1Groups) * kLossTerms; }
size_t photo_loss_maps(int width, int height) { return (size_t)3 * 3 * (size_t)width * (size_t)height; }

struct LossImages {
    const float* x;   // image:  [height][width][sx]
    const float* y;   // target: [height][width][sy]
    int width, height, sx, sy;
};

// The workgroup's three sums: wave sums (every lane active), the four waves added in wave order, one row of partials.
__device__ __forceinline__ void loss_write_partials(double (&acc)[kLossTerms], double (*s_wave)[kLossTerms], double* row) {
    const uint32_t wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
#pragma unroll
    for (int e = 0; e < kLossTerms; ++e) {
        const double s = wave_sum_f64(acc[e]);
        if (lane == 0) s_wave[wave][e] = s;
    }
    __syncthreads();
    if (threadIdx.x < kLossTerms) {
        const uint32_t e = threadIdx.x;
        row[e] = ((s_wave[0][e] + s_wave[1][e]) + s_wave[2][e]) + s_wave[3][e];
    }
}

template <bool MAPS>
__global__ __launch_bounds__(kLossThreads) void k_loss_ssim(LossImages im, double* __restrict__ maps, double* __restrict__ partials) {
    __shared__ float s_x[kLossRows][kLossHaloCols], s_y[kLossRows][kLossHaloCols];
    __shared__ double s_h[5][kLossRows][kLossCols];   // the horizontal pass of x, y, x^2, y^2, xy
    __shared__ double s_wave[kLossThreads / WAVE][kLossTerms];
    const int x0 = (int)blockIdx.x * kLossTile, y0 = (int)blockIdx.y * kLossTile;

    for (int i = threadIdx.x; i < kLossRows * kLossHaloCols; i += kLossThreads) {
        const int r = i / kLossHaloCols, c = i - r * kLossHaloCols;
        const int px = x0 - kLossRadius + c / 3, py = y0 - kLossRadius + r, ch = c % 3;
        float vx = 0.0f, vy = 0.0f;   // (the padding: a zero, not a product with data)
        if (px >= 0 && px < im.width && py >= 0 && py < im.height) {
            const size_t p = (size_t)py * (size_t)im.width + (size_t)px;
            vx = im.x[p * (size_t)im.sx + ch], vy = im.y[p * (size_t)im.sy + ch];
        }
        s_x[r][c] = vx, s_y[r][c] = vy;
    }
    __syncthreads();

    for (int i = threadIdx.x; i < kLossRows * kLossCols; i += kLossThreads) {
        const int r = i / kLossCols, c = i - r * kLossCols;
        double m1 = 0.0, m2 = 0.0, e11 = 0.0, e22 = 0.0, e12 = 0.0;
#pragma unroll
        for (int k = 0; k < kLossTaps; ++k) {
            const double g = loss_tap(k), xv = (double)s_x[r][c + 3 * k], yv = (double)s_y[r][c + 3 * k];
            m1 = __builtin_fma(g, xv, m1), m2 = __builtin_fma(g, yv, m2);
            e11 = __builtin_fma(g, xv * xv, e11), e22 = __builtin_fma(g, yv * yv, e22), e12 = __builtin_fma(g, xv * yv, e12);
        }
        s_h[0][r][c] = m1, s_h[1][r][c] = m2, s_h[2][r][c] = e11, s_h[3][r][c] = e22, s_h[4][r][c] = e12;
    }
    __syncthreads();

    double acc[kLossTerms] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < kLossOutputs; ++j) {
        const int i = (int)threadIdx.x + j * kLossThreads, r = i / kLossCols, c = i - r * kLossCols;
        const int px = x0 + c / 3, py = y0 + r;
        double m1 = 0.0, m2 = 0.0, e11 = 0.0, e22 = 0.0, e12 = 0.0;
#pragma unroll
        for (int k = 0; k < kLossTaps; ++k) {
            const double g = loss_tap(k);
            m1 = __builtin_fma(g, s_h[0][r + k][c], m1), m2 = __builtin_fma(g, s_h[1][r + k][c], m2);
            e11 = __builtin_fma(g, s_h[2][r + k][c], e11), e22 = __builtin_fma(g, s_h[3][r + k][c], e22);
            e12 = __builtin_fma(g, s_h[4][r + k][c], e12);
        }
        if (px >= im.width || py >= im.height) continue;   // (the tile overhangs the image: nothing is summed or written)
        const double C1 = 1e-4, C2 = 9e-4;
        const double m12 = m1 * m2, m11 = m1 * m1, m22 = m2 * m2;
        const double s11 = e11 - m11, s22 = e22 - m22, s12 = e12 - m12;
        const double A = 2.0 * m12 + C1, B = 2.0 * s12 + C2, Cc = (m11 + m22) + C1, D = (s11 + s22) + C2;
        const double rc = 1.0 / Cc, rd = 1.0 / D, rcd = rc * rd;
        const double S = (A * B) * rcd;
        const double xv = (double)s_x[r + kLossRadius][c + 3 * kLossRadius], yv = (double)s_y[r + kLossRadius][c + 3 * kLossRadius];
        const double d = xv - yv;
        acc[0] = acc[0] + fabs(d), acc[1] = acc[1] + S, acc[2] = acc[2] + d * d;
        if (MAPS) {
            const size_t plane = (size_t)3 * (size_t)im.width * (size_t)im.height;
            const size_t at = ((size_t)py * (size_t)im.width + (size_t)px) * 3 + (size_t)(c % 3);
            maps[at] = (2.0 * m2) * (B - A) * rcd + ((2.0 * m1) * S) * (rd - rc);   // P1
            maps[plane + at] = -(S * rd);                                             // P2
            maps[2 * plane + at] = (2.0 * A) * rcd;                                   // P3
        }
    }
    // (the lanes have met again: every lane of the wave is active for the DPP moves)
    loss_write_partials(acc, s_wave, partials + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kLossTerms);
}

__global__ __launch_bounds__(kLossThreads) void k_loss_grad(LossImages im, const double* __restrict__ maps, double c_l1, double c_ssim,
                                                            float* __restrict__ grad) {
    __shared__ double s_p[kLossRows][kLossHaloCols];
    __shared__ double s_h[kLossRows][kLossCols];
    const int x0 = (int)blockIdx.x * kLossTile, y0 = (int)blockIdx.y * kLossTile;
    const size_t plane = (size_t)3 * (size_t)im.width * (size_t)im.height;
    // the lane's three outputs: their pixels of both images first (the loads fly while the maps are convolved)
    double xv[kLossOutputs], yv[kLossOutputs], sign[kLossOutputs], G[kLossOutputs];
    size_t at[kLossOutputs];
    bool inside[kLossOutputs];
#pragma unroll
    for (int j = 0; j < kLossOutputs; ++j) {
        const int i = (int)threadIdx.x + j * kLossThreads, r = i / kLossCols, c = i - r * kLossCols;
        const int px = x0 + c / 3, py = y0 + r;
        inside[j] = px < im.width && py < im.height;   // (the tile may overhang the image: nothing is read or written there)
        const size_t p = inside[j] ? (size_t)py * (size_t)im.width + (size_t)px : 0;
        const float xf = im.x[p * (size_t)im.sx + c % 3], yf = im.y[p * (size_t)im.sy + c % 3];
        xv[j] = (double)xf, yv[j] = (double)yf, at[j] = p * 3 + c % 3, G[j] = 0.0;
        sign[j] = xf > yf ? 1.0 : (xf < yf ? -1.0 : 0.0);   // sign(0) = 0; an unordered pair takes the window's NaN below
    }

#pragma unroll 1
    for (int m = 0; m < 3; ++m) {
        // (s_p is free: the horizontal pass that read it lies behind the barrier in front of the last vertical pass)
        for (int i = threadIdx.x; i < kLossRows * kLossHaloCols; i += kLossThreads) {
            const int r = i / kLossHaloCols, c = i - r * kLossHaloCols;
            const int px = x0 - kLossRadius + c / 3, py = y0 - kLossRadius + r;
            double v = 0.0;
            if (px >= 0 && px < im.width && py >= 0 && py < im.height)
                v = maps[(size_t)m * plane + ((size_t)py * (size_t)im.width + (size_t)px) * 3 + (size_t)(c % 3)];
            s_p[r][c] = v;
        }
        __syncthreads();   // (also: every lane has finished the vertical pass over the previous map's s_h)
        for (int i = threadIdx.x; i < kLossRows * kLossCols; i += kLossThreads) {
            const int r = i / kLossCols, c = i - r * kLossCols;
            double h = 0.0;
#pragma unroll
            for (int k = 0; k < kLossTaps; ++k) h = __builtin_fma(loss_tap(k), s_p[r][c + 3 * k], h);
            s_h[r][c] = h;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kLossOutputs; ++j) {
            const int i = (int)threadIdx.x + j * kLossThreads, r = i / kLossCols, c = i - r * kLossCols;
            double v = 0.0;
#pragma unroll
            for (int k = 0; k < kLossTaps; ++k) v = __builtin_fma(loss_tap(k), s_h[r + k][c], v);
            // G = P1* + 2 x P2* + y P3*
            const double coef = m == 0 ? 1.0 : (m == 1 ? 2.0 * xv[j] : yv[j]);
            G[j] = __builtin_fma(coef, v, G[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < kLossOutputs; ++j)
        if (inside[j]) grad[at[j]] = (float)(c_l1 * sign[j] - c_ssim * G[j]);
}

// lambda = 0.  Element e = 3 pixel + channel; lanes stride over the elements by the grid.
template <bool GRAD>
__global__ __launch_bounds__(kLossThreads) void k_loss_l1(LossImages im, double c_l1, float* __restrict__ grad, double* __restrict__ partials) {
    __shared__ double s_wave[kLossThreads / WAVE][kLossTerms];
    const size_t n = (size_t)3 * (size_t)im.width * (size_t)im.height;
    double acc[kLossTerms] = {0.0, 0.0, 0.0};
    for (size_t e = (size_t)blockIdx.x * kLossThreads + threadIdx.x; e < n; e += (size_t)gridDim.x * kLossThreads) {
        const size_t p = e / 3, ch = e - p * 3;
        const float xf = im.x[p * (size_t)im.sx + ch], yf = im.y[p * (size_t)im.sy + ch];
        const double d = (double)xf - (double)yf;
        acc[0] = acc[0] + fabs(d), acc[2] = acc[2] + d * d;
        if (GRAD) {
            const double sign = xf > yf ? 1.0 : (xf < yf ? -1.0 : 0.0);
            grad[e] = (float)(c_l1 * (d != d ? d : sign));   // (a NaN pixel: its own element is NaN, nothing else)
        }
    }
    loss_write_partials(acc, s_wave, partials + (size_t)blockIdx.x * kLossTerms);
}

// terms[0..3] = loss, l1, ssim, mse.  ssim_evaluated == 0 (lambda = 0): terms[2] is a quiet NaN and the loss is the L1 term.
__global__ __launch_bounds__(kLossThreads) void k_loss_finish(const double* __restrict__ partials, uint32_t rows, double n, double lambda,
                                                              int ssim_evaluated, double* __restrict__ terms) {
    __shared__ double s_wave[kLossThreads / WAVE][kLossTerms];
    double acc[kLossTerms] = {0.0, 0.0, 0.0};
#pragma unroll 8
    for (uint32_t r = threadIdx.x; r < rows; r += kLossThreads) {
#pragma unroll
        for (int e = 0; e < kLossTerms; ++e) acc[e] = acc[e] + partials[(size_t)r * kLossTerms + e];
    }
    const uint32_t wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
#pragma unroll
    for (int e = 0; e < kLossTerms; ++e) {
        const double s = wave_sum_f64(acc[e]);
        if (lane == 0) s_wave[wave][e] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t[kLossTerms];
#pragma unroll
        for (int e = 0; e < kLossTerms; ++e) t[e] = (((s_wave[0][e] + s_wave[1][e]) + s_wave[2][e]) + s_wave[3][e]) / n;
        const double l1 = t[0], mse = t[2];
        const double ssim = ssim_evaluated ? t[1] : __longlong_as_double(0x7FF8000000000000ll);
        terms[0] = ssim_evaluated ? (1.0 - lambda) * l1 + lambda * (1.0 - ssim) : l1;
        terms[1] = l1, terms[2] = ssim, terms[3] = mse;
    }
}

void launch_photo_loss(const gs_photo_loss& l, double* maps, double* partials, hipStream_t s) {
    const LossImages im{l.image, l.target, l.width, l.height, l.image_stride, l.target_stride};
    const double n = 3.0 * (double)l.width * (double)l.height;   // (exact: below 2^53)
    const double c_l1 = (1.0 - l.lambda_dssim) / n, c_ssim = l.lambda_dssim / n;
    uint32_t rows;
    if (l.lambda_dssim == 0.0) {
        const uint64_t lanes = (uint64_t)3 * (uint64_t)l.width * (uint64_t)l.height;
        rows = (uint32_t)std::min<uint64_t>((lanes + kLossThreads - 1) / kLossThreads, kLossL1Groups);
        if (l.grad_rgb) hipLaunchKernelGGL((k_loss_l1<true>), dim3(rows), dim3(kLossThreads), 0, s, im, c_l1, l.grad_rgb, partials);
        else hipLaunchKernelGGL((k_loss_l1<false>), dim3(rows), dim3(kLossThreads), 0, s, im, c_l1, l.grad_rgb, partials);
    } else {
        const dim3 grid((l.width + kLossTile - 1) / kLossTile, (l.height + kLossTile - 1) / kLossTile);
        rows = grid.x * grid.y;
        if (l.grad_rgb) {
            hipLaunchKernelGGL((k_loss_ssim<true>), grid, dim3(kLossThreads), 0, s, im, maps, partials);
            hipLaunchKernelGGL(k_loss_grad, grid, dim3(kLossThreads), 0, s, im, maps, c_l1, c_ssim, l.grad_rgb);
        } else {
            hipLaunchKernelGGL((k_loss_ssim<false>), grid, dim3(kLossThreads), 0, s, im, maps, partials);
        }
    }
    if (l.terms)
        hipLaunchKernelGGL(k_loss_finish, dim3(1), dim3(kLossThreads), 0, s, partials, rows, n, l.lambda_dssim, l.lambda_dssim != 0.0 ? 1 : 0, l.terms);
}

}  // namespace gs
