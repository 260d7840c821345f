// gs_tile_walk.h -- the walk of the last frame's tile lists that k_contrib (gs_contrib.hip), k_features (gs_features.hip),
// k_lift (gs_lift.hip) and k_blend_backward (gs_backward.hip) share, and the quadrant test they share with the blend
// (gs_blend.hip: blend_walk).
//
// Device code, included by those five translation units; built with -ffp-contract=off like them: every product and sum of the
// walk is rounded on its own.  Reference restated: render.comp:61-89 (the shader gs_blend.hip restates).  Each piece stands here
// ONCE, with the one comment that explains it: a change to the slack, to the record layout or to the exit rule is made here.
#pragma once
#include "gs_device.h"

namespace gs {

// ---------------------------------------------------------------------------------------
// The quadrant test.
// min over the pixel rectangle [xa,xb] x [ya,yb] of q(d) = 0.5 (c00 dx^2 + c11 dy^2) + c01 dx dy,
// d = uv - pixel.  q is convex with its minimum 0 at d = 0: inside the rectangle the answer is 0,
// otherwise the minimum lies on an edge facing the centre, where q is a 1-D parabola.
// h00 = c00 / 2, h11 = c11 / 2; r11 = -c01 rcp(c11), r00 = -c01 rcp(c00): the entry's own terms, carried in its record.
__device__ __forceinline__ float min_q_rect(float h00, float c01, float h11, float r11, float r00, float u, float v, float xa,
                                            float xb, float ya, float yb) {
    const float dx_lo = u - xb, dx_hi = u - xa, dy_lo = v - yb, dy_hi = v - ya;
    const bool in_x = !(dx_lo > 0.0f) && !(dx_hi < 0.0f), in_y = !(dy_lo > 0.0f) && !(dy_hi < 0.0f);  // NaN -> inside
    // This is a bound, not part of the pipeline's arithmetic: FMAs are welcome (the caller's slack covers rounding).
    // q(a, t) = h00 a^2 + t (h11 t + c01 a) with h = c / 2.  Only the edges that face the centre can hold the minimum
    // (a segment from the centre to a point of a far edge crosses a near edge, where the convex q is smaller): at most
    // one vertical and one horizontal edge; on an edge one coordinate is fixed and the other is the parabola's
    // minimiser r * fixed, clamped to the edge.
    const float a = dx_lo > 0.0f ? dx_lo : dx_hi;  // the vertical edge nearer to the centre: dx fixed, parabola in dy
    const float t = fminf(fmaxf(r11 * a, dy_lo), dy_hi);
    const float qv = __builtin_fmaf(t, __builtin_fmaf(h11, t, c01 * a), h00 * a * a);
    const float b = dy_lo > 0.0f ? dy_lo : dy_hi;  // the horizontal edge nearer to the centre
    const float s = fminf(fmaxf(r00 * b, dx_lo), dx_hi);
    const float qh = __builtin_fmaf(s, __builtin_fmaf(h00, s, c01 * b), h11 * b * b);
    // The cull `mq > lim` needs mq to be a LOWER bound of q over the quadrant, and evaluating the parabola at an inexact
    // minimiser (r11, r00 are v_rcp_f32's, 1 ULP, evaluated once per Gaussian in k_preprocess instead of once per wave and entry
    // here) OVER-estimates its minimum -- by a second-order amount: q(t* + dt) - q(t*) = h dt^2 with
    // dt/t* ~ 2^-23, i.e. ~1e-14 relative, which quadrant_keep's slack (9.6e-7 x the quadratic's largest terms) absorbs
    // many times over.  A coarser reciprocal or a smaller slack must revisit this.
    return in_x ? (in_y ? 0.0f : qh) : (in_y ? qv : fminf(qv, qh));
}

// Entry `lane` of a 64-entry chunk against the wave's quadrant [rx0, rx1] x [ry0, ry1]: the wave's mask of the entries that some
// pixel of the quadrant may keep.  An entry it drops is skipped by every pixel of the quadrant (power < cut there), so dropping
// it changes no bit.  h00, c01, h11: the conic with its diagonal halved (scaling by a power of two is exact, and
// |c / 2| = |c| / 2 bit for bit); cut, r11, r00, u, v: the record's; have: the lane holds an entry of the list.
// cut = +inf: no power <= 0 is kept (never enters); -inf (NaN or infinite opacity: min(0.99, NaN) is 0.99 in the pipeline's
// definition): never culled.
// (Every lane computes: the wave pays for these instructions as soon as one lane needs them, and the AND of scalar masks needs
//  no branch and no rebuilding from a VGPR; what a lane without an entry computes is never looked at.)
__device__ __forceinline__ uint64_t quadrant_keep(float h00, float c01, float h11, float cut, float r11, float r00, float u, float v,
                                                  bool have, float rx0, float rx1, float ry0, float ry1) {
    uint64_t bm = __builtin_amdgcn_ballot_w64(have) & __builtin_amdgcn_ballot_w64(cut <= 0.0f);
    const float mq = min_q_rect(h00, c01, h11, r11, r00, u, v, rx0, rx1, ry0, ry1);
    // The rounding error of the shader's `power` (and of mq) is relative to the TERMS c00 dx^2, c11 dy^2,
    // c01 dx dy, not to their sum: a thin diagonal splat far from its centre has terms ~1e5 cancelling to
    // q ~ 5.  The slack therefore grows with the terms at the quadrant's corner farthest from the centre
    // (16 roundings of 2^-24 each, generously).
    const float ax = fmaxf(fabsf(u - rx0), fabsf(u - rx1));
    const float ay = fmaxf(fabsf(v - ry0), fabsf(v - ry1));
    const float mag = __builtin_fmaf(fabsf(h00) * ax, ax, __builtin_fmaf(fabsf(h11) * ay, ay, fabsf(c01) * ax * ay));
    return bm & __builtin_amdgcn_ballot_w64(!(mq > __builtin_fmaf(mag, 9.6e-7f, -cut)));  // NaN -> keep
}

// ---------------------------------------------------------------------------------------
// The passes over the last frame's lists.  One workgroup of BLOCK threads per tile in tile_order, one pixel per lane, a wave per
// 8 x 8 quadrant: the blend's geometry, so quadrant_keep lets a wave skip the entries none of its pixels keeps.  The list is
// taken in chunks of 64 entries STAGED ONCE PER WORKGROUP: waves 0, 1, 2 put one 16-byte third of the 64 records each (the 48
// bytes the walk reads) into s_rec[3][WAVE], plane-major {c00 c01 c11 o} {u v r g} {b cut r11 r00}; wave 3 stages what the pass
// keeps beside them (the chunk's ids at least).
//
// Barriers.  Two per chunk (staged -> walk -> the pass's flush, and the next chunk may be staged), taken by ALL FOUR waves of the
// tile: a wave whose pixels have all broken (or that never had one to walk) walks nothing more but stays -- it is a part of the
// loader -- and says so ONCE in s_done (walk_begin, or the walk_chunk after which its `alive` reads 0); the workgroup leaves the
// loop together, at the chunk after whose second barrier s_done reads BLOCK / WAVE, or at the list's end.  s_done is written only
// between the two barriers of a chunk (and before the first chunk's), and read only after the second: the exit is uniform.  No
// wave ends early, so no barrier waits for a wave that has left (cf. gs_blend.hip's header), and no barrier follows the loop.
// Both __syncthreads() and the test of s_done stand in each kernel's own loop, never in a helper here.
// ---------------------------------------------------------------------------------------

// The pixel of a lane and the quadrant of its wave.
struct WalkPixel {
    int lane, w;              // lane of the wave, wave of the tile (= quadrant: bit 0 right, bit 1 lower)
    uint32_t tile;            // this workgroup's tile
    uint32_t px, py;
    bool inside;              // render.comp:36-39
    size_t p;                 // py * width + px (meaningful where `inside`)
    float fx, fy;
    float rx0, rx1, ry0, ry1; // the quadrant's pixel centres' rectangle
};

__device__ __forceinline__ WalkPixel walk_pixel(const uint32_t* __restrict__ tile_order, uint32_t width, uint32_t height,
                                                uint32_t tiles_x) {
    WalkPixel q;
    q.lane = threadIdx.x & (WAVE - 1);
    q.w = threadIdx.x / WAVE;
    q.tile = tile_order[blockIdx.x];
    const uint32_t tile_x = q.tile % tiles_x, tile_y = q.tile / tiles_x;
    const uint32_t qx0 = tile_x * kTile + (q.w & 1) * 8, qy0 = tile_y * kTile + (q.w >> 1) * 8;
    q.px = qx0 + (q.lane & 7);
    q.py = qy0 + (q.lane >> 3);
    q.inside = q.px < width && q.py < height;
    q.p = (size_t)q.py * width + q.px;
    q.fx = (float)q.px;
    q.fy = (float)q.py;
    q.rx0 = (float)qx0;
    q.ry0 = (float)qy0;
    q.rx1 = (float)qx0 + 7.0f;
    q.ry1 = (float)qy0 + 7.0f;
    return q;
}

// The workgroup's copy of kExpfTab and the zeroed s_done; the kernel's next barrier publishes both.
__device__ __forceinline__ void walk_init_shared(uint2* __restrict__ s_exptab, uint32_t* __restrict__ s_done) {
    const int tid = threadIdx.x;
    if (tid < 32) {
        const uint64_t v = kExpfTab[tid];
        s_exptab[tid] = make_uint2((uint32_t)v, (uint32_t)(v >> 32));
    }
    if (tid == 0) *s_done = 0;
}

// A mask made of ballots is the same in every lane; this says so where the compiler has lost track of it.  walk_chunk's `alive`
// is carried round two loops and past the lane-dependent branches of a pass's `blended` (lane 0's LDS atomics among them); where
// the compiler then takes it for a per-lane value it keeps it, and every mask derived from it, in vector registers, runs the pair
// loop under exec masks and sums the ballot's population count lane by lane.  (A mask that is already scalar costs nothing here.)
__device__ __forceinline__ uint64_t wave_uniform(uint64_t m) {
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(m >> 32)) << 32) |
           (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)m);
}

// `alive`: the wave's pixels that walk (`walks`: inside / counted) and have not broken.  After the barrier that published s_done.
__device__ __forceinline__ uint64_t walk_begin(bool walks, int lane, uint32_t* __restrict__ s_done) {
    const uint64_t alive = __builtin_amdgcn_ballot_w64(walks);
    if (alive == 0 && lane == 0) atomicAdd(s_done, 1u);
    return alive;
}

// The software pipeline over the chunks, as the blend's: ids two chunks ahead, this thread's 16-byte part of a record one chunk
// ahead, both in registers.  DEPTH: wave 3 also fetches the record's depth (the first float of its fourth 16-byte part) into
// r_nxt.x; otherwise wave 3 fetches nothing.  Use: prime(); per chunk, stage g_nxt / r_nxt, then advance(base).
template <bool DEPTH>
struct ListPipeline {
    const uint32_t* __restrict__ sorted_gid;
    const AttrRecord* __restrict__ rec;
    uint2 range;
    int lane, w;
    uint32_t g_nxt, g_next;  // ids of the chunk to stage next, of the chunk after it
    float4 r_nxt;            // this thread's part of record g_nxt

    __device__ __forceinline__ void fetch() {
        if (w < 3) r_nxt = reinterpret_cast<const float4*>(rec + g_nxt)[w];
        else if (DEPTH) r_nxt.x = rec[g_nxt].depth_radius.x;
    }
    __device__ __forceinline__ void prime() {
        g_nxt = g_next = 0;
        r_nxt = make_float4(0, 0, 0, 0);
        const uint32_t i0 = range.x + (uint32_t)lane;
        if (i0 < range.y) {
            g_nxt = sorted_gid[i0];
            fetch();
        }
        const uint32_t i1 = i0 + WAVE;
        if (i1 < range.y) g_next = sorted_gid[i1];
    }
    __device__ __forceinline__ void advance(uint32_t base) {
        const uint32_t i1 = base + WAVE + (uint32_t)lane;
        g_nxt = g_next;
        if (i1 < range.y) fetch();
        const uint32_t i2 = i1 + WAVE;
        if (i2 < range.y) g_next = sorted_gid[i2];
    }
};

// One wave's walk of the staged chunk (n_here entries), between the chunk's two barriers: render.comp:61-89 for the wave's alive
// pixels -- `power > 0` skips the entry (:68), `alpha < 1/255` skips it (:78, decided on `power` against the record's alpha cut, as
// every blend mode decides it), `T (1 - alpha) < 1e-4` ends the pixel's walk (:83) -- always with the REFERENCE's arithmetic,
// whatever mode the frame was blended in: `power` uncontracted, exp = gs_expf_libm.  For an entry k that some lane of the wave
// blends -- nothing is called for an empty ballot, the common case -- it calls
//     blended(k, bl, upd, alpha, test_T, T)
// with every lane of the wave active: bl the lanes that reach :87, upd this lane's bit of it, alpha and T as :87 reads them,
// test_T = T (1 - alpha).  The callable applies :88 itself -- T = test_T where upd -- after its last use of T.
// A wave with nobody alive walks nothing; one whose last pixel breaks here says so in s_done (see Barriers).
template <class Blended>
__device__ __forceinline__ void walk_chunk(const float4 (*__restrict__ s_rec)[WAVE], const uint2* __restrict__ s_exptab,
                                           uint32_t* __restrict__ s_done, const WalkPixel& q, uint32_t n_here, uint64_t& alive,
                                           float& T, Blended&& blended) {
    if (alive == 0) return;
    const int lane = q.lane;
    const float4 co = s_rec[0][lane], uv = s_rec[1][lane], bc = s_rec[2][lane];
    uint64_t bm = quadrant_keep(0.5f * co.x, co.y, 0.5f * co.z, bc.y, bc.z, bc.w, uv.x, uv.y, (uint32_t)lane < n_here, q.rx0, q.rx1,
                                q.ry0, q.ry1);
    while (bm) {
        const int k = __ffsll((unsigned long long)bm) - 1;
        bm &= bm - 1;
        const float4 e0 = s_rec[0][k], e1 = s_rec[1][k];
        const float ecut = s_rec[2][k].y;
        const float dx = e1.x - q.fx, dy = e1.y - q.fy;
        // :66  -0.5 * (c00 dx dx + c11 dy dy) - c01 dx dy, every product and sum rounded (the scaling by -0.5 is exact)
        const float cx = -0.5f * e0.x, cy = -e0.y, cz = -0.5f * e0.z;
        const float s = cx * dx * dx + cz * dy * dy;
        const float power = s + cy * dx * dy;
        // :68 and :78 (a NaN power skips the entry; power >= cut  <=>  alpha >= 1/255 with the reference's exp)
        const uint64_t m2 = alive & __builtin_amdgcn_ballot_w64(power <= 0.0f) & __builtin_amdgcn_ballot_w64(!(power < ecut));
        if (m2 == 0) continue;
        const float alpha = fminf(0.99f, e0.w * gs_expf_libm(power, s_exptab));  // :77
        const float test_T = T * (1 - alpha);
        const uint64_t mk = m2 & __builtin_amdgcn_ballot_w64(test_T < 0.0001f);  // :82-85 break
        const uint64_t bl = m2 & ~mk;                                            // lanes that reach :87
        if (bl != 0) blended(k, bl, (bool)__builtin_amdgcn_inverse_ballot_w64(bl), alpha, test_T, T);
        alive = wave_uniform(alive & ~mk);
        if (alive == 0) break;
    }
    if (alive == 0 && lane == 0) atomicAdd(s_done, 1u);
}

}  // namespace gs
