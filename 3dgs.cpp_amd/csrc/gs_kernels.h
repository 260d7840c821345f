// gs_kernels.h -- launch wrappers of the gfx950 kernels (gs_scene / gs_preprocess / gs_radix / gs_bin_l1 / gs_bin_l2 / gs_blend / gs_contrib / gs_features / gs_lift / gs_backward / gs_project_backward / gs_camera_backward / gs_loss / gs_optim / gs_densify / gs_knn .hip).
// Host-side declarations only; everything takes raw device pointers + a stream.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gs3d_hip.h"
#include "gs_levels.h"  // kTile, kBinSortLevels, kBinSlabLevel, kBinSortLimit

namespace gs {

constexpr int kSortTileKeys = 2048;   // keys per radix tile (256 threads x 8)
constexpr int kSortMaxBlocks = 1024;  // fixed sort grid (data-dependent sizes stay on the device)

// Packed scene blob (59 floats per Gaussian + padding): planes 0..10 are SoA with a plane stride of
// blob_stride(n) = n rounded up to 16 floats -- plane p of Gaussian i is blob[p*stride + i] -- followed by the SH
// block as AoS: the 48 SH floats of Gaussian i are blob[11*stride + 48*i .. +48).  With the blob itself 64-byte
// aligned, every plane and every Gaussian's 192-byte SH block start on a 64-byte line for any n.
enum ScenePlane { P_POS = 0, P_SCALE = 3, P_ROT = 6, P_OPACITY = 10, P_SH = 11, P_COUNT = 59 };
constexpr uint64_t blob_stride(uint64_t n) { return (n + 15) & ~uint64_t(15); }
constexpr uint64_t blob_floats(uint64_t n) { return P_SH * blob_stride(n) + 48 * n; }

struct SceneView {
    const float* blob;   // 11 planes of `stride` floats, then n x 48 SH floats
    const float* cov3d;  // 6 planes of n floats
    uint32_t n;
    uint32_t stride;     // blob_stride(n)
    const uint16_t* sh16;  // nullable: the SH block as binary16, n x 48 (gs_scene_quantize_sh); read instead of the fp32 one
    const float* acut;   // n floats: the alpha cut of every Gaussian (launch_alpha_cut), a function of its opacity, computed at load
    // Nullable.  The arrays above may hold the Gaussians in ANOTHER ORDER than the scene's (gs_scene: spatial / Morton order, so
    // that a wave's 64 Gaussians are neighbours in space: culled together, fetched together, binned together): Gaussian j of them
    // is Gaussian perm[j] of the scene, and everything a frame writes (tiles, depth, boxes, records, list entries) goes by THAT id.
    const uint32_t* perm;
};

// Per-frame buffers indexed by Gaussian id.
// What the blend gathers per list entry -- conic + opacity, uv + r g, b + alpha cut + r11 r00: 48 bytes -- lives in ONE 64-byte, 64-byte
// aligned record per Gaussian, so that an entry costs the memory system one line instead of three (three separate
// arrays measured 10 % slower in the blend and 9 % in the frame rate: the gathers are request-bound, not byte-bound).
// The record is the reference's VertexAttribute (common.glsl:42-49) in spirit; what the binning kernels stream or
// gather on their own (tiles, tile box, depth) additionally lives in dense arrays.
struct AttrRecord {
    float4 conic_op;   // c00 c01 c11 opacity
    float4 uv_rg;      // u v r g
    // b, alpha cut (the most negative `power` at which render.comp:78 keeps the entry), and the two entry-only terms of the
    // blend's quadrant test: r11 = -c01 rcp(c11), r00 = -c01 rcp(c00) (gs_tile_walk.h, min_q_rect), evaluated once per Gaussian
    // here instead of once per (wave, entry) there
    float4 b_cut_r;
    float4 depth_radius;  // depth, radius, 0, 0: read by the stage taps only (k_preprocess writes a record as one full 64-byte line)
};
static_assert(sizeof(AttrRecord) == 64, "one line per Gaussian");

struct AttrView {
    uint32_t* tiles;     // tiles_overlap (0 = culled)      } written by k_preprocess only when `vis` is null (the plane-input
    float* depth;        //                                 } level 1, the global path, bins of >= 16 x 16 tiles read them);
    ushort4* aabb;       //                                 } with the dense lists: rebuilt on demand for the stage taps
                         // (nor are they written by a frame of the one-pass level 1, L1Fused below: rebuilt from its records)
    AttrRecord* rec;     // written for visible Gaussians only
    // Optional (null: not written): the frame's visible Gaussians as DENSE lists in any order, 16 bytes each --
    // {id, depth bits, tile box x0 | y0 << 16, x1 | y1 << 16} -- which the level-1 kernels of the bin-local path stream
    // instead of walking the N-wide planes above (half of whose lanes are culled) with a dependent gather behind them.
    // kVisRegions lists of vis_region_slots slots each: workgroup b of k_preprocess appends to list b % kVisRegions, a wave
    // taking its run of slots with ONE atomic add on the list's counter, vis_count[region * kVisCounterStride].  (One list
    // with one counter was measured first: 94 k same-address atomics per frame at 6 M Gaussians retire at ~10 ns each and
    // k_preprocess took 1.1 ms instead of 0.27.)  The frame's last kernel (k_blend) zeroes the counters for the next frame.
    uint4* vis;
    uint32_t* vis_count;
    uint32_t vis_region_slots;
};
constexpr uint32_t kVisRegions = 256, kVisCounterStride = 32;  // a counter per 128 bytes
// slots per list for a scene of n Gaussians: what the workgroups (of 256) that append to it can hold, a whole number of level-1 blocks
uint32_t vis_region_slots(uint32_t n);

// The ONE-PASS level 1 (round 16; bin-local path, bins of <= 8 x 8 tiles, scenes below dense_min that have their spatial copy):
// k_preprocess files its visible Gaussians' candidate records itself, and k_l1_hist / k_l1_scan / k_l1_scatter_any_order are not
// launched.  Bin b -- counted over the ON-SCREEN bins, row by row -- owns the region [b cap, (b + 1) cap) of the candidate buffer,
// cap = cand_capacity / on-screen bins; a workgroup counts its Gaussians per bin in LDS and takes its run of every bin it touches
// with one returning atomic add on that bin's cursor.  The scene's spatial (Morton) copy is what makes this cheap: 256 consecutive
// Gaussians touch 4 bins or so, not 100 (profiles/r16_atomic_rate_sparse.txt).  `words`: one counter per 128 bytes -- kVisRegions
// counters of visible Gaussians (V, summed by level 2), then the cursor of every padded bin; the frame's last kernel (k_frame_end)
// zeroes them for the buffer set's next frame.  Such a frame's k_preprocess writes no tiles / depth / aabb planes (nothing of the
// frame reads them; the stage taps rebuild them: launch_records_to_planes).  A cursor ends at the bin's TRUE count whatever its region holds: level 2 reads its
// bin's count there (and b cap as its offset), flags a region that ran over, and adds up E1 and the fullest bin.
constexpr uint32_t kL1FusedStride = 32, kL1FusedCursor0 = kVisRegions, kL1FusedWords = (kVisRegions + 1024) * kL1FusedStride;
struct L1Fused {
    uint32_t* words;  // null: the three level-1 kernels run
    uint32_t* cand;
    uint32_t cap;     // records per bin region
    uint64_t* vis_mask;  // [ceil(n / 64)] bit j % 64 of word j / 64: the j-th Gaussian in the order read is visible (instead of the planes)
    uint32_t tiles_x, tiles_y, bins_x, bins_y;
    int bin_shift, grid_shift;
};

// Device-resident frame counters.
struct Counters {
    uint32_t visible;    // V
    uint32_t instances;  // D (may exceed capacity: then `overflow` is set and nothing past capacity is written)
    uint32_t overflow;   // bit 0: the capacity (candidates or lists) was exceeded; bit 1: a bin outgrew the in-LDS order of its level
    uint32_t bin_entries;  // E1: (bin, Gaussian) candidates of the level-1 binning
    uint32_t max_bin;    // candidates in the fullest bin
    uint32_t slabs;      // depth-slab descriptors written by k_bin_slabs for k_slab_work (level 4)
    // written BY the guarded blend (the host copy, published when the blend starts, does not hold them; gs_get_stats reads the device words):
    uint32_t blend_resolved;  // break decisions (render.comp:83) inside the guard's window, resolved by replaying the pixel exactly
    uint32_t blend_redo;      // quadrants (8 x 8 px) abandoned and re-rendered whole with the reference's arithmetic
    // the work queue of k_bin_queue (level 4 in one launch): items handed out so far (bins first, then depth slabs); bins beyond a slab planned so far
    uint32_t q_head, q_bins_done;
    // tile instances actually LISTED: the cursor the lists are placed by.  Equal to `instances` unless level 2 made the lists from the
    // records' alpha-cut boxes (gs_bin.h: bin_box_pair), then at most that.  0 after a frame of k_bin_build (which has one cursor).
    // (Cleared by k_preprocess and published by the blend with the rest of this block: no kernel of its own touches it.)
    uint32_t listed;
};
// The frame's timeline, stamped by the kernels themselves (round 6).  Every pass's first kernel writes the constant-rate clock
// (wall_clock64: s_memrealtime, hipDeviceAttributeWallClockRate kHz) at its start -- thread 0 of workgroup 0 -- and a one-wave kernel
// behind the blend stamps the frame's end and copies the stamps to pinned host memory.  Round 5 bracketed the passes with hipEvents
// (the reference's vkCmdWriteTimestamp, Renderer.cpp:484-526): each record is a barrier packet the next dispatch waits for, 4.5 us
// of idle GPU apiece, 22 us of a 290-us frame rendered alone (profiles/r06_seams.txt); two kernels with nothing between them start
// back to back.  A span therefore runs from a pass's first kernel's start to the next pass's: the seam belongs to the pass before it.
enum FrameStamp { ST_PREPROCESS = 0, ST_ORDER = 1, ST_L1_COUNT = 2, ST_L1_SCATTER = 3, ST_L2 = 4, ST_BLEND = 5, ST_END = 6, ST_COUNT = 8 };

// What changes from one frame to the next.  Normally these travel as kernel arguments; when a frame is replayed
// as a captured HIP graph (gs_set_graph_mode) they are read from this block in device memory instead, which the
// host refreshes with one small copy ahead of the graph launch -- the graph itself never needs re-recording.
struct FrameParams {
    gs_uniforms u;
    float* rgba;
    uint8_t* bgra;
    Counters* host_counters;
    uint64_t* host_stamps;  // pinned, [ST_COUNT]
};

constexpr int kBinSortMax = 16384;  // the largest in-LDS order (gs_levels.h: kBinSortLimit[3])
constexpr uint32_t kSlabDescBytes = 288, kSlabCapacity = 8192, kSlabWorkGroups = 512, kQueueWorkGroups = 256;

// cov3D of Gaussians [first, first + count) of the blob (6 planes of n floats; the other Gaussians' values stay)
void launch_cov3d(const float* blob, float* cov3d, uint32_t n, uint32_t stride, uint32_t first, uint32_t count, hipStream_t s);
// cut[i] = the most negative power <= 0 with !(min(0.99, opacity[i] * expf(power)) < 1/255)  (render.comp:77-78; +inf: none,
// -inf: all), exact for libm's expf: the blend compares `power` with it instead of alpha with 1/255 (gs_device.h: alpha_cut)
// *beyond_unit (device memory, nullable, zeroed by the caller): set to 1 if any opacity exceeds 1
void launch_alpha_cut(const float* blob, float* cut, uint32_t n, uint32_t stride, uint32_t* beyond_unit, hipStream_t s);
// dst = the blob with its Gaussians in the order perm (dst Gaussian j = src Gaussian perm[j]): 11 planes + the SH block
void launch_permute_blob(const float* src, const uint32_t* perm, float* dst, uint32_t n, uint32_t stride, hipStream_t s);
// *out (device) = sum of the blob's 32-bit patterns, as 64-bit integers (wrapping): what gs_dist_verify compares across ranks
void launch_blob_checksum(const float* blob, uint64_t floats, uint64_t* out, hipStream_t s);
// fp32 SH block of the blob -> binary16 (round to nearest even): the 48 values of each Gaussian in [first, first + count)
void launch_sh_to_half(const float* blob, uint16_t* sh16, uint32_t stride, uint32_t first, uint32_t count, hipStream_t s);
// Gaussians [first, first + count) of the blob from a trainer's device arrays (row i of each array = Gaussian first + i), activated as
// gs::host::activate_record activates a PLY record, bit for bit; a null member leaves what the blob holds (gs3d_hip.h: gs_device_arrays).
// replace_rest: the SH bands above the DC term are written -- from sh_rest, zero beyond sh_rest_coeffs (0: all zero, sh_rest not read)
void launch_ingest_arrays(const gs_device_arrays& a, float* blob, uint32_t stride, uint32_t first, uint32_t count, bool replace_rest,
                          hipStream_t s);
// gs_scene_transform: what k_scene_transform takes from the host (gs_sh_rotation.h: everything computed in binary64 and rounded
// once), all of it wave-uniform.  x -> s R x + t; q = the normalised rotation; M = the SH band matrices M_1, M_2, M_3, row-major.
struct SceneTransform {
    float R[9];  // row-major
    float t[3];
    float s;
    float q[4];  // w x y z
    float M[9 + 25 + 49];
};
// Gaussians [first, first + count) of the blob moved by x, in place: positions, scales, rotations, SH bands 1..3 (gs3d_hip.h)
void launch_scene_transform(const SceneTransform& x, float* blob, uint32_t stride, uint32_t first, uint32_t count, hipStream_t s);
// Gaussians [first, first + count) of the blob as PLY-domain values, the inverse of launch_ingest_arrays (gs3d_hip.h:
// gs_scene_to_device_arrays): into the trainer's arrays (row i = Gaussian first + i; a null member is skipped), or as
// 62-float PLY records (records[i] = Gaussian first + i).  Nothing of the blob changes.
void launch_scene_export(const gs_device_arrays_out& a, const float* blob, uint32_t stride, uint32_t first, uint32_t count, hipStream_t s);
void launch_scene_export_records(float* records, const float* blob, uint32_t stride, uint32_t first, uint32_t count, hipStream_t s);
// counters (nullable): the kernel clears the frame's counters, so that a frame needs no memset node.
// fp (nullable, device memory): read the uniforms / output pointers from it instead of the arguments (graph replay)
// stamps (nullable, device memory, [ST_COUNT]): the frame's timeline, see FrameStamp
// antialiased: the records carry opacity * sqrt(det(cov2D) / det(cov2D + 0.3 I)) and that opacity's alpha cut, taken per
// frame (gs_set_antialiased); sv.acut is not read.  Everything else the kernel writes is the same either way.
void launch_preprocess(const SceneView& sv, const gs_uniforms& u, const AttrView& av, Counters* counters,
                       const FrameParams* fp, uint64_t* stamps, bool antialiased, const L1Fused& lf, hipStream_t s);
// behind the frame's last kernel: stamps[ST_END] = now, the stamps copied to host_stamps (pinned; fp non-null: fp->host_stamps);
// l1_words (nullable): the first l1_counters counters of L1Fused::words are zeroed for the next frame on these buffers
void launch_frame_end(uint64_t* stamps, uint64_t* host_stamps, const FrameParams* fp, uint32_t* l1_words, uint32_t l1_counters, hipStream_t s);

// Stable LSD radix pass on (u32 key, u32 value) pairs, 8-bit digit at `shift` (the global depth order).
//   first != 0: the input is (key = bits(depth[i]), value = i) for every i < n_static with tiles[i] != 0
//               (compaction folded into the first pass); the element count is written to *n_out.
//   first == 0: the element count is read from *n_in (device memory).
// scratch: block histograms, 256 * (blocks + 1) uint32.
struct RadixPass {
    const uint32_t* keys_in;
    const uint32_t* vals_in;
    uint32_t* keys_out;
    uint32_t* vals_out;
    const uint32_t* n_in;     // device count (first == 0)
    uint32_t n_static;        // N (first != 0) or the capacity bound used to size the grid
    const uint32_t* tiles;    // first != 0
    uint32_t* n_out;          // first != 0
    uint32_t* block_hist;     // [256][blocks]
    uint32_t* digit_total;    // [256]
    int shift;
    int bits;                 // significant bits in this digit (<= 8)
    int blocks;
    int first;
    uint64_t* stamps;         // nullable: the pass's first kernel stamps [ST_ORDER] (the caller sets it on the first pass only)
};
void launch_radix_pass(const RadixPass& p, hipStream_t s);

// Two-level binning (gs_bin_l1.hip, gs_bin_l2.hip): level 1 lists the items (Gaussians in index order, or the visible Gaussians in
// depth order when `order` is given) per bin of S x S tiles; level 2 turns each bin's list into the per-tile lists
// (ordering it by (depth bits, id) in LDS first when sort is set), the tile ranges and D.
struct BinLaunch {
    const uint32_t* order;      // null: item p = Gaussian p; else Gaussian order[p]
    const uint32_t* n_items;    // device-resident item count (null: n_bound)
    uint32_t n_bound;           // N: sizes the grid and the hist table
    const uint32_t* tiles;      // [N]
    const ushort4* aabb;        // [N]
    const float* depth;         // [N]
    const uint4* vis;           // null, or (any-order scatter only) AttrView::vis / vis_count / vis_region_slots: the items are the lists' entries
    uint32_t* vis_count;
    uint32_t vis_region_slots;
    uint32_t* hist;             // [padded bins + 1][bin_level1_columns(n_bound)] (the last row: visible items per block)
    uint32_t* bin_count;        // [2048]: per padded bin its candidate count, then (from 1024 on) its offset in the candidate buffer
    uint32_t* cand;             // [cand_capacity] records (3 words each) or ids
    uint32_t* ranges;           // [T][2]
    uint32_t* sorted_gid;       // [capacity (+4)]
    Counters* counters;
    uint32_t capacity;          // tile instances the lists hold
    uint32_t cand_capacity;     // level-1 candidates the candidate buffer holds
    const uint32_t* l1_fused_words;  // non-null: level 1 ran inside k_preprocess (L1Fused) -- a bin's count is its cursor, its offset
    uint32_t l1_fused_cap;           // (on-screen index) x this; level 2 produces V, E1, the fullest bin and the overflow flag
    bool reference_boxes;       // k_bin_fast: make the lists from the records' reference boxes (no alpha-cut cull; gs_bin_l2.hip: BuildArgs)
    void* slabs;                // [slab_capacity] 288-byte depth-slab descriptors (level 4)
    uint32_t slab_capacity;
    uint32_t slab_epoch;        // != 0: level 4 as ONE launch (k_bin_queue); a value no earlier launch on these descriptors carried
                                // (a descriptor is ready when it holds this launch's epoch).  0: k_bin_slabs + k_slab_work
    uint32_t tiles_x, tiles_y, bins_x, bins_y;
    int bin_shift;              // log2 S
    int grid_shift;             // 4 or 5: padded bin id = by << grid_shift | bx
    uint64_t* stamps;           // nullable: the frame's timeline (FrameStamp); level 1 and level 2 stamp their starts
};
// tiles / depth / aabb of the visible Gaussians rebuilt from the dense lists of the frame that just ran (stage taps: k_preprocess
// writes no planes when level 1 streams the lists); av.vis must be the lists of that frame
void launch_vis_to_planes(const AttrView& av, uint32_t n, hipStream_t s);
// the same after a frame of the one-pass level 1 (L1Fused): from its visibility bits and records; perm: SceneView::perm of that frame
void launch_records_to_planes(const uint64_t* vis_mask, const uint32_t* perm, const AttrView& av, uint32_t n, uint32_t width, uint32_t height,
                              hipStream_t s);
uint32_t bin_level1_blocks(uint32_t n_items);
uint32_t bin_level1_columns(uint32_t n_items);  // columns of the hist table: level-1 blocks over the planes or over the dense lists, whichever is more
void bin_debug_occupancy();
hipError_t bin_prepare_device();                                    // once per device, before the first launch_bin_level2
void launch_bin_level1_count(const BinLaunch& b, hipStream_t s);    // k_l1_hist, k_l1_scan
// any_order: the candidates of a bin may land in any order inside each block's run (the bin-local path with bins of
// <= 8 x 8 tiles orders them by (depth, id) anyway); otherwise item order is kept
void launch_bin_level1_scatter(const BinLaunch& b, bool any_order, hipStream_t s);  // k_l1_scatter / k_l1_scatter_any_order
// level 0 .. 4: the bin's candidates are ordered by (depth bits, id) in LDS, up to kBinSortLimit[level] per bin (level 4 in
// several slabs); level 5: no ordering (the candidates arrive in depth order: global path), any bin size
void launch_bin_level2(const BinLaunch& b, int level, hipStream_t s);  // k_bin_build

// render.comp counterpart.
// tile_order[b] = the tile workgroup b renders (a permutation of the tiles)
void launch_blend(const uint32_t* ranges, const uint32_t* sorted_gid, const uint32_t* tile_order, const AttrView& av,
                  uint32_t width,
                  uint32_t height, float* rgba, uint8_t* bgra, Counters* counters,
                  Counters* host_counters /* pinned, nullable: *host_counters = *counters */,
                  int exp_mode /* 0 pipeline polynomial, 1 v_exp_f32, 2 libm's expf restated in binary64, 3 v_exp_f32 under the guard
                                  of render.comp:82 (break decisions near the cut taken from mode 2's arithmetic; needs every
                                  opacity <= 1: the caller passes 2 for a scene that holds a larger one) */,
                  bool contract /* the three FMA contractions GLSL permits in render.comp:66,87, or (default) none */,
                  const FrameParams* fp,
                  bool lockstep /* the four waves of a tile take every chunk of its list together (s_barrier): gs_blend.hip */,
                  uint64_t* stamps /* nullable: [ST_BLEND] = the kernel's start */,
                  hipStream_t s);

// A finished frame's per-tile lists, as the four passes below walk them: the first six arguments of each of their kernels.
struct TileLists {
    const uint32_t* ranges;      // [T][2]
    const uint32_t* sorted_gid;  // the lists, bin-major
    const uint32_t* tile_order;  // tile_order[b] = the tile workgroup b walks
    const AttrRecord* rec;       // [N]
    uint32_t width, height;
};

// gs_accumulate_contributions (gs3d_hip.h; gs_contrib.hip): a second walk of a finished frame's per-tile lists with the reference's
// arithmetic.  Reads ranges / sorted_gid / rec of that frame, writes the caller's arrays only: weight[g] += sum of q, pixels[g] +=
// blended pixels (integer atomics), top_id[pixel] = the dominant id.  mask, weight, pixels, top_id: nullable, device memory.
void launch_contributions(const TileLists& t, const uint8_t* mask, uint64_t* weight, uint32_t* pixels, uint32_t* top_id, hipStream_t s);

// gs_blend_features (gs3d_hip.h; gs_features.hip): the same second walk, per pixel: `channels` caller-supplied per-Gaussian floats
// blended as the colour is (features [N][channels] -> out_features [height][width][channels]), alpha = 1 - T, expected and median
// depth.  Channels go in groups of kFeatureGroup, one launch per group on `s`, each walking the lists again; the first launch (or a
// channel-less one) writes alpha and the depths.  Every output is nullable; with out_features null no channel is blended.
constexpr int kFeatureGroup = 16;
void launch_features(const TileLists& t, const float* features, uint32_t channels, float* out_features, float* out_alpha, float* out_depth,
                     float* out_median, hipStream_t s);

// gs_lift_pixels (gs3d_hip.h; gs_lift.hip): the same second walk, transposed: per counted pixel (inside the image, mask null or
// != 0) `channels` caller-supplied floats (values [height][width][channels]) are carried onto the Gaussians blended there with
// k_contrib's w = fl32(alpha T): out[g][c] += (double)w values[p][c], out_weight[g] += (double)w, binary64 atomic adds.  Channels
// go in groups of kLiftGroup, one launch per group on `s`, each walking the lists again; the first launch (or a channel-less one)
// adds the weights.  mask, out, out_weight: nullable, device memory; with out null no channel is lifted.
constexpr int kLiftGroup = 16, kLiftGroupSmall = 4;  // (a last group of at most 4 channels runs a kernel of 4)
void launch_lift(const TileLists& t, const uint8_t* mask, const float* values, uint32_t channels, double* out, double* out_weight,
                 hipStream_t s);

// gs_blend_backward (gs3d_hip.h; gs_backward.hip): the backward of the blend over the same lists: from grad_rgb [height][width][3]
// and grad_alpha [height][width] (nullable: zeros) the per-Gaussian sums d_colour [N][3], d_opacity [N], d_conic [N][3], d_uv [N][2],
// binary64 atomic adds.  One launch that walks every tile's list twice (the suffix sums R_i), or once when d_colour alone is asked
// for.  Every output is nullable, device memory; with all four null nothing is launched.
void launch_blend_backward(const TileLists& t, const float* grad_rgb, const float* grad_alpha, double* d_colour, double* d_opacity,
                           double* d_conic, double* d_uv, hipStream_t s);

// gs_project_backward (gs3d_hip.h; gs_project_backward.hip): the projection half of the backward, one lane per Gaussian of sv in the
// order the frame read it: from g's four input arrays (nullable: zeros) the sums of g's six output arrays (nullable: skipped), by
// scene id, for the Gaussians with tiles[id] != 0.  tiles, rec: the frame's tiles_overlap plane and records, by scene id; u,
// antialiased: what the frame ran with.  One writer per element, no atomics.
void launch_project_backward(const SceneView& sv, const uint32_t* tiles, const AttrRecord* rec, const gs_uniforms& u, bool antialiased,
                             const gs_project_grads& g, hipStream_t s);

// gs_camera_backward (gs3d_hip.h; gs_camera_backward.hip): the camera half of the backward over the same inputs: the 27 sums over
// the Gaussians with tiles[id] != 0 are ADDED to g's three output arrays (nullable: skipped).  Two launches: at most
// GS_CAMERA_BACKWARD_LANES lanes striding over sv, one row of 27 partials per workgroup into `partials` (the renderer's, at least
// camera_backward_partials() doubles), then one wave that adds the rows in index order.  No atomics: the same bits every call.
size_t camera_backward_partials();
void launch_camera_backward(const SceneView& sv, const uint32_t* tiles, const AttrRecord* rec, const gs_uniforms& u, bool antialiased,
                            const gs_camera_grads& g, double* partials, hipStream_t s);

// gs_photometric_loss (gs3d_hip.h; gs_loss.hip): l's terms and grad_rgb (at least one not null; l checked by the caller) of l's two
// images.  lambda > 0: k_loss_ssim over tiles of 16 x 16 pixels, one row of three partial sums per workgroup into `partials` (the
// renderer's, at least photo_loss_partials() doubles) and, where grad_rgb is asked for, the three P maps into `maps` (the renderer's,
// at least photo_loss_maps() doubles; not touched otherwise) for k_loss_grad to convolve.  lambda == 0: k_loss_l1 alone.  terms:
// k_loss_finish, one workgroup that adds the rows in a fixed order.  No atomics: the same bits every call.
size_t photo_loss_partials(int width, int height);
size_t photo_loss_maps(int width, int height);
void launch_photo_loss(const gs_photo_loss& l, double* maps, double* partials, hipStream_t s);

// gs_scene_adam_step (gs3d_hip.h; gs_optim.hip): one Adam step of the Gaussians of a mask, in the caller's tensors and in the blob.
// A group is a gs_adam_group with its step size lr / bias_correction1 formed by the caller; all four pointers null: not stepped.
struct AdamGroup {
    float* param;
    double* grad;
    float* exp_avg;
    float* exp_avg_sq;
    double step;  // lr / bias_correction1
};
struct AdamStep {
    AdamGroup means, log_scales, quats, opacity_logits, sh_dc, sh_rest;
    uint32_t sh_rest_coeffs;  // 3, 8 or 15 where sh_rest is stepped
    const uint8_t* mask;      // [n] by scene id, nullable: every Gaussian
    double beta1, beta2, one_minus_beta1, one_minus_beta2, sqrt_bc2, eps;
    bool zero_grads;
};
// One launch over the n Gaussians of `blob` (the scene's own, in scene order: not the copy in spatial order), a workgroup per 256 of
// them; what is derived from the planes it writes is the caller's to redo.
void launch_adam_step(const AdamStep& a, float* blob, uint32_t stride, uint32_t n, hipStream_t s);
// gs_visible_mask: mask[id] = tiles[id] != 0, or that ORed into mask[id]; tiles: the frame's tiles_overlap plane, by scene id.
void launch_visible_mask(const uint32_t* tiles, uint8_t* mask, uint32_t n, bool accumulate, hipStream_t s);

// Adaptive density control (gs3d_hip.h; gs_densify.hip).
// gs_accumulate_densify_stats: the three statistics of the Gaussians with tiles[id] != 0, by scene id; rec: the frame's records
// (the radius), width, height: the frame's.  One lane per Gaussian, no atomics.
void launch_densify_stats(const uint32_t* tiles, const AttrRecord* rec, const gs_densify_stats& st, uint32_t n, uint32_t width,
                          uint32_t height, hipStream_t s);
// gs_densify_plan: the two offset arrays into in.scratch ([0, n] and [n + 1, 2 n + 1]).  parts: 2 * densify_partitions(n) words of
// the caller's for the partitions' sums.  Three launches on `s`; nothing is synchronised here.
size_t densify_partitions(uint32_t n);
void launch_densify_plan(const gs_densify_input& in, uint32_t n, uint32_t* parts, hipStream_t s);
// gs_densify_apply: the output arrays from the inputs and the offsets the plan left in in.scratch; a workgroup per
// GS_DENSIFY_BLOCK parents.  The caller has checked that the offsets end in out.n_out and out.n_noise.
void launch_densify_apply(const gs_densify_input& in, uint32_t n, const gs_densify_output& out, hipStream_t s);

// gs_knn_dist2 (gs3d_hip.h; gs_knn.hip, gs_knn_rules.h): the caller's scratch, cut up.  Every segment starts on 16 bytes of the
// scratch's first 16-byte boundary (knn_scratch_bytes counts the slack for a scratch that is only 4-byte aligned).
struct KnnBuffers {
    float4* sorted;          // [n]  the points in Morton order: x, y, z, bits of the id
    float4* boxes;           // [2 boxes]  lo.xyz, hi.xyz of every GS_KNN_BOX consecutive sorted points
    uint32_t* keys[2];       // [n] each: the radix passes' ping-pong (codes)
    uint32_t* vals[2];       // [n] each: (ids); the order ends in vals[0]
    uint32_t* block_hist;    // [256][radix blocks]
    uint32_t* digit_total;   // [256]
    float* bbox_parts;       // [kKnnBoundParts][8]  stage one of the bounding box
    float* bbox;             // [8]  lo.xyz, 0, hi.xyz, 0
    uint32_t* count;         // [1]  n, where the radix passes read it
};
constexpr uint32_t kKnnBoundParts = 1024;
inline uint32_t knn_boxes(uint32_t n) { return (uint32_t)(((uint64_t)n + GS_KNN_BOX - 1) / GS_KNN_BOX); }
size_t knn_scratch_bytes(uint64_t n);
KnnBuffers knn_buffers(void* scratch, uint32_t n);
// Seventeen launches on `s` (bounding box x 2, codes, four radix passes of three kernels, gather + boxes, search); nothing is
// synchronised here.
// 1 <= k <= GS_KNN_MAX_K, n != 0; mean, dist2, visits: nullable.
void launch_knn(const float* points, uint32_t n, int k, float* mean, float* dist2, uint32_t* visits, const KnnBuffers& b, hipStream_t s);

}  // namespace gs
