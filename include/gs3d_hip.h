/*
 * gs3d_hip.h -- C ABI of libgs3d_hip.so, the MI355X (gfx950) splat rasterizer.
 *
 * This is the drop-in boundary for the per-frame hot path of shg8/3DGS.cpp
 * (preprocess -> scan -> duplicate -> sort -> tile ranges -> alpha blend).
 * Plain pointers and sizes only; no C++/torch types.  Each entry point names
 * the reference interface it replaces (paths relative to /root/reference).
 * The reference-API C++ mirror (VulkanSplatting / Renderer / GSScene) in
 * include/3dgs/ and 3dgs.cpp_amd/csrc/host/ is a thin layer over these calls.
 *
 * All functions return 0 on success and a negative gs_status on failure;
 * gs_last_error() returns the message for the calling thread (the reference
 * throws std::runtime_error with the same text, e.g. GSScene.h:29).
 * Handles are not thread-safe.  By default a renderer has one HIP stream and one
 * frame in flight (VulkanContext.h:6 FRAMES_IN_FLIGHT 1); gs_set_frames_in_flight(k)
 * gives it k buffer sets on k streams.
 */
#ifndef GS3D_HIP_H
#define GS3D_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gs_scene gs_scene;       /* replaces class GSScene,  src/GSScene.h:23-65   */
typedef struct gs_renderer gs_renderer; /* replaces class Renderer, src/Renderer.h:19-168 */

enum gs_status {
    GS_OK = 0,
    GS_ERR_INVALID = -1,   /* bad argument */
    GS_ERR_IO = -2,        /* file missing / malformed PLY (GSScene.h:29, GSScene.cpp:101,147) */
    GS_ERR_DEVICE = -3,    /* HIP error, or no gfx950 device: there is NO CPU fallback */
    GS_ERR_NOMEM = -4,
    GS_ERR_OVERFLOW = -5   /* instance buffers could not be grown (Renderer.cpp:541-563) */
};

/* Renderer::Camera, src/Renderer.h:40-50 (defaults :79-85). */
typedef struct {
    float position[3];
    float rotation[4]; /* quaternion w, x, y, z */
    float fov;         /* degrees, horizontal */
    float near_plane;
    float far_plane;
} gs_camera;

/* Renderer::UniformBuffer, src/Renderer.h:21-29; std140, 160 bytes, column-major. */
typedef struct {
    float camera_position[4];
    float proj_mat[16];
    float view_mat[16];
    uint32_t width;
    uint32_t height;
    float tan_fovx;
    float tan_fovy;
} gs_uniforms;

/* Timestamps of Renderer::retrieveTimestamps (Renderer.cpp:85-100): the six span
 * names registered at Renderer.cpp:484-526,580-699, plus the "instances" metric
 * (Renderer.cpp:540). */
typedef struct {
    uint64_t num_gaussians; /* N */
    uint64_t num_visible;   /* V = #Gaussians with tiles_overlap != 0 */
    uint64_t num_instances; /* D = "instances" */
    uint64_t instance_capacity;
    float ms_preprocess;
    float ms_prefix_sum;
    float ms_preprocess_sort;
    float ms_sort;
    float ms_tile_boundary;
    float ms_render;
    float ms_total;
    uint32_t retries; /* frames re-run after growing the instance buffers */
    uint32_t num_bin_entries; /* E1: (bin, Gaussian) candidates of the tile binning's first level */
    uint32_t max_bin_entries; /* candidates in the fullest bin */
    uint32_t sort_path;       /* depth-order path the frame took: 1 = global, 2 = bin-local (gs_set_sort_path) */
    uint32_t bin_tiles;       /* edge of the frame's bins in tiles (4, 8, 16 or 32) */
    uint32_t sort_level;      /* 0 .. 3: in-LDS order of up to 4096 / 8192 / 12288 / 16384 candidates per bin; 4: up to 65535 in depth slabs; 5: global path */
    uint32_t blend_redo;      /* gs_get_stats only, exp mode 3: quadrants (8 x 8 px) of the last frame abandoned by the fast pass and re-rendered with mode 2's arithmetic */
    uint32_t blend_resolved;  /* gs_get_stats only, exp mode 3: break decisions (render.comp:83) that fell inside the guard's window and were resolved by an exact replay of that pixel */
    uint32_t pad_;
} gs_frame_stats;

/* Stage taps for parity tests (the role of Buffer::download / assertEquals,
 * src/vulkan/Buffer.cpp:176-226).  Layouts are documented in DESIGN.md. */
enum gs_stage {
    GS_STAGE_TILES = 0,          /* uint32[N]  tiles_overlap                                  */
    GS_STAGE_DEPTH = 1,          /* float[N]   view-space depth (valid where tiles != 0)      */
    GS_STAGE_RADIUS = 2,         /* float[N]                                                  */
    GS_STAGE_AABB = 3,           /* uint16[4N] x0 y0 x1 y1                                    */
    GS_STAGE_CONIC_OPACITY = 4,  /* float[4N]                                                 */
    GS_STAGE_UV_RG = 5,          /* float[4N]  u v r g                                        */
    GS_STAGE_B = 6,              /* float[N]   b                                              */
    GS_STAGE_DEPTH_ORDER = 7,    /* uint32[V]  visible Gaussian ids, ascending (depth, id)    */
    GS_STAGE_ALPHA_CUT = 8,      /* float[N]   the most negative `power` at which render.comp:78 keeps an entry of this Gaussian
                                               (from its opacity, exact for libm's expf; +inf: never kept, -inf: always)  */
    GS_STAGE_SORTED_TILE = 11,   /* uint32[D]  == sorted key >> 32 of the reference (expanded from the ranges) */
    GS_STAGE_SORTED_GID = 12,    /* uint32[D]  == sorted payload of the reference             */
    GS_STAGE_RANGES = 13,        /* uint32[2T] == tileBoundaryBuffer                          */
    GS_STAGE_LISTS_RAW = 14,     /* uint32[D]  the per-tile lists exactly as they lie in HBM (bin-major)            */
    GS_STAGE_RANGES_RAW = 15,    /* uint32[2T] each tile's (start, end) in GS_STAGE_LISTS_RAW; (0, 0) when empty    */
    /* the lists as the blend walked them (gs_set_tile_cull): tile order, like 12 / 13; equal to those unless the frame is culled */
    GS_STAGE_LISTS_CULLED = 16,  /* uint32[L]  L = gs_get_listed_instances                     */
    GS_STAGE_RANGES_CULLED = 17  /* uint32[2T] each tile's (start, end) in GS_STAGE_LISTS_CULLED; (0, 0) when empty */
};

const char* gs_last_error(void);
int gs_device_count(int* count);

/* ---- scene: GSScene ------------------------------------------------------- */

/* GSScene::GSScene(filename) + GSScene::load (GSScene.h:25-31, GSScene.cpp:26-68):
 * parse the binary PLY, apply exp/sigmoid/normalize + SH reorder, upload as SoA,
 * run the cov3D precompute (GSScene.cpp:157-184). */
int gs_scene_load_ply(const char* path, int device, gs_scene** out);

/* Host-only halves of GSScene::load, usable without a GPU:
 *   gs_read_ply: loadPlyHeader + payload read (GSScene.cpp:99-149, :36-41); records may be NULL to
 *                query *n_out first; capacity in records.
 *   gs_activate_records: the per-record conversion (GSScene.cpp:42-55): exp(scale), sigmoid(opacity),
 *                normalize(rot), planar->interleaved SH; n x 62 floats -> n x 60 floats (GSScene::Vertex). */
int gs_read_ply(const char* path, float* records, uint64_t capacity, uint64_t* n_out);
int gs_activate_records(const float* records, uint64_t n, float* vertices);

/* Same, from n PLY-domain records (62 floats each, GSScene.cpp:17-24) in host memory. */
int gs_scene_from_records(const float* records, uint64_t n, int device, gs_scene** out);

/* From n activated GSScene::Vertex structs (60 floats each, GSScene.h:41-46) in host
 * memory: what vertexBuffer->uploadFrom(staging) transfers (GSScene.cpp:61). */
int gs_scene_from_vertices(const float* vertices, uint64_t n, int device, gs_scene** out);

/* Adopt a packed SoA blob already resident in HBM (gs_scene_blob_floats(n) floats:
 * 11 SoA planes pos[3] scale[3] rot[4] opacity[1], each padded to st = n rounded up to 16 floats, then the SH
 * block as AoS sh[n][48]; d_blob must be 64-byte aligned, which makes every plane and every Gaussian's 192-byte
 * SH block start on a 64-byte line); the caller keeps it alive.
 * This is the multi-GPU path: rank 0 builds the blob, RCCL broadcasts it, every rank
 * adopts its copy.  No reference counterpart (the reference is single-GPU). */
int gs_scene_from_device_blob(float* d_blob, uint64_t n, int device, gs_scene** out);
uint64_t gs_scene_blob_floats(uint64_t n);
int gs_scene_blob(const gs_scene* s, float** d_blob, uint64_t* floats);

/* A trainer's model as it lies in HBM: six dense fp32 arrays of n rows each, the layout of the Inria trainer's parameters
 * (_xyz, _scaling, _rotation, _opacity, _features_dc (N,1,3), _features_rest (N,15,3)) and of gsplat's (means, scales, quats,
 * opacities, sh0, shN).  Device pointers on the scene's device, 4-byte aligned and nothing more (a slice of a larger tensor
 * is a legal argument).  The values are PLY-domain, i.e. not yet activated. */
typedef struct {
    const float* means;           /* [n][3]                                   */
    const float* log_scales;      /* [n][3]   exp() is applied here           */
    const float* quats;           /* [n][4]   w x y z, raw; normalised here   */
    const float* opacity_logits;  /* [n]      sigmoid is applied here         */
    const float* sh_dc;           /* [n][3]                                   */
    const float* sh_rest;         /* [n][sh_rest_coeffs][3], RGB innermost    */
    uint32_t     sh_rest_coeffs;  /* 0, 3, 8 or 15 (SH degree 0..3)           */
} gs_device_arrays;

/* GSScene::load's conversion loop and upload (GSScene.cpp:36-61) with the data ALREADY ON THE DEVICE: one kernel applies
 * exp / sigmoid / normalize and lays the six arrays out as the scene's blob, device to device, then the load-time passes of
 * every other way in run unchanged (cov3D, the alpha cuts, for large scenes the copy in spatial order).  No host copy of the
 * model, no PCIe transfer.  The scene is BIT FOR BIT the one gs_scene_from_records builds from the same numbers (exp is
 * libm's expf restated, division and square root are IEEE; a NaN stays a NaN, its sign and payload are the device's).
 * SH bands beyond sh_rest_coeffs are zero; sh_rest may be NULL only with sh_rest_coeffs == 0; every other member is required.
 * stream: a hipStream_t (NULL: the default stream).  The ingest is enqueued on it, behind whatever the caller has enqueued
 * there (the trainer's optimiser step); the call returns after synchronising it.  The arrays are not referenced afterwards.
 * GS_ERR_INVALID: a null argument, n >= 2^31, sh_rest_coeffs not in {0, 3, 8, 15}, a misaligned pointer. */
int gs_scene_from_device_arrays(const gs_device_arrays* a, uint64_t n, int device, void* stream, gs_scene** out);
/* Overwrite Gaussians [first, first + count) of a scene of ANY origin from such arrays (row i = Gaussian first + i), in
 * place: the live view of a training run.  The Gaussian count is fixed (a densification changes it: gs_densify_plan and
 * gs_densify_apply, below, make the new arrays on the device).  A NULL member means "keep what the scene holds"; sh_rest == NULL keeps the higher bands whatever
 * sh_rest_coeffs says, a non-NULL sh_rest replaces all of them (zero beyond sh_rest_coeffs).  count == 0 or no member at
 * all: a successful no-op.  Everything derived from what changed is redone on `stream` before the call returns (it
 * synchronises the stream): cov3D, the alpha cuts and the opacity flag behind exp mode 3, the binary16 SH block of a
 * quantised scene, the copy in spatial order.  The ORDER of that copy is not recomputed: it is the order of the positions
 * the scene was built with, a matter of speed only (frames are identical in any order); a model that has moved far is
 * better served by a new scene.  No device pointer a renderer holds changes, so the scene's renderers -- captured graphs
 * included -- go on working.  The frames they have in flight read the scene while they run: call gs_synchronize on EVERY
 * renderer of the scene first; a frame that straddles the update reads a mixture of both states. */
int gs_scene_update_from_device_arrays(gs_scene* s, const gs_device_arrays* a, uint64_t first, uint64_t count, void* stream);

/* A similarity of the world: x -> scale * R(rotation) x + translation.  No reference counterpart (GSScene only loads). */
typedef struct {
    float rotation[4];     /* quaternion w x y z, the convention of gs_camera.rotation; normalised here (binary64) */
    float translation[3];
    float scale;           /* uniform, finite, > 0 */
} gs_transform;
/* Move Gaussians [first, first + count) of a scene of ANY origin by t, in place and on the device: put a trained scene the
 * right way up and at the right size, align two captures, let a rigid part of a scene follow an object from frame to frame.
 * For every Gaussian of the range, with q_R the normalised rotation and R its matrix:
 *     position' = scale * R position + translation          scales' = scale * scales (the activated ones)
 *     rotation' = normalize(q_R (x) rotation)               (Hamilton product, q_R on the left; renormalised on every call, so
 *                                                            that repeated transforms do not let the norm drift)
 *     SH band l = 1, 2, 3 of each colour channel: c'_l = M_l(R) c_l, where M_l is defined by f'(d) = f(R^T d) for every unit d
 *     and f is the colour function preprocess evaluates (its basis, signs and coefficient order; sh[3 j + channel]) -- a
 *     rotated splat whose SH are left alone shows its colours from the wrong side.
 * Opacity and the SH DC term keep their bits; so does everything outside the range, the planes' padding included.  binary32,
 * one rounding per operation in the order k_scene_transform (gs_scene.hip) documents; R and M_l are computed in binary64 and
 * rounded once.  What is derived is redone on `stream` (a hipStream_t, NULL: the default stream; the call is enqueued behind
 * what the caller has enqueued there and returns after synchronising it): cov3D; the binary16 SH block of a quantised scene;
 * the copy in spatial order if the scene has one (whole planes then; its ORDER is not recomputed, as in
 * gs_scene_update_from_device_arrays).  Without that copy every pass covers the range only, so a small range is cheap.  The
 * alpha cuts stay: opacity does not change.  No device pointer a renderer holds changes: renderers and their captured graphs go
 * on working.  Frames in flight read the scene while they run: call gs_synchronize on EVERY renderer of the scene first.
 * count == 0: a successful no-op.  The identity is not special-cased (rotations renormalise).
 * GS_ERR_INVALID, before a device is selected: a null argument; a scale that is not finite or <= 0; a non-finite translation;
 * a quaternion that is non-finite or of zero norm; a range out of bounds.
 * Non-uniform scales and reflections are not similarities of a splat model (neither SH nor the quaternion form carry them). */
int gs_scene_transform(gs_scene* s, const gs_transform* t, uint64_t first, uint64_t count, void* stream);
/* Host only, no device: the three band matrices that rotate SH coefficients with R(t->rotation) -- M_1 3 x 3, M_2 5 x 5, M_3 7 x 7,
 * row-major, back to back: 83 floats (binary64, rounded once).  c'[i] = sum_j M_l[i][j] c[j] over the band's coefficients of
 * one channel, in the scene's coefficient order.  Translation and scale do not enter (they are validated all the same). */
int gs_transform_sh_matrices(const gs_transform* t, float out[83]);
/* Host only: the camera that sees the transformed scene exactly as `in` saw the original -- position scale * R p + translation,
 * rotation q_R (x) q_cam, near and far planes times scale, fov kept.  Depths of that view are scale times the original's.
 * in->rotation is used as it is, NOT normalised (gs_camera_uniforms does not normalise it either): the product has its norm. */
int gs_transform_camera(const gs_transform* t, const gs_camera* in, gs_camera* out);

/* ---- export: the scene back out, as PLY-domain values.  No reference counterpart (GSScene only loads). -------------------
 * The inverse of the activation.  Positions, the rotation AS STORED and the 48 SH coefficients are copies of bits (the
 * record's planar f_rest is the exact inverse of gs_activate_records' reorder; normals are 0).  A scale s and an opacity o are
 * exported as the binary32 pre-activation value whose activation -- exp, 1 / (1 + exp(-x)), evaluated as every way into a
 * scene evaluates them -- is closest to the stored value: a first guess log(s), log(o / (1 - o)) computed in binary64 and
 * rounded once, then the best of that value and its binary32 neighbours at distance <= 4 (ties: the order 0, -1, +1, -2, ..).
 * The rule is stated operation by operation in gs_host_math.h and gs_scene.hip; host and device give the same bits.
 *   - A stored value that IS an image of the activation (every scene that was loaded and not transformed) re-activates to
 *     exactly the stored bits: a scene that is saved and reloaded has the same positions, scales, opacities and SH, bit for
 *     bit.  Measured over 6e7 scales exp(x), x in [-103, 88], and 5.8e7 opacities sigmoid(x), x in [-100, 17]: every one; the
 *     scales never needed a neighbour, the opacities one at distance <= 2.
 *   - A stored value that is not an image (a transformed scale, a subnormal) gets the nearest image: the rule, not an error.
 *   - s == 0 -> -inf, s == +inf -> +inf, s < 0 or NaN -> NaN;  o == 0 -> -inf, o == 1 -> +inf, o outside [0, 1] or NaN -> NaN.
 *   - ROTATIONS round-trip to within a bound, NOT bit for bit: the stored quaternion is normalised and a reload normalises
 *     it again; its dot product is 1 +- a few 2^-24, so each component may move by up to 8 * 2^-24 relative (measured
 *     <= 4.8 * 2^-24, on 36 % of rows) -- and with it cov3D and the frame, by rounding noise.
 * gs_deactivate_vertices: host only, no device: the inverse of gs_activate_records; n x 60 floats -> n x 62 floats.
 * gs_write_ply: host only: n records as the reference's binary PLY (little endian, the 62 float properties x y z nx ny nz
 *   f_dc_0..2 f_rest_0..44 opacity scale_0..2 rot_0..3), which gs_read_ply takes as the records they are and the reference
 *   loads.  An I/O error removes the partly written file: GS_ERR_IO. */
int gs_deactivate_vertices(const float* vertices, uint64_t n, float* records);
int gs_write_ply(const char* path, const float* records, uint64_t n);
/* Where gs_scene_to_device_arrays puts the model: gs_device_arrays with writable members (device pointers on the scene's
 * device, 4-byte aligned and nothing more; n rows each). */
typedef struct {
    float* means;           /* [n][3]                                          */
    float* log_scales;      /* [n][3]   log of the stored scale (see above)    */
    float* quats;           /* [n][4]   w x y z, as stored (normalised)        */
    float* opacity_logits;  /* [n]      logit of the stored opacity            */
    float* sh_dc;           /* [n][3]                                          */
    float* sh_rest;         /* [n][sh_rest_coeffs][3], RGB innermost           */
    uint32_t sh_rest_coeffs; /* 0, 3, 8 or 15: higher bands are dropped        */
} gs_device_arrays_out;
/* Gaussians [first, first + count) of a scene of ANY origin as the six arrays gs_scene_from_device_arrays accepts, device
 * to device (row i = Gaussian first + i): masking, concatenating, pruning and re-ordering scenes is then tensor work on
 * the device, and a trainer can start from a PLY loaded and aligned here.  A NULL member is skipped (sh_rest == NULL: the
 * caller does not want the higher bands, whatever sh_rest_coeffs says); count == 0 is a successful no-op.  It reads the
 * scene's canonical blob -- id order, never the copy in spatial order -- and the fp32 SH block even when the scene is
 * quantised (gs_scene_quantize_sh keeps that block; the binary16 one is not exported).  Nothing in the scene changes.  The
 * work is enqueued on `stream` (a hipStream_t, NULL: the default stream) and the call returns after synchronising it.
 * GS_ERR_INVALID, before a device is selected: a null argument, a range out of bounds, sh_rest_coeffs not in {0, 3, 8, 15},
 * a misaligned pointer. */
int gs_scene_to_device_arrays(const gs_scene* s, const gs_device_arrays_out* a, uint64_t first, uint64_t count, void* stream);
/* Gaussians [first, first + count) as PLY records (62 floats each) in host memory: the PLY-domain twin of
 * gs_scene_download_vertex_range, equal to gs_deactivate_vertices of it bit for bit. */
int gs_scene_download_records(const gs_scene* s, uint64_t first, uint64_t count, float* records);
/* The whole scene as a PLY, byte for byte what gs_write_ply writes from gs_scene_download_records: streamed in chunks (the
 * kernel fills one of two device buffers with records, an asynchronous copy moves them to pinned host memory, the file is
 * written from there while the next chunk is produced; 64-bit offsets), so no host copy of the scene is made.  An I/O error
 * removes the partly written file: GS_ERR_IO. */
int gs_scene_save_ply(const gs_scene* s, const char* path);

/* GSScene::getNumVertices (GSScene.h:37-39). */
uint64_t gs_scene_num_vertices(const gs_scene* s);
/* Opt-in storage quantisation (no reference counterpart; the reference keeps fp32 SH, GSScene.h:41-46): the 48 SH
 * coefficients of every Gaussian are rounded to binary16 (nearest even) once, and preprocess reads 96 B instead of
 * 192 B per visible Gaussian.  It CHANGES the scene: the result equals the reference pipeline run on the rounded
 * coefficients (what the parity tests feed the oracle), not on the original ones.  gs_scene_sh_bits: 32 or 16.
 * The switch is read when a frame is enqueued: frames already in flight on the scene's renderers finish on the fp32 block
 * (which stays allocated), later ones read the binary16 block -- call gs_synchronize first if no frame may straddle it.
 * gs_dist_broadcast_scene replicates the setting. */
int gs_scene_quantize_sh(gs_scene* s);
int gs_scene_sh_bits(const gs_scene* s);
/* Vertices [first, first + count) as GSScene::Vertex (60 floats each): spot checks of scenes too large to read back whole. */
int gs_scene_download_vertex_range(const gs_scene* s, uint64_t first, uint64_t count, float* vertices);
/* Read back the activated vertices as GSScene::Vertex[n] / cov3DBuffer as float[6n]. */
int gs_scene_download_vertices(const gs_scene* s, float* vertices);
int gs_scene_download_cov3d(const gs_scene* s, float* cov3d);
void gs_scene_destroy(gs_scene* s);

/* ---- renderer: Renderer --------------------------------------------------- */

/* Renderer::initialize (Renderer.cpp:19-31) minus Vulkan/swapchain/GUI: stream,
 * per-frame buffers, the completion events.  The scene must outlive the renderer. */
int gs_renderer_create(gs_scene* scene, gs_renderer** out);
void gs_renderer_destroy(gs_renderer* r);

/* Renderer::updateUniforms (Renderer.cpp:719-754), host arithmetic only. */
int gs_camera_uniforms(const gs_camera* cam, uint32_t width, uint32_t height, gs_uniforms* out);

/* Renderer::draw (Renderer.cpp:366-426): enqueue one frame on the renderer's stream.
 * d_rgba: width*height*4 floats in HBM (RGB + alpha 1, render.comp:98) or NULL;
 * d_bgra: width*height*4 bytes B8G8R8A8_UNORM (Swapchain.cpp:22-28) or NULL.
 * Asynchronous: returns after enqueueing; gs_synchronize() or gs_get_stats() waits.
 * The instance count stays on the device (no mid-frame readback, cf. Renderer.cpp:391-399);
 * an overflow of the instance buffers is detected at the next gs_synchronize/gs_get_stats,
 * which grows them and re-runs the frame (Renderer.cpp:541-563).
 *
 * "The last frame" -- what the stage taps, gs_accumulate_contributions, gs_blend_features, gs_lift_pixels, gs_blend_backward, gs_project_backward and gs_camera_backward answer from -- is the
 * most recently enqueued frame, once it has retired.  What an error of gs_render / gs_render_host leaves of it:
 *   * A REFUSED call changes nothing.  Refused (GS_ERR_INVALID, before any queued frame is waited for and before anything is
 *     allocated): a null argument, an empty framebuffer, a tile box beyond 16 bits, a resolution beyond the tile binning.  The
 *     last frame is still the last frame: every tap and every pass gives what it gave before the call, queued frames stay
 *     queued, and the next frame -- one replayed from a captured graph too -- is what it would have been without the call.
 *   * A call that FAILS WHILE RETIRING queued frames -- GS_ERR_OVERFLOW: a bin too full or depths too crowded for the forced
 *     bin-local path (gs_set_sort_path(r, 2)), instance buffers that overflowed repeatedly, more than 2^30 tile instances or
 *     level-1 candidates -- leaves the renderer WITHOUT a last frame.  Every queued frame was dropped: none of their targets is
 *     valid, and the frame of the failing call, if any, was not enqueued.  The taps and the four passes return GS_ERR_INVALID
 *     ("no frame rendered yet") until a frame rendered after the failure has retired; gs_get_stats keeps describing the last
 *     frame that did retire (blend_redo / blend_resolved, which are read from the device, are 0 meanwhile).  The renderer
 *     renders on: after gs_set_sort_path(r, 0) the same pose gives the right frame.  The same holds for gs_synchronize,
 *     gs_get_stats and every other call that waits for queued frames and returns such an error.
 *   * A device or allocation error (GS_ERR_DEVICE, GS_ERR_NOMEM) while the frame is being issued also leaves the renderer
 *     without a last frame. */
int gs_render(gs_renderer* r, const gs_uniforms* u, float* d_rgba, uint8_t* d_bgra);

/* Convenience: gs_render into host buffers, synchronous. */
int gs_render_host(gs_renderer* r, const gs_uniforms* u, float* h_rgba, uint8_t* h_bgra);

int gs_synchronize(gs_renderer* r);
/* Enable/disable the six per-pass spans of gs_frame_stats (off: the total only).  The reference writes timestamps around every
 * pass (Renderer.cpp:484-526, 580-699; QueryManager.cpp:22-41); here the kernels stamp the device's constant-rate clock at
 * their start themselves, so the spans cost nothing (round 5 recorded a hipEvent per pass: 4.5 us of idle GPU each).  A
 * span runs from the start of a pass's first kernel to the start of the next pass's. */
int gs_set_timing(gs_renderer* r, int enabled);
/* Frames that may be queued on the stream before gs_render blocks (1..8, default 1 like
 * FRAMES_IN_FLIGHT, VulkanContext.h:6).  With k > 1 the renderer keeps k sets of per-frame buffers
 * on k streams: the host enqueues frame i+1 while frame i runs, and the two frames' passes overlap
 * on the GPU.  Frames that may be in flight together must be given distinct output buffers.  An
 * overflowed frame and everything queued behind it are re-run after growing. */
int gs_set_frames_in_flight(gs_renderer* r, int frames);
/* How the per-tile lists get their depth order (same lists either way; no reference counterpart -- the reference
 * sorts all D instances, sort/hist.comp + sort/sort.comp):
 *   1  global:    the V visible Gaussians are ordered by depth first (12 small kernels), then binned;
 *   2  bin-local: Gaussians are binned in index order (bins of S x S tiles, up to 32 x 32 of them) and the workgroup
 *                 that builds a bin's tile lists first orders its candidates in LDS (6 kernels per frame);
 *                 a bin with more than 16384 candidates does not fit -> GS_ERR_OVERFLOW at the next synchronisation;
 *   0  automatic (default): bin-local, with a transparent re-run on the global path when a bin does not fit (and back
 *                 once the bins have fitted again for 32 frames).
 * The GS_STAGE_DEPTH_ORDER tap exists on path 1 only. */
int gs_set_sort_path(gs_renderer* r, int mode);
/* The blend's arithmetic (render.comp:61-98).  The reference for every mode is the shader's text read literally and
 * evaluated the way its CPU compilation (the checker the tests pin this library to) evaluates it: every product
 * and sum of :66 and :87 rounded on its own, exp() of :77 = glibc's expf (x86-64 FMA build, glibc >= 2.27).
 *
 * In EVERY mode render.comp:78's cut `alpha < 1/255` is decided exactly as the reference decides it: on `power`, against the
 * Gaussian's alpha cut (GS_STAGE_ALPHA_CUT: computed at load from the opacity with libm's expf; expf is monotone, so
 * power >= cut <=> alpha >= 1/255 bit for bit).
 *
 * gs_set_exp_mode -- exp() of render.comp:77, which GLSL leaves to the implementation (3 + 2|x| ULP):
 *   3  (default) the hardware's v_exp_f32 UNDER A GUARD: render.comp:82's break `T (1 - alpha) < 1e-4` is the one decision a
 *      fast exp can still flip (T drifts by a few ULP per blended entry).  A pixel whose T (1 - alpha) comes within a proven
 *      window of 1e-4 (gs_blend.hip: kGuard*; a few 1e-5 relative) gets the reference's decision COMPUTED: that one pixel's
 *      list is replayed with mode 2's arithmetic (about one pixel in 1300 at config B; gs_frame_stats::blend_resolved counts
 *      them).  A quadrant that would need more than eight such replays is re-rendered whole with mode 2's arithmetic
 *      (blend_redo), and a scene that holds an opacity > 1 (outside the sigmoid's range, where the bound does not apply) is
 *      blended in mode 2 altogether.  Everything else has taken exactly the reference's decisions: the frame is within
 *      ROUNDING NOISE of the reference text on any scene (<= 1e-5 asserted by the GPU tests on every configuration, measured
 *      <= 4.2e-7), with no threshold-flip pixels -- BASELINE.json's bar is 1e-4 -- at nearly the unguarded loop's speed.
 *      Not reproducible bit for bit on a CPU (v_exp_f32 is not).
 *   2  glibc's expf algorithm restated in binary64 (x 32/ln2 = k + r, 2^(k/32) from a 32-entry table, a cubic, one rounding
 *      to binary32): bit-equal to that libm on every binary32 <= 0 (checked exhaustively on the device and on the host).
 *      The frame is BIT-IDENTICAL to render.comp compiled for a CPU (tests/test_gpu_blend_modes.py, test_gpu_full_size.py);
 *      ~17 % fewer frames/s than mode 3 at config B.  Domain note: valid for opacity <= 1 and power >= -104 (no underflow branch;
 *      the alpha cut keeps smaller powers away from it for every finite opacity).
 *   0  the pipeline-defined binary32 polynomial (< 2 ULP): reproducible bit for bit on a CPU (the oracle's fast reading);
 *      unguarded, so a pixel may break one entry early or late where T (1 - alpha) sits within rounding of 1e-4;
 *   1  the hardware's v_exp_f32 without the guard.
 * With gs_set_blend_contraction(1) mode 3 runs as mode 1: the contracted `power` already differs from the reference's.
 * GS_EXP_MODE sets the initial mode for hosts that cannot call this (the viewer). */
int gs_set_exp_mode(gs_renderer* r, int mode);
/* gs_set_blend_contraction -- render.comp:66 and :87 hold three multiply-adds that GLSL lets a compiler contract into FMAs
 * (the shader has no `precise`).  0 (default): as written, one rounding per operation; 1: the three contractions (5 VALU
 * instructions per blended pair fewer).  The two differ by ULP noise on benign scenes and by up to 3e-3 on scenes of thin,
 * long splats, where `power` is a difference of much larger terms.
 * GS_BLEND_CONTRACTION sets the initial mode. */
int gs_set_blend_contraction(gs_renderer* r, int enabled);
/* gs_set_antialiased -- scenes trained with ANTIALIASED rasterisation (gsplat rasterize_mode="antialiased", splatfacto's
 * antialiased mode, Mip-Splatting's 2D filter) pay for the 0.3 px^2 that preprocess.comp:63-64 adds to the 2D covariance's
 * diagonal by scaling each splat's opacity with a view-dependent factor:
 *     comp = min(1, sqrt(max(0, det(cov2D) / det(cov2D + 0.3 I))))      opacity' = opacity * comp
 * (binary32, det(cov2D) in the same operation order as the dilated determinant; the min only catches rounding past 1, so an
 * opacity <= 1 stays <= 1).  0 (default): off, the reference's pipeline; 1: on.  No reference counterpart: the reference is
 * the non-antialiased pipeline.  Opacity enters neither the cull, the radius, the tile box nor the depth order, so the
 * per-tile lists, the ranges and the depth order are the same as with the mode off; only the record's opacity and alpha cut
 * change (the cut is then taken per frame from opacity', GS_STAGE_ALPHA_CUT shows it).  A frame of scene S with the mode on
 * is bit-identical to the frame, with the mode off, of the scene S' whose opacities are the opacity' values
 * (GS_STAGE_CONIC_OPACITY .w) of that view.  det(cov2D) <= 0 gives comp = 0: the splat stays in the lists and never
 * contributes.  Mip-Splatting's 3D filter (the filter_3D PLY property) and other 2D kernel sizes are out of scope: they
 * change the box and the lists.  Frames already queued finish with the previous setting.  GS_ANTIALIASED=1 sets the initial
 * value at renderer creation (the viewer, pose_shard_host). */
int gs_set_antialiased(gs_renderer* r, int enabled);
/* 1 if the antialiased mode is on, 0 if off, a negative gs_status on error. */
int gs_get_antialiased(gs_renderer* r);
/* Replay frames as ONE captured HIP graph each (answers VulkanContext.h:6 / Renderer.cpp:391-395, 532-717: the
 * reference re-records its render command buffer every frame because dispatch sizes depend on D; here every grid is
 * data-independent, so a frame's launches are captured once per configuration -- resolution, depth-order level,
 * capacity -- and what changes per frame, the uniforms and the output pointers, is read by the kernels from a small
 * parameter block refreshed by one copy ahead of the launch).  Per-pass spans are not recorded in this mode
 * (ms_total still is).  Default off: it lowers the host's cost per frame, not the GPU's.  GS_GRAPH=1 sets the initial mode. */
int gs_set_graph_mode(gs_renderer* r, int enabled);
/* The blend's LOCKSTEP: the four waves of a 16 x 16 tile take every 64-entry chunk of its list together (one workgroup barrier per
 * chunk), so that their gathers of the same splat records meet in the CU's L1.  It changes no pixel (the frames are bit-identical
 * either way), only where the time goes: +25 % of the blend on trained-like scenes (long lists of which an 8 x 8 quadrant keeps one
 * entry in seven: the kernel is bound by its L1 misses), -9 % on scenes whose blend is bound by the pair loop.  mode -1 (default):
 * the renderer measures the rate at which frames complete under both settings over its first 60 to 130 frames, switches lockstep
 * on only where it wins by 3 % in two passes running, and looks again every 4096 frames or when the frame's size changes;
 * 0 / 1: pinned off / on (also GS_BLEND_LOCKSTEP=0 / 1 at renderer creation). */
int gs_set_blend_lockstep(gs_renderer* r, int mode);
/* The setting the next frame will run with (0 / 1; negative: error); *settled (nullable) = 1 once the measurement has decided
 * (or the mode is pinned). */
int gs_get_blend_lockstep(gs_renderer* r, int* settled);
/* The ONE-PASS level 1: k_preprocess files the level-1 candidate records itself -- one device atomic per (workgroup, bin its 256
 * Gaussians touch) -- and the three level-1 kernels are not launched.  It changes no output (taps, images and counts are equal
 * either way).  mode -1 (default): by rule -- bin-local frames with bins of at most 8 x 8 tiles, scenes below the dense-list
 * threshold that have their spatial copy, a bin region (candidate capacity / bins) of at least 5/4 of the last frame's fullest bin,
 * and no more than 8 bins per visible Gaussian; 0: never; 1: wherever the frame's structure allows.  A frame whose bin region runs
 * over is re-run on the three kernels, which then stay for 32 frames.  GS_L1_FUSED=-1 / 0 / 1 sets the initial mode. */
int gs_set_level1_fused(gs_renderer* r, int mode);
/* 1: the most recently enqueued frame took the one-pass level 1; 0: it ran the three level-1 kernels (negative: error). */
int gs_get_level1_fused(gs_renderer* r);
/* The ALPHA-CUT TILE CULL (default on; GS_TILE_CULL=0 / 1 sets the initial value).  render.comp:78 skips an entry whose alpha is
 * below 1/255, i.e. whose `power` is below the Gaussian's alpha cut: a Gaussian reaches no further than the ellipse power = cut,
 * which is usually well inside the 3-sigma tile box of preprocess.comp:160-165.  On the frames of the one-pass level 1 that
 * k_bin_fast orders (depth-order levels 0 .. 3) the per-tile lists the blend walks are made from the tiles that ellipse's bounding
 * rectangle touches (csrc/gs_tile_cull.h, with the slack that makes the rule conservative against the shader's rounded power):
 * every entry left out is one the shader skips at every pixel of the tile, so images, contributions, feature maps and lifts are
 * what they are without the cull.  What describes the REFERENCE's lists does not move either: gs_frame_stats (num_instances is
 * the reference's D; capacity growth and retries follow it) and the taps GS_STAGE_SORTED_TILE / _SORTED_GID / _RANGES /
 * _LISTS_RAW / _RANGES_RAW, which on a culled frame are answered by running level 2 once more over the frame's candidate
 * records with the reference boxes, into buffers of the taps' own.  GS_STAGE_LISTS_CULLED / _RANGES_CULLED show the lists as
 * walked.  Frames of the three-kernel level 1, of the dense lists, of the slab level and of the global path are not culled. */
int gs_set_tile_cull(gs_renderer* r, int enabled);
/* 1 / 0: the switch (negative: error).  *last_frame_culled (nullable): 1 if the most recently enqueued frame's lists are culled. */
int gs_get_tile_cull(gs_renderer* r, int* last_frame_culled);
/* Tile instances in the lists of the last frame as the blend walked them: num_instances unless the frame is culled.  Synchronizes. */
int gs_get_listed_instances(gs_renderer* r, uint64_t* out);
/* Sums of the per-pass spans over all frames retired since the last reset (ms fields are sums,
 * counts are those of the last frame); *frames = number of frames summed.  Synchronizes. */
int gs_get_timing_totals(gs_renderer* r, gs_frame_stats* sum, uint64_t* frames, int reset);
/* Completion-to-completion intervals (ms, GPU timestamps of the blend's end) of consecutive retired frames: the
 * frame time a consumer sees with frames in flight -- what the reference's FPS counter samples once a second
 * (Renderer.cpp:436-444), per frame.  Copies the most recent min(capacity, *n_out) values, oldest first; *n_out =
 * number available (at most 8192 are kept).  Synchronizes. */
int gs_get_frame_intervals(gs_renderer* r, float* out_ms, uint64_t capacity, uint64_t* n_out, int reset);
/* Renderer::retrieveTimestamps (Renderer.cpp:85-100) for the last frame; synchronizes. */
int gs_get_stats(gs_renderer* r, gs_frame_stats* out);
/* The same WITHOUT waiting, for a frame loop that keeps frames in flight (gs_set_frames_in_flight): retires the queued frames
 * that have completed (growing the buffers and re-running on overflow, like gs_synchronize) and returns the statistics of the
 * most recently retired one (all zero before the first).  *frames_retired (nullable) = frames retired since the renderer was
 * created.  blend_redo / blend_resolved are not read here (0). */
int gs_poll_stats(gs_renderer* r, gs_frame_stats* out, uint64_t* frames_retired);
/* Copy a stage buffer of the last frame to host memory; synchronizes.  The per-tile lists live bin-major in HBM;
 * GS_STAGE_SORTED_GID / _SORTED_TILE / _RANGES present them laid end to end in tile order, i.e. as the reference's
 * sorted payload, the tile half of its sorted keys and its tileBoundaryBuffer.  GS_ERR_INVALID ("no frame rendered yet") before
 * the first frame and while the renderer has no last frame (gs_render: a call that failed while retiring queued frames); a
 * refused gs_render changes no tap. */
int gs_debug_download(gs_renderer* r, int stage, void* dst, uint64_t bytes);
/* What every Gaussian contributed to the LAST frame: its weight, the pixels it was blended in, and per pixel the Gaussian that
 * dominates it -- for pruning by significance over a set of views, brush / lasso selection (mask) and click-to-pick (top_id).
 * No reference counterpart.  One more kernel (gs_contrib.hip) walks the per-tile lists and attribute records the frame left in
 * HBM; it reads ranges, lists and records of that frame and writes the four arrays below and nothing the renderer owns: the
 * next frame, the stage taps and captured graphs are unaffected.
 *
 * Per pixel the tile's list is walked exactly as render.comp:61-89 walks it: `power > 0` skips an entry (:68), `alpha < 1/255`
 * skips it (:78), `T (1 - alpha) < 1e-4` ends the walk (:83).  An entry that reaches :87 is BLENDED at that pixel with
 *     w = fl32(alpha * T)        alpha, T: the binary32 values of :87 (T before :88 updates it)
 *     q = w * 2^24 rounded to the nearest integer, ties to even        (the scaling is exact; 6 <= q < 2^24)
 * A pixel is COUNTED if it lies inside the image and mask (if given) is not 0 there.  Then
 *     weight[g] += sum of q over the counted pixels that blend g        (unit: 2^-24 of a pixel's full weight)
 *     pixels[g] += the number of those pixels
 *     top_id[p]  = the id with the largest w at p, the earlier list entry on equal w; 0xFFFFFFFF where nothing was blended
 *                  or p is not counted
 * weight and pixels are ADDED to (zero them once, call after each of many views); top_id is overwritten.  The sums are integers,
 * so they do not depend on the order the adds arrive in: two calls give the same bits.  The mask gates what is recorded, never
 * a pixel's T.
 *
 * The arithmetic is ALWAYS the reference's -- `power` with every product and sum rounded on its own, exp() = glibc's expf
 * restated (exp mode 2), :78 decided on `power` against the record's alpha cut -- whatever gs_set_exp_mode,
 * gs_set_blend_contraction and gs_set_blend_lockstep say.  The default blend (exp mode 3) takes the same decisions by
 * construction, so the counts describe the frame it rendered; the weights are the reference's and differ from what its
 * v_exp_f32 accumulated by rounding noise.  With gs_set_blend_contraction(1) the pass STAYS UNCONTRACTED: where the contracted
 * `power` of the frame fell on the other side of a cut, the pass reports the reference's decision, not the frame's.  With
 * gs_set_antialiased(1) the records carry opacity' and its cut, and the pass follows them.
 *
 * Ids are SCENE ids, also for a scene that is read through its copy in spatial order (the lists hold scene ids).
 *
 * All four members are device pointers on the renderer's device, each nullable: mask [height][width] bytes; weight [N] 64-bit,
 * 8-byte aligned; pixels [N] 32-bit and top_id [height][width] 32-bit, 4-byte aligned.  N = gs_scene_num_vertices, width and
 * height those of the last frame.  The call synchronizes like gs_debug_download (queued frames retire, an overflowed frame is
 * re-run), enqueues on the last frame's stream and returns when the arrays are written.  GS_ERR_INVALID: r or c NULL (checked
 * before any device is touched), no frame rendered yet, a misaligned pointer (judged by its value alone).  All three outputs
 * NULL: nothing is launched.  "No frame rendered yet" is also the answer while the renderer has no last frame (gs_render: after
 * a call that failed while retiring queued frames; nothing is written then); a refused gs_render changes nothing the pass gives. */
typedef struct {
    const uint8_t* mask;
    uint64_t* weight;
    uint32_t* pixels;
    uint32_t* top_id;
} gs_contributions;
int gs_accumulate_contributions(gs_renderer* r, const gs_contributions* c);
/* Per-pixel maps of the LAST frame: caller-supplied per-Gaussian channels blended exactly as render.comp:87 blends the colour
 * (labels, language or DINO features, normals, a heat map of gs_accumulate_contributions' weights, per-Gaussian error), the
 * pixel's coverage, and its expected and median depth -- for compositing over a background or another renderer's output,
 * occlusion against meshes, TSDF fusion and picking a 3D point.  No reference counterpart.  The sibling of
 * gs_accumulate_contributions: one more kernel (gs_features.hip) walks the per-tile lists and attribute records the frame left in
 * HBM; it reads ranges, lists and records of that frame and the caller's `features`, and writes the caller's four arrays and
 * nothing the renderer owns: the next frame, the stage taps and captured graphs are unaffected.
 *
 * Per pixel the tile's list is walked exactly as gs_accumulate_contributions documents it (render.comp:61-89): `power > 0` skips
 * an entry (:68), `alpha < 1/255` skips it (:78), `T (1 - alpha) < 1e-4` ends the walk (:83) -- ALWAYS with the reference's
 * arithmetic: `power` with every product and sum rounded on its own, exp() = glibc's expf restated (exp mode 2), :78 decided on
 * `power` against the record's alpha cut, whatever gs_set_exp_mode, gs_set_blend_contraction and gs_set_blend_lockstep say the
 * frame ran with.  With gs_set_antialiased(1) the records carry opacity' and its cut, and the pass follows them.
 *
 * An entry of Gaussian g that reaches :87 adds, with that line's binary32 alpha and T (T before :88 updates it), starting from
 * F = 0, D = 0, M unset:
 *     F[c] = F[c] + (features[g][c] * alpha) * T     for every channel c            (the order of :87)
 *     D    = D    + (depth[g]       * alpha) * T     depth[g]: the view-space depth of the frame's record (GS_STAGE_DEPTH)
 *     M    = depth[g]   if M is still unset and T * (1 - alpha) < 0.5     (the first blended entry that takes T below one half)
 * and at the walk's end the pixel gets
 *     out_features     = F
 *     out_depth        = D                 the EXPECTED depth, NOT normalised: divide by out_alpha where that is > 0
 *     out_alpha        = fl32(1 - T)       T when the walk ends; a break at :83 leaves T as it was before the breaking entry
 *     out_depth_median = M, or +inf if M is unset
 * All outputs are OVERWRITTEN, never added to.  A pixel with an empty list gets 0, 0, 0, +inf.  Nothing is written for positions
 * outside the image.  Each pixel adds in list order on one lane: the outputs are defined bit for bit, there are no atomics, and
 * two calls give the same bits.  A feature row takes part only at the pixels that blend its Gaussian: a NaN in the row of a
 * Gaussian that is in no tile list reaches no output.  Two facts that follow from the definition:
 *   - While T >= 0.5, :83 cannot fire (alpha <= 0.99 gives T (1 - alpha) >= 0.005), so no walk ends before M is set once T can
 *     fall below one half: out_depth_median is finite exactly where the final T < 0.5.
 *   - With features[g] = (r, g, b) of the frame's records, out_features is the exp-mode-2 image's RGB bit for bit.
 *
 * Ids are SCENE ids, also for a scene that is read through its copy in spatial order: features[g] is the row of scene Gaussian g.
 *
 * Channels are processed in groups of 16 per launch, each launch walking the lists again (the sums of different channels do not
 * depend on one another, so grouping changes no bit); the first also writes alpha and the depths.  Cost: INTEGRATION.md, 3e.
 *
 * features [N][channels] row-major; out_features [height][width][channels], channel innermost; out_alpha, out_depth,
 * out_depth_median [height][width].  All are device pointers to floats on the renderer's device, 4-byte aligned and nothing
 * more; each output is nullable; features may be NULL only with channels == 0.  N = gs_scene_num_vertices, width and height
 * those of the last frame, channels 0 .. GS_FEATURE_CHANNELS_MAX.  The call synchronizes like gs_accumulate_contributions (queued
 * frames retire, an overflowed frame is re-run), enqueues on the last frame's stream and returns when the arrays are written.
 * GS_ERR_INVALID, checked before any device is touched: r or m NULL; channels > GS_FEATURE_CHANNELS_MAX; channels > 0 with
 * features NULL, or with out_features NULL while features is given (rejected rather than ignored); a misaligned pointer (judged
 * by its value alone).  GS_ERR_INVALID also when no frame has been rendered yet, and while the renderer has no last frame
 * (gs_render: after a call that failed while retiring queued frames; nothing is written then); a refused gs_render changes
 * nothing the pass gives.  All four outputs NULL: success, nothing is
 * launched.  channels == 0 with out_features given: that output is not touched. */
#define GS_FEATURE_CHANNELS_MAX 256
typedef struct {
    const float* features;      /* [N][channels] row-major, device; may be NULL only with channels == 0 */
    uint32_t     channels;      /* 0 .. GS_FEATURE_CHANNELS_MAX */
    float* out_features;        /* [height][width][channels], channel innermost */
    float* out_alpha;           /* [height][width] */
    float* out_depth;           /* [height][width]  expected depth, NOT normalised */
    float* out_depth_median;    /* [height][width] */
} gs_feature_maps;
int gs_blend_features(gs_renderer* r, const gs_feature_maps* m);
/* Per-pixel values of the LAST frame carried back onto its Gaussians: the transpose of gs_blend_features in its `features`
 * argument, with the weights of gs_accumulate_contributions -- for lifting 2D maps into the scene without training (segmentation
 * masks, multi-label votes, DINO / CLIP features, per-pixel error: out[g] / out_weight[g] accumulated over a camera set), for the
 * gradient of gs_blend_features with respect to `features` (the frame's geometry is a constant), and for re-baking colours or
 * per-Gaussian statistics from edited images.  No reference counterpart.  One more kernel (gs_lift.hip) walks the per-tile lists
 * and attribute records the frame left in HBM; it reads ranges, lists and records of that frame and the caller's `values` and
 * `mask`, and adds to the caller's two arrays and writes nothing the renderer owns: the next frame, the stage taps and captured
 * graphs are unaffected.
 *
 * Per pixel the tile's list is walked exactly as gs_accumulate_contributions documents it (render.comp:61-89): `power > 0` skips
 * an entry (:68), `alpha < 1/255` skips it (:78), `T (1 - alpha) < 1e-4` ends the walk (:83) -- ALWAYS with the reference's
 * arithmetic: `power` with every product and sum rounded on its own, exp() = glibc's expf restated (exp mode 2), :78 decided on
 * `power` against the record's alpha cut, whatever gs_set_exp_mode, gs_set_blend_contraction and gs_set_blend_lockstep say the
 * frame ran with.  With gs_set_antialiased(1) the records carry opacity' and its cut, and the pass follows them.  Ids are SCENE
 * ids, also for a scene that is read through its copy in spatial order: out[g] is the row of scene Gaussian g.
 *
 * A pixel is COUNTED if it lies inside the image and mask is NULL or not 0 there.  The mask gates what is recorded, never a
 * pixel's T.  For a counted pixel p and an entry of Gaussian g that reaches :87 there, with that line's binary32 alpha and T (T
 * before :88 updates it):
 *     w              = fl32(alpha * T)                         the w of gs_accumulate_contributions
 *     out[g][c]     += (double)w * (double)values[p][c]        for every channel c; the product of two binary32 values is exact
 *     out_weight[g] += (double)w
 * Both arrays are ADDED to (zero them once, call after each of many views).  Every add is a binary64 add; the ORDER of the adds
 * is unspecified.  The sums are not integers, so -- unlike gs_accumulate_contributions -- two calls need not give the same bits.
 * The result is within (n - 1) * 2^-53 * sum|terms| of the exact sum of the n terms a Gaussian receives (plus what the array
 * held), and it is bit-exact whenever a Gaussian receives at most two terms into an element that held zero, because a binary64
 * add is commutative.  A `values` row takes part only through the entries its own counted pixel blends: a NaN at an uncounted
 * pixel, at a pixel outside every list, or at a pixel that skipped the entry reaches no output (a term is selected, never
 * multiplied by zero); the values of an uncounted pixel are not read at all.
 *
 * Channels are processed in groups of 16 per launch, each launch walking the lists again; the first also adds the weights.  Per
 * launch there is one device atomic per (blended entry, tile, channel), never one per pixel.  Cost: INTEGRATION.md, 3f.
 *
 * values [height][width][channels], channel innermost, floats, 4-byte aligned and nothing more; mask [height][width] bytes, any
 * address; out [N][channels] row-major and out_weight [N], doubles, 8-byte aligned.  All are device pointers on the renderer's
 * device.  out and out_weight must be ORDINARY device allocations (hipMalloc, a torch tensor): the adds are the hardware's
 * global_atomic_add_f64, which fine-grained or host-coherent memory need not honour.  N = gs_scene_num_vertices, width and
 * height those of the last frame, channels 0 .. GS_LIFT_CHANNELS_MAX.  The call synchronizes like gs_blend_features (queued frames
 * retire, an overflowed frame is re-run), enqueues on the last frame's stream and returns when the arrays are written.
 * That stream is the renderer's own and is NON-BLOCKING: the call waits for nothing the caller has queued elsewhere.  values, mask
 * and the contents of out and out_weight -- the zeros they start from included -- must be COMPLETE when the call is made: the
 * caller synchronises the stream that produces them first (hipStreamSynchronize, or an event this thread has waited on).  The
 * Python wrapper does so for torch's current stream.
 * GS_ERR_INVALID, checked before any device is touched: r or l NULL; channels > GS_LIFT_CHANNELS_MAX; channels > 0 with values
 * NULL, or with out NULL while values is given (rejected rather than ignored); a misaligned pointer (judged by its value alone).
 * GS_ERR_INVALID also when no frame has been rendered yet, and while the renderer has no last frame (gs_render: after a call
 * that failed while retiring queued frames; nothing is added then); a refused gs_render changes nothing the pass gives, up to
 * the order of its adds.  out and out_weight both NULL: success, nothing is launched.
 * channels == 0 with out_weight given: only the weights are written; out, if given, is not touched. */
#define GS_LIFT_CHANNELS_MAX 256
typedef struct {
    const float*   values;      /* [height][width][channels], channel innermost, device; NULL only with channels == 0 */
    uint32_t       channels;    /* 0 .. GS_LIFT_CHANNELS_MAX */
    const uint8_t* mask;        /* [height][width] bytes, nullable: only pixels where it is not 0 are counted */
    double*        out;         /* [N][channels] row-major, ADDED to */
    double*        out_weight;  /* [N], ADDED to: the sum of w itself */
} gs_pixel_lift;
int gs_lift_pixels(gs_renderer* r, const gs_pixel_lift* l);
/* The backward of the blend of the LAST frame: from dL/d(image RGB) and dL/d(out_alpha of gs_blend_features) the gradients with
 * respect to what shapes each splat on the screen -- its colour, opacity, conic and screen position -- summed per Gaussian.  It
 * is what the rasteriser backward of a 3DGS trainer computes; the projection half (means, scales, quaternions, SH -> uv, conic,
 * rgb) is gs_project_backward, below.  No reference counterpart.  One more kernel (gs_backward.hip)
 * walks the per-tile lists and attribute records the frame left in HBM, twice per tile inside one launch; it reads ranges, lists
 * and records of that frame and the caller's two maps, adds to the caller's four arrays and writes nothing the renderer owns.
 *
 * Per pixel the list is walked exactly as gs_lift_pixels documents it (render.comp:61-89), with the reference's arithmetic
 * whatever mode the frame ran in.  For the pixel's blended entries i = 1 .. L (those that reach :87), in list order:
 *     alpha_i, T_i   the binary32 values :87 reads, T_i before :88
 *     prod_i         fl32(o * e_i), e_i the exp of :77 (glibc's expf restated); alpha_i = min(0.99, prod_i)
 *     dx_i, dy_i     the binary32 values of :66
 *     m_i            fl32(1 - alpha_i), at least 0.01
 *     T_f            the binary32 T at the end of the walk (a break at :83 leaves it as it was, as in gs_blend_features)
 *     c00 c01 c11 o, u v r g, b   the entry's record;   G = grad_rgb[p];   ga = grad_alpha[p], 0 when grad_alpha is NULL
 * The decisions -- the `power > 0` skip, the 1/255 skip, the break -- are constants and carry no gradient.  Everything below is
 * binary64 on exact conversions of those binary32 values:
 *     a_i  = G_r r + G_g g + G_b b        w_i = (double)fl32(alpha_i T_i)        R_i = sum over j > i of a_j w_j
 *     d_colour[g] += w_i * G                                   (this IS gs_lift_pixels of grad_rgb)
 *     galpha_i = T_i a_i - (R_i - ga T_f) / m_i
 *     flows_i  = (prod_i <= 0.99f)        false for a clamped alpha and for a NaN product: those pairs add only to d_colour
 *     if flows_i:
 *       d_opacity[g] += galpha_i * e_i
 *       gp = galpha_i * alpha_i
 *       d_conic[g]   += gp * (-0.5 dx^2, -dx dy, -0.5 dy^2)
 *       d_uv[g]      += gp * (-(c00 dx + c01 dy), -(c01 dx + c11 dy))
 * A term exists only for a (pixel, blended entry) pair inside the image: a NaN in grad_rgb at a pixel reaches only the Gaussians
 * blended there (a term is selected, never multiplied by zero), and the maps are not read at all under a tile whose list is
 * empty.  Every add is a binary64 add.  The order of the adds is unspecified, and so is the association inside a term, including
 * whether R_i is a suffix sum or a total minus a prefix: the contract is a bound, not a bit pattern.  With n_g the number of terms
 * Gaussian g receives and A the sum of the terms' magnitudes (every constituent by its absolute value, R_i entering as
 * (L + 2) sum_j |a_j| w_j), the result is within (n_g + 8) 2^-53 A of the exact sum; tests/backward_reference.py derives it.
 * Tile cull (gs_set_tile_cull) changes no sum: an entry the cull drops is one every pixel of the tile skips.
 *
 * Scene ids, ordinary device allocations for the outputs (global_atomic_add_f64), inputs and the contents of the outputs COMPLETE
 * before the call, the renderer's own NON-BLOCKING stream, the synchronisation (queued frames retire, an overflowed frame is
 * re-run, the call returns when the arrays are written), "no frame rendered yet" and the behaviour after a refused or failed
 * gs_render: all as gs_lift_pixels states them.
 * GS_ERR_INVALID, checked before any device is touched: r or g NULL; an output given while grad_rgb is NULL; a float pointer
 * that is not 4-byte aligned or a double pointer that is not 8-byte aligned (judged by its value alone).  All four outputs NULL:
 * success, nothing is launched.  width and height are those of the last frame, N = gs_scene_num_vertices.  Cost: INTEGRATION.md, 3g. */
typedef struct {
    const float* grad_rgb;    /* [height][width][3] dL/d(image RGB); required unless every output is NULL */
    const float* grad_alpha;  /* [height][width]    dL/d(out_alpha of gs_blend_features); nullable = zeros */
    double* d_colour;         /* [N][3]  ADDED to */
    double* d_opacity;        /* [N]     ADDED to */
    double* d_conic;          /* [N][3]  c00 c01 c11, ADDED to */
    double* d_uv;             /* [N][2]  ADDED to */
} gs_blend_grads;
int gs_blend_backward(gs_renderer* r, const gs_blend_grads* g);
/* The projection half of the backward of the LAST frame: from the gradients with respect to each visible Gaussian's screen-space
 * record -- what gs_blend_backward sums -- to the gradients with respect to the six tensors gs_scene_to_device_arrays exports
 * (means, log-scales, quaternions, opacity logits, SH DC and rest).  With gs_blend_backward in front of it this is the whole
 * backward of a frame, at the frame's values.  No reference counterpart.  One kernel (gs_project_backward.hip), one lane per
 * Gaussian; it reads the scene, the frame's records and visibility and the caller's four arrays, adds to the caller's six and
 * writes nothing the renderer or the scene owns.  No per-frame kernel is involved.
 *
 * THE FUNCTION.  For a Gaussian with stored binary32 position p, activated scale s, stored quaternion q (w x y z), activated opacity
 * o and the 16 x 3 SH coefficients AS STORED (binary16 storage widened exactly), and the frame's gs_uniforms, the record is this
 * exact real function F.  Every constant is the frame's binary32 constant converted exactly (0.3f, 0.5f, the constants of the SH
 * basis; lim_x = the binary32 product 1.3f * tan_fovx); P[r][c] = proj_mat[4 c + r], V[r][c] = view_mat[4 c + r]; W, H = width, height.
 *     h = P (p, 1)                       t = V (p, 1), rows 0..2
 *     u = ((h0 / h3 + 1) W - 1) / 2      v = ((h1 / h3 + 1) H - 1) / 2
 *     tx = clamp(t0 / t2, +-lim_x) t2,  ty likewise.  THE BRANCH OF EACH CLAMP IS A CONSTANT, taken as the frame took it: by the
 *          binary32 comparison of k_preprocess on its binary32 t0 / t2.  Where the clamp binds, tx = c t2 with c = +-lim_x is still
 *          differentiated through t2.
 *     J = [[fx / t2, 0, -fx tx / t2^2], [0, fy / t2, -fy ty / t2^2]]       fx = W / (2 tan_fovx), fy = H / (2 tan_fovy)
 *     A = J V(3 x 3)
 *     Sigma = R(q^) diag(s^2) R(q^)^T,  q^ = q / |q|,  R the standard rotation matrix of a unit quaternion: the matrix the scene's
 *          cov3D planes hold, recomputed from s and q, not read from the rounded planes
 *     cov = A Sigma A^T
 *     m00 = cov00 + 0.3    m11 = cov11 + 0.3    m01 = cov01    det = m00 m11 - m01^2
 *     (c00, c01, c11) = (m11, -m01, m00) / det
 *     o' = o                                  in a frame rendered with gs_set_antialiased off
 *     o' = o comp,  comp = sqrt(det_raw / det),  det_raw = cov00 cov11 - cov01^2          in an antialiased frame.  There is no
 *          min(1, .): in exact arithmetic it never binds.  Where the binary64 det_raw <= 0, comp is the constant 0.
 *     d = (p - camera_position) / |p - camera_position|
 *     rgb_k = 0.5 + sum_j B_j(d) sh[j][k],  B_j the sixteen basis polynomials (signs and constants included) of preprocess.comp's
 *          compute_sh, as polynomials in three independent variables.  Channel 0 is max(0, .): ITS BRANCH IS A CONSTANT, it flows
 *          iff the frame's record holds r > 0.
 *     parameters:  s = exp(ls),  o = 1 / (1 + exp(-l)),  q^ = q / |q|:  the derivatives are s d/ds, o (1 - o) d/do and
 *          (g - q^ (q^ . g)) / |q|, evaluated at the STORED values, |q| the stored quaternion's own norm in binary64 -- the
 *          gradients with respect to the six tensors gs_scene_to_device_arrays returns.
 * Radius, tile box, depth, alpha cut and the culls carry no gradient; neither does the camera HERE: its gradient is
 * gs_camera_backward's, below.
 * With inputs g_colour[3], g_opacity, g_conic[3] (c00 c01 c11), g_uv[2] per Gaussian (binary64; a NULL array = zeros) every parameter
 * theta of a VISIBLE Gaussian -- one whose GS_STAGE_TILES value of that frame is not 0 -- receives  sum_x g_x dx/dtheta  over the
 * nine record values x (o' for the opacity), by the chain rule over the nodes above.  Everything is binary64 on exact conversions
 * of the stored binary32 values and the uniforms; the association is unspecified: the contract is a bound, not a bit pattern --
 * with every input gradient, partial and product taken by its absolute value and the condition factor of each cancelling
 * intermediate (h3, t2, the cov2D entries, det, det_raw) carried along into a magnitude A, |result - exact| <= 660 * 2^-53 * A;
 * tests/project_backward_reference.py derives it and counts the 660.
 *   * Outputs are ADDED to (zero them once; gradients accumulate over a camera set).  One writer per element: two calls give the
 *     same bits.  An add of an exact zero may be omitted (it is: an element no gradient reaches keeps its bits).
 *   * A Gaussian the frame culled is not touched at all: neither its inputs nor its outputs are read or written.
 *   * A NaN among one Gaussian's inputs reaches that Gaussian's rows only.
 *   * sh_rest_coeffs = K in {0, 3, 8, 15}: d_sh_rest is [N][K][3], the coefficients 1 .. K; higher bands are not written (they
 *     still shape rgb, and through d the means).
 * THE SCENE MUST STILL HOLD WHAT THE FRAME RENDERED: the pass reads positions, scales, rotations, opacities and SH from the scene
 * as it is now.  gs_scene_update_from_device_arrays, gs_scene_transform or gs_scene_quantize_sh between the frame and this call
 * give the gradient of no frame.  It answers for the frame, not for a gs_set_antialiased made after it.
 * Scene ids, ordinary device allocations, inputs and the contents of the outputs COMPLETE before the call, the renderer's own
 * NON-BLOCKING stream, the synchronisation (queued frames retire, an overflowed frame is re-run, the call returns when the arrays
 * are written), "no frame rendered yet" and the behaviour after a refused or failed gs_render: all as gs_lift_pixels states them.
 * GS_ERR_INVALID, checked before any device is touched: r or g NULL; a pointer that is not 8-byte aligned (judged by its value
 * alone); sh_rest_coeffs not in {0, 3, 8, 15}, or not 0 while d_sh_rest is NULL.  All six outputs NULL: success, nothing is
 * launched.  N = gs_scene_num_vertices.  Cost: INTEGRATION.md, 3h. */
typedef struct {
    const double* d_colour;   /* [N][3]  dL/d(r g b of the record); nullable = zeros */
    const double* d_opacity;  /* [N]     dL/d(opacity of the record); nullable = zeros */
    const double* d_conic;    /* [N][3]  c00 c01 c11; nullable = zeros */
    const double* d_uv;       /* [N][2]  nullable = zeros */
    double* d_means;          /* [N][3]  ADDED to */
    double* d_log_scales;     /* [N][3]  ADDED to */
    double* d_quats;          /* [N][4]  w x y z, ADDED to */
    double* d_opacity_logits; /* [N]     ADDED to */
    double* d_sh_dc;          /* [N][3]  ADDED to */
    double* d_sh_rest;        /* [N][sh_rest_coeffs][3], RGB innermost, ADDED to */
    uint32_t sh_rest_coeffs;  /* 0, 3, 8 or 15: higher bands are not written */
} gs_project_grads;
int gs_project_backward(gs_renderer* r, const gs_project_grads* g);
/* The camera half of the backward of the LAST frame, gs_project_backward's sibling: from the same four per-Gaussian input
 * gradients to the gradients with respect to the frame's gs_uniforms -- what refining a pose, tracking a camera against a held
 * scene or registering a photograph need.  gs_camera_uniforms_backward (host) carries them on to the gs_camera's position and
 * rotation.  No reference counterpart.  Two launches (gs_camera_backward.hip): the per-Gaussian chain is the very one
 * gs_project_backward evaluates (gs_project_chain.h), followed by a reduction over the visible Gaussians; the pass reads the scene,
 * the frame's records and visibility and the caller's four arrays, adds to the caller's three and writes nothing else but a
 * scratch buffer of partial sums the renderer owns.  No per-frame kernel is involved.
 *
 * THE FUNCTION is the record function F above with the same branches as constants, exactly as they are there: each clamp's
 * branch as k_preprocess took it in binary32, red's max(0, .) by the record, visibility by GS_STAGE_TILES, det_raw <= 0 in an
 * antialiased frame.  It is differentiated with respect to the frame's uniforms instead of the Gaussian's parameters:
 *     V[r][c] = view_mat[4 c + r], rows 0..2, columns 0..3: enters through t = V (p, 1) and through A = J V(3 x 3).  Row 3 is
 *         not read by F: it carries no gradient and the element is left untouched.
 *     P[r][c] = proj_mat[4 c + r], rows 0, 1 and 3: enters through h = P (p, 1) to u v.  Row 2 is not read by F: left untouched.
 *     camera_position[0..2]: enters through d = (p - c) / |p - c| to rgb.
 * CARRYING NO GRADIENT: tan_fovx, tan_fovy, width, height, lim_x, lim_y (the intrinsics -- fx, fy and the clamp's limits are
 * constants here); the culls, radius, depth, tile box and alpha cut.
 * For each of these 27 uniforms x the result is  sum over the visible Gaussians i of the last frame of  sum_y g_y[i] dy_i/dx
 * over the nine record values y gs_project_backward lists.  With the chain's nodes (g_t = dL/dt, gA = dL/dA, g_h = dL/dh rows
 * 0, 1, 3, g_d = dL/dd, jaa = J[a][a], ja2 = J[a][2]) Gaussian i's terms are
 *     dV[r][c] = g_t[r] (p, 1)[c] + (r < 2 ? jaa[r] gA[r][c] : ja2[0] gA[0][c] + ja2[1] gA[1][c])  for c < 3;   dV[r][3] = g_t[r]
 *     dP[r][c] = g_h[r] (p, 1)[c]
 *     dc       = -(g_d - d (d . g_d)) / |p - c|
 * Every operation is binary64 on exact conversions of the stored binary32 values and of the frame's binary32 uniforms; the
 * association is unspecified, so the contract is a bound: with A_i the magnitude of Gaussian i's term (every input gradient,
 * partial and product by its absolute value, the condition factors of h3, t2, the cov2D entries, det and det_raw carried along),
 *     |result - exact| <= 650 * 2^-53 * sum_i A_i  +  (n_visible + 1) * 2^-53 * sum_i A_i   (+ 2^-53 of what the element held)
 * -- the per-term path constant, and the summation of n_visible terms in any order plus the add into the caller's array.
 * tests/camera_backward_reference.py derives it and counts both constants.
 *   * Outputs are ADDED to: one add per element of what the call computed (zero them once; gradients accumulate over a camera
 *     set).  An add of an exact zero may be omitted (it is: the element keeps its bits).
 *   * All three outputs NULL: success, nothing is launched.  Every Gaussian culled: nothing is added.
 *   * A Gaussian the frame culled is not touched: its inputs are not read, a NaN in its rows changes nothing.  A NaN in a visible
 *     Gaussian's row reaches every output element that Gaussian has a term in.
 *   * Two calls on the same frame with the same inputs give the same bits: no floating-point atomics anywhere in the pass, and
 *     the association is fixed for a given N and build.  At most GS_CAMERA_BACKWARD_LANES lanes are launched, one per Gaussian in
 *     the order the frame read the scene; a scene with more Gaussians is strided over (lane l takes l, l + LANES, ...).
 *   * It answers for the last frame and ITS uniforms, not for a gs_set_antialiased made after it; the scene must still hold what
 *     the frame rendered (as gs_project_backward states it).
 * Scene ids, ordinary device allocations, inputs and the contents of the outputs COMPLETE before the call, the renderer's own
 * NON-BLOCKING stream, the synchronisation (queued frames retire, an overflowed frame is re-run, the call returns when the arrays
 * are written), "no frame rendered yet" and the behaviour after a refused or failed gs_render: all as gs_lift_pixels states them.
 * GS_ERR_INVALID, checked before any device is touched: r or g NULL; a pointer that is not 8-byte aligned (judged by its value
 * alone).  N = gs_scene_num_vertices.  Cost: INTEGRATION.md, 3i. */
#define GS_CAMERA_BACKWARD_LANES 131072u
typedef struct {
    const double* d_colour;          /* [N][3] inputs exactly as gs_project_grads: nullable = zeros */
    const double* d_opacity;         /* [N]    */
    const double* d_conic;           /* [N][3] */
    const double* d_uv;              /* [N][2] */
    double* d_view_mat;              /* [16] device, laid out as view_mat; rows 0..2 ADDED to, row 3 untouched; nullable */
    double* d_proj_mat;              /* [16] device, laid out as proj_mat; rows 0, 1, 3 ADDED to, row 2 untouched; nullable */
    double* d_camera_position;       /* [3]  device, ADDED to; nullable */
} gs_camera_grads;
int gs_camera_backward(gs_renderer* r, const gs_camera_grads* g);
/* Host only, no device: from the gradients with respect to gs_camera_uniforms' view_mat, proj_mat and camera_position (host
 * copies of what gs_camera_backward summed; any values are taken, every row included) to the gradients with respect to the
 * gs_camera's position and rotation.  Binary64.  It is the gradient of the exact real function behind gs_camera_uniforms,
 *     M = T(position) mat4_cast(rotation)  (the quaternion NOT normalised, as the forward),   view = M^-1,   proj = persp view,
 *     then the y and z rows of view and the y row of proj negated;   camera_position = position  (the direct term),
 * evaluated at the binary32 camera values converted exactly (persp from fov, near_plane, far_plane, width and height, which
 * carry no gradient):  g_M = -M^-T g_view M^-T.  Outputs are WRITTEN.  d_rotation (w x y z) is the gradient with respect to the
 * RAW quaternion: a caller who keeps a unit quaternion projects it onto the tangent of the sphere themselves (as
 * gs_transform_camera, nothing here normalises).  GS_ERR_INVALID: a null argument, an empty framebuffer. */
int gs_camera_uniforms_backward(const gs_camera* cam, uint32_t width, uint32_t height,
                                const double d_view_mat[16], const double d_proj_mat[16], const double d_camera_position[3],
                                double d_position[3], double d_rotation[4]);   /* host pointers; outputs WRITTEN */
/* The photometric loss of a trainer's step and its image gradient: what stands between a rendered frame and gs_blend_backward.
 * No reference counterpart.  The loss is the one the 3DGS trainers minimise (Inria loss_utils.ssim, gsplat, fused-ssim):
 * (1 - lambda) L1 + lambda (1 - SSIM), an 11 x 11 Gaussian window of sigma 1.5, "same" zero padding, lambda = 0.2 by custom.
 *
 * THE FUNCTION, in exact real arithmetic.  x = image, y = target: binary32, [height][width] pixels of 3 channels with a pixel
 * stride of 3 or 4 floats each (stride 4 lets the renderer's RGBA go in uncopied; its fourth float is never read).
 *     g[k] = exp(-(k - 5)^2 / 4.5) / sum,  k = 0..10;    w = g g^T;
 *     a*  = the 11 x 11 correlation of a map with w, per channel, with zeros outside the image;
 *     n = 3 height width;    C1 = 1e-4;    C2 = 9e-4.
 * Forward:
 *     mu1 = x*   mu2 = y*   s11 = (x^2)* - mu1^2   s22 = (y^2)* - mu2^2   s12 = (x y)* - mu1 mu2
 *     A = 2 mu1 mu2 + C1    B = 2 s12 + C2    C = mu1^2 + mu2^2 + C1    D = s11 + s22 + C2    S = A B / (C D)
 *     l1 = sum |x - y| / n    ssim = sum S / n    mse = sum (x - y)^2 / n    loss = (1 - lambda) l1 + lambda (1 - ssim)
 * Gradient:
 *     P1 = 2 mu2 (B - A) / (C D) + 2 mu1 S (1 / D - 1 / C)      P2 = -S / D      P3 = 2 A / (C D)
 *     d loss / d x = (1 - lambda) sign(x - y) / n  -  (lambda / n) (P1* + 2 x P2* + y P3*)        sign(0) = 0
 * (w is symmetric, so the zero-padded correlation is its own transpose.)
 *
 * NUMERICAL CONTRACT.  Binary64 on exact conversions of the binary32 inputs (a product of two of them is exact); g is the
 * binary64 rounding of its definition; C1 and C2 are the binary64 roundings of theirs.  The association is open -- separable or
 * direct, fused multiply-add or not -- so the contract is a bound against the exact value: the roundings of the loosest
 * permitted association, times 2^-53, times the magnitude, where each cancelling intermediate (s11, s22, s12, B - A,
 * 1 / D - 1 / C) enters by the sum of its constituents' absolute values and each division by its condition.  A grad_rgb element
 * is the binary64 value rounded once to binary32: it adds 2^-24 |want| and a denormal floor of 2^-149.  A term adds
 * (n + K) 2^-53 sum |addends|.  tests/photometric_loss_reference.py derives the bound and counts its constants (K_CONV = 124 per
 * correlation); tests/test_photometric_loss_api.py holds that module to torch.autograd and to binary80.
 *   * No atomics: per-workgroup partial sums go to a row of the renderer's scratch and one workgroup adds the rows in a fixed
 *     order.  Two calls with the same inputs and size give the same bits in terms and grad_rgb.  Outputs are WRITTEN.
 *   * A NaN or infinity goes where the arithmetic takes it: the terms, and grad_rgb within 10 pixels (Chebyshev distance) of the
 *     bad pixel.  Everywhere else grad_rgb is the finite value the contract bounds.  The zero padding is a zero, never a product
 *     with data.
 *   * lambda_dssim == 0: the window is never evaluated, one pass runs, terms[2] is written as a quiet NaN ("not evaluated"),
 *     and grad_rgb = fl32(sign(x - y) / n).
 *   * grad_rgb == NULL: forward only -- the evaluation call, for logging PSNR and SSIM.  Both outputs NULL: success, nothing
 *     is launched.
 * THE RENDERER gives the call its device, its non-blocking stream and a home for scratch (gs_loss.hip: three binary64 maps of
 * the image's size, 72 bytes per pixel, when grad_rgb is asked for with lambda > 0; 24 bytes per tile of 16 x 16 pixels
 * otherwise).  Scratch grows on demand and is freed with the renderer.  width and height are NOT tied to the last frame: the
 * call neither reads nor changes it, works before any frame was rendered and after a refused or failed gs_render, and a pass
 * over the last frame made after it answers as if it had not been called.  It is ordered behind queued frames -- they retire
 * first, as for the passes over the last frame, so image may be the buffer a gs_render that has not retired is still writing
 * (an error of a retiring frame is this call's error) -- and returns synchronised.  Inputs written on other streams must be
 * COMPLETE before the call, as gs_lift_pixels states.
 * GS_ERR_INVALID, checked before any device is touched (r is not dereferenced first): r or l NULL; image or target NULL while
 * an output is asked for; width or height outside 1 .. GS_PHOTO_LOSS_MAX_EXTENT; a stride other than 3 or 4; lambda_dssim
 * outside [0, 1] or NaN; a float pointer that is not 4-byte aligned or terms not 8-byte aligned (judged by its value alone).
 * Cost: INTEGRATION.md, 3j. */
#define GS_PHOTO_LOSS_MAX_EXTENT 16384
typedef struct {
    const float* image;    /* [height][width][image_stride]   first 3 floats of a pixel are read */
    const float* target;   /* [height][width][target_stride] */
    int width, height;     /* 1 .. 16384 each; NOT tied to the last frame */
    int image_stride, target_stride;   /* 3 or 4 */
    double lambda_dssim;   /* in [0, 1] */
    double* terms;         /* device, [4] = loss, l1, ssim, mse; WRITTEN; nullable */
    float*  grad_rgb;      /* device, [height][width][3] = d loss / d image, WRITTEN; nullable;
                              exactly what gs_blend_backward takes */
} gs_photo_loss;
int gs_photometric_loss(gs_renderer* r, const gs_photo_loss* l);
/* The LAST frame's visibility as the mask gs_scene_adam_step takes: mask[id] = (the frame's GS_STAGE_TILES value of Gaussian id
 * != 0) ? 1 : 0, by SCENE id (also on a scene that keeps a copy in spatial order), N = gs_scene_num_vertices bytes of device
 * memory on the scene's device.  accumulate != 0: the byte is ORed into what mask[id] holds -- the union over a camera set; zero
 * the mask once.  One kernel (gs_optim.hip).  No reference counterpart.  Ordinary device allocations, the mask's contents
 * COMPLETE before an accumulating call, the renderer's own NON-BLOCKING stream, the synchronisation (queued frames retire, an
 * overflowed frame is re-run, the call returns when the mask is written), "no frame rendered yet" and the behaviour after a
 * refused or failed gs_render: all as gs_project_backward states them.
 * GS_ERR_INVALID, checked before any device is touched: r or mask NULL. */
int gs_visible_mask(gs_renderer* r, uint8_t* mask, int accumulate);

/* ---- the optimiser's step: a sparse Adam on the trainer's tensors that leaves the scene ready for the next frame -----------
 * One Adam step of the Gaussians of a mask ("SelectiveAdam" / "SparseGaussianAdam": a Gaussian the frames did not see is not
 * stepped and its moments do not decay), in the caller's tensors AND in the scene: the parameters, gradients and moments are
 * the six PLY-domain arrays of gs_device_arrays and their companions; the scene receives the activated values of the new
 * parameters.  No reference counterpart.  One kernel (gs_optim.hip: k_adam_step), then the load-time passes over what changed.
 *
 * THE UPDATE, for every masked Gaussian and every element of every given group, with p, m, v the stored binary32 parameter and
 * moments converted exactly and g the binary64 gradient.  All arithmetic is binary64, every operation is rounded on its own
 * (the unit is built with -ffp-contract=off), in exactly this order:
 *     m' = (beta1 * m) + ((1 - beta1) * g)              (1 - beta1) and (1 - beta2) formed once, in binary64
 *     v' = (beta2 * v) + (((1 - beta2) * g) * g)
 *     d  = (sqrt(v') / sqrt(bias_correction2)) + eps    sqrt and / are IEEE; sqrt(bias_correction2) formed once on the host
 *     p' = p - ((lr / bias_correction1) * (m' / d))     lr / bias_correction1 formed once on the host, per group
 *     exp_avg <- fl32(m')    exp_avg_sq <- fl32(v')    param <- fl32(p')        one rounding each, at the store
 * This is torch.optim.Adam's update (amsgrad = False, no weight decay, not maximize) with the moments kept in binary32; the
 * update uses the unrounded m' and v'.  The order is fixed and every operation is IEEE: THE CONTRACT IS A BIT PATTERN, not a
 * bound (tests/adam_step_reference.py restates it in numpy).
 *   * An UNMASKED Gaussian: nothing is read and nothing is written -- not its parameters, moments or gradients, not the scene's
 *     rows.  Its moments do not decay (a dense Adam would go on moving it by its old momentum).
 *   * A NaN or infinite gradient reaches the masked Gaussian's own elements only.
 *   * zero_grads != 0: exactly the elements that were read as g are set to +0.0, so that gs_project_backward, which ADDS, can
 *     go on using tensors that were zeroed once.
 * THE SCENE.  For each masked Gaussian the planes of every STEPPED group are written from the new binary32 parameters with the
 * arithmetic of gs_scene_from_device_arrays (exp: libm's expf restated, for the scales; q * (1 / sqrtf(dot)) for the rotation;
 * 1 / (1 + expf(-l)) for the opacity; SH copied): afterwards the scene's blob is BIT FOR BIT what
 * gs_scene_update_from_device_arrays of the new parameters over those rows would have made -- with one difference: the SH
 * bands beyond sh_rest_coeffs KEEP what the scene holds (the update zeroes them when it is given sh_rest).  A group that is
 * not stepped keeps its planes.  What is derived from what changed is redone on `stream` with the same passes and under the
 * same conditions as gs_scene_update_from_device_arrays: the copy in spatial order (its order stays), cov3D after log_scales
 * or quats, the binary16 SH block of a quantised scene after sh_dc or sh_rest, the alpha cuts and the opacity flag behind exp
 * mode 3 after opacity_logits.  No device pointer a renderer holds changes, so the scene's renderers -- captured graphs included
 * -- go on working.
 * stream: a hipStream_t (NULL: the default stream).  The step is enqueued on it, behind what the caller has enqueued there;
 * the call returns after synchronising it.  Tensors written on OTHER streams (gs_project_backward's gradients are written on
 * the renderer's stream, but that call returns synchronised) must be complete before the call.  Frames in flight read the scene
 * while they run: call gs_synchronize on EVERY renderer of the scene first, as gs_scene_update_from_device_arrays states.
 * All pointers are device pointers on the scene's device; N = gs_scene_num_vertices rows each.
 * GS_ERR_INVALID, checked before any device is touched: s or a NULL; a group with some but not all of its four pointers; a
 * param, exp_avg or exp_avg_sq pointer that is not 4-byte aligned, a grad pointer that is not 8-byte aligned (judged by their
 * values alone); sh_rest_coeffs not in {0, 3, 8, 15}, or sh_rest given with 0; an lr that is not finite or < 0 (of a given
 * group); beta1 or beta2 outside [0, 1); eps not finite or < 0; a bias correction outside (0, 1].  A call with no group at
 * all, or on a scene of no Gaussians, succeeds and does nothing.  Cost: INTEGRATION.md, 3k. */
typedef struct {
    float*  param;       /* [N][...] binary32, the trainer's tensor, updated in place; 4-byte aligned            */
    double* grad;        /* same shape, binary64: what gs_project_backward added to; 8-byte aligned                */
    float*  exp_avg;     /* same shape, binary32, updated in place                                               */
    float*  exp_avg_sq;  /* same shape, binary32, updated in place                                               */
    double  lr;
} gs_adam_group;         /* all four pointers NULL: the group is not stepped and the scene keeps what it holds   */
typedef struct {
    gs_adam_group means, log_scales, quats, opacity_logits, sh_dc, sh_rest;   /* row shapes as gs_device_arrays */
    uint32_t sh_rest_coeffs;        /* 0, 3, 8 or 15: sh_rest is [N][sh_rest_coeffs][3]; higher bands keep their bits */
    const uint8_t* mask;            /* [N] by scene id, nonzero = step this Gaussian; NULL = every Gaussian */
    double beta1, beta2, eps;
    double bias_correction1, bias_correction2;   /* 1 - beta^t, computed by the caller */
    int zero_grads;                 /* nonzero: the gradient rows that were consumed are set to +0.0 */
} gs_adam_step;
int gs_scene_adam_step(gs_scene* s, const gs_adam_step* a, void* stream);

/* ---- adaptive density control: the statistic, the decision and the compaction of a trainer's model, on the device ----------
 * What a 3DGS trainer does every hundred iterations -- clone the small Gaussians with a large screen-space gradient, split the
 * large ones, prune the transparent and the oversized -- over the six PLY-domain arrays of gs_device_arrays and the twelve
 * moment arrays of gs_scene_adam_step.  Three calls (gs_densify.hip); the new scene is then gs_scene_from_device_arrays of the
 * new arrays, with a new renderer.  No reference counterpart.  The unit is built with -ffp-contract=off: every operation below
 * is rounded on its own, in the order written, and THE CONTRACT OF ALL THREE CALLS IS A BIT PATTERN
 * (tests/densify_reference.py restates them in numpy).  INTEGRATION.md, 3l.
 *
 * 1. THE STATISTIC of the LAST frame, for every Gaussian id with stage("tiles")[id] != 0, with (gx, gy) = d_uv[id] -- the row
 * gs_blend_backward summed -- and W, H the width and height of that frame; binary64:
 *     grad_sum[id]   += sqrt(((gx * (W / 2)) * (gx * (W / 2))) + ((gy * (H / 2)) * (gy * (H / 2))))      W / 2, H / 2 exact
 *     count[id]      += 1
 *     max_radius[id]  = max(max_radius[id], stage("radius")[id])       binary32; the new value is taken where it is GREATER
 * The norm is that of the Inria trainer's viewspace_point_tensor.grad, whose dL_dmean2D carries the same 0.5 W and 0.5 H (its
 * screen position is in NDC): the customary threshold 2e-4 means here what it means there.  One lane per Gaussian, no atomics:
 * the same bits every call.  An invisible Gaussian's three elements are neither read nor written.  Scene ids, inputs and the
 * contents of the three arrays COMPLETE before the call, the renderer's own NON-BLOCKING stream, the synchronisation (queued
 * frames retire, an overflowed frame is re-run, the call returns when the arrays are written), "no frame rendered yet" and
 * the behaviour after a refused or failed gs_render: all as gs_visible_mask states them.
 * GS_ERR_INVALID, checked before any device is touched: r or s NULL; a NULL member; d_uv or grad_sum not 8-byte aligned, count
 * or max_radius not 4-byte aligned (judged by their values alone). */
typedef struct {
    const double* d_uv;    /* [N][2]  gs_blend_backward's sum for the last frame                           */
    double*   grad_sum;    /* [N]     ADDED to                                                              */
    uint32_t* count;       /* [N]     frames that saw the Gaussian, incremented                             */
    float*    max_radius;  /* [N]     the largest screen radius (pixels) any of those frames gave it         */
} gs_densify_stats;
int gs_accumulate_densify_stats(gs_renderer* r, const gs_densify_stats* s);

/* 2. THE DECISION, per parent i of a model of n rows.  With ls, logit, (grad_sum, count, max_radius) its rows:
 *     avg   = count != 0 ? grad_sum / (double)count : 0.0                  binary64; grad_sum is not read where count == 0
 *     sg_k  = gs_scene_from_device_arrays' binary32 activation of ls_k (libm's expf restated), k = 0, 1, 2
 *     s     = sg_0;  if (sg_1 > s) s = sg_1;  if (sg_2 > s) s = sg_2;      converted exactly to binary64
 *     o     = 1.0f / (1.0f + expf(-logit))                                 the same ingest's binary32, converted exactly
 *     grow  = avg >= grad_threshold
 *     clone = grow && s <= dense_extent        split = grow && s > dense_extent        keep otherwise
 * (a NaN compares false everywhere: a NaN average keeps, a NaN s neither clones nor splits, a NaN is never pruned).
 * THE SEMANTICS are the sequence trainers run: append one copy of every clone; append two children of every split and remove
 * the split parent; then prune over the EXTENDED set, whose statistics are zero for the appended rows (gsplat's default
 * strategy).  A row is pruned where its o < min_opacity, or max_screen_radius > 0 and its own max_radius > max_screen_radius
 * (only an original has a radius), or max_world_scale > 0 and its own s > max_world_scale -- for a split child the s of its NEW
 * log-scales (below).  A clone's copy shares o and s with its original; the two children of a split share o and their new s:
 * THEY SHARE THEIR PRUNE DECISION, so a split parent yields 0 or 2 rows, a cloned one 0, 1 (the copy, where only the radius
 * pruned the original) or 2, a kept one 0 or 1.
 *     row_offset[0 .. n]   = the exclusive prefix sum of those yields              scratch[0 .. n]
 *     noise_offset[0 .. n] = ... of "is a split parent whose children survive"    scratch[n + 1 .. 2 n + 1]
 * *n_out = row_offset[n] and *n_noise = noise_offset[n].  The scan is deterministic: a workgroup per GS_DENSIFY_PARTITION
 * parents reduces, one workgroup scans the partitions' sums in turns of 256 with a carry, a workgroup per partition scans its
 * own parents from its base (integers: the result has one value).  A model that would grow beyond 2^31 - 1 rows is refused
 * with GS_ERR_INVALID after the scan (the scratch is then written, nothing else is).
 * stream: a hipStream_t (NULL: the default stream); the work is enqueued on it behind what the caller has enqueued there and
 * the call returns after synchronising it.  All pointers are device pointers on `device`.  n == 0: success, both counts 0,
 * nothing is launched and the scratch is not touched.
 * GS_ERR_INVALID, checked before any device is touched: in, n_out or n_noise NULL; n >= 2^31; with n != 0: a NULL parameter
 * array (sh_rest only with sh_rest_coeffs != 0), statistic array or scratch; sh_rest_coeffs not in {0, 3, 8, 15}; a float or
 * uint32 pointer that is not 4-byte aligned, grad_sum not 8-byte aligned; a rule member that is NaN. */
#define GS_DENSIFY_PARTITION 2048u   /* parents per workgroup of the plan's scan */
#define GS_DENSIFY_BLOCK 256u        /* parents per workgroup of the apply     */
#define GS_DENSIFY_LOG_1_6 0x1.e148a1a2726cep-2   /* the binary64 nearest log(1.6) */
typedef struct {
    double grad_threshold;     /* on the average screen-space gradient norm (customarily 2e-4)             */
    double dense_extent;       /* percent_dense * scene extent: at most this large clones, larger splits   */
    double min_opacity;        /* prune below                                                              */
    double max_screen_radius;  /* prune above, pixels; <= 0: off                                           */
    double max_world_scale;    /* prune above; <= 0: off                                                   */
} gs_densify_rule;
typedef struct {
    gs_device_arrays params;     /* the model, n rows each                                                 */
    const double*   grad_sum;    /* [n] the three arrays gs_accumulate_densify_stats keeps                 */
    const uint32_t* count;
    const float*    max_radius;
    gs_densify_rule rule;
    uint32_t* scratch;           /* [2 (n + 1)] written by the plan, read by the apply                     */
} gs_densify_input;
int gs_densify_plan(const gs_densify_input* in, uint64_t n, int device, void* stream, uint64_t* n_out, uint64_t* n_noise);

/* 3. THE COMPACTION: the new model and its Adam moments from the old ones and the plan's two offset arrays.  Output rows are
 * ordered BY PARENT id, a parent's survivors adjacent, the original before its copy, child 0 before child 1 (trainers append:
 * survivors, then clones, then splits; parent order keeps ids spatially coherent, which k_adam_step's early exit and the
 * scene's Morton read order profit from).  Each output row:
 *   - a kept original, a clone's original: every parameter and both moments are copied bit for bit;
 *   - a clone's copy: parameters copied bit for bit, moments +0.0;
 *   - child c in {0, 1} of a split parent with ordinal j = noise_offset[i]: quats, opacity_logits, sh_dc, sh_rest copied,
 *     moments +0.0, and with t = noise[j][c] (binary32 -> binary64 exactly), all binary64:
 *         ls'_k = fl32(ls_k - GS_DENSIFY_LOG_1_6)
 *         (w, x, y, z) = q_e * inv, e = 0..3, binary32: inv = 1.0f / sqrtf((q_0 q_0 + q_1 q_1) + (q_2 q_2 + q_3 q_3)), the
 *                        ingest's normalisation; converted exactly
 *         R00 = 1 - 2 ((y y) + (z z))   R01 = 2 ((x y) - (w z))       R02 = 2 ((x z) + (w y))
 *         R10 = 2 ((x y) + (w z))       R11 = 1 - 2 ((x x) + (z z))   R12 = 2 ((y z) - (w x))
 *         R20 = 2 ((x z) - (w y))       R21 = 2 ((y z) + (w x))       R22 = 1 - 2 ((x x) + (y y))
 *         d_k = sg_k * t_k              (exact: two binary32 factors)
 *         m'_r = fl32(m_r + (((R_r0 * d_0) + (R_r1 * d_1)) + (R_r2 * d_2)))
 *     The kernel holds no random number generator: the result is a pure function of its inputs.
 * A NaN in a parent's statistic or parameters reaches that parent's rows only.  The inputs keep their bits.
 * A moment pair of a group may be NULL (both in, both out): that group has no moments to carry.  Every output array has n_out
 * rows and must not overlap an input.  n_out and n_noise are the plan's: the call reads row_offset[n] and noise_offset[n] back
 * and refuses with GS_ERR_INVALID, before anything is written, when they differ.  n_out == 0 or n == 0: success, nothing is
 * launched.  stream and synchronisation: as gs_densify_plan.
 * GS_ERR_INVALID, checked before any device is touched: in or out NULL; everything gs_densify_plan refuses about `in` and n;
 * n_out > 2 n or >= 2^31, n_noise > n or 2 n_noise > n_out; noise NULL with n_noise != 0, or not 4-byte aligned; with
 * n_out != 0: a NULL output parameter array (sh_rest only with sh_rest_coeffs != 0), a group with some but not all of its four
 * moment pointers; one moment of an input or of an output pair without the other; moments of sh_rest with sh_rest_coeffs == 0;
 * the output's sh_rest_coeffs not the input's; a pointer that is not 4-byte aligned. */
typedef struct {
    const float* exp_avg[6];         /* in, [n][...]: means, log_scales, quats, opacity_logits, sh_dc, sh_rest; nullable */
    const float* exp_avg_sq[6];
    const float* noise;              /* [n_noise][2][3] standard-normal draws, the caller's                              */
    uint64_t n_noise, n_out;         /* what gs_densify_plan returned                                                   */
    gs_device_arrays_out params;     /* out, [n_out][...]; sh_rest_coeffs must equal the input's                         */
    float* out_exp_avg[6];           /* out, [n_out][...]: given exactly where the input pair is                         */
    float* out_exp_avg_sq[6];
} gs_densify_output;
int gs_densify_apply(const gs_densify_input* in, uint64_t n, const gs_densify_output* out, int device, void* stream);

/* ---- initialisation from a point cloud: the mean squared distance to the k nearest neighbours ---------------------------
 * What a 3DGS trainer derives a point's initial scale from (the Inria trainer's simple_knn.distCUDA2, k = 3).  Scene-less,
 * like gs_densify_plan; no reference counterpart (the reference has no training).  gs_knn.hip, gs_knn_rules.h.
 * THE QUANTITY, for points p[0 .. n), binary32 [n][3], every coordinate finite (a precondition: the C entry does not look;
 * non-finite coordinates give unspecified values, never an access outside the arrays), and 1 <= k <= GS_KNN_MAX_K.
 * Every operation is binary32, rounded on its own (the library is built with -ffp-contract=off):
 *     dx = fl(xi - xj), dy = fl(yi - yj), dz = fl(zi - zj)
 *     d2(i, j) = fl( fl( fl(dx dx) + fl(dy dy) ) + fl(dz dz) )              for every j != i, BY INDEX: a coincident point
 *                                                                            at another index counts, with distance 0
 *     ke = min(k, n - 1);  best[0] <= ... <= best[ke - 1] = the ke smallest of those values; a candidate replaces a kept
 *                          value only where d2 < kept, so a NaN is never kept, nor is a d2 that overflowed to +inf
 *                          (the slot then stays +inf, which is that value)
 *     mean_dist2[i] = fl( fl( ... fl(best[0] + best[1]) + ... + best[ke - 1]) / (float)ke ),   +0.0f where ke == 0
 *     dist2[i][0 .. k) = best, padded with +inf beyond ke
 * The ke smallest values of a multiset do not depend on the order they are met in: the result has exactly ONE value, and the
 * contract is a bit pattern, equal to the brute force over all pairs (tests/knn_reference.py), whatever the kernels do to
 * avoid it.  Neighbour IDS are not returned: among equal distances they would depend on the order of the search.
 * THE SEARCH: the points are ordered by a 30-bit Morton code over their bounding box (10 bits per axis; an axis without extent
 * is cell 0; four stable radix passes, ties in id order) and gathered in that order; every GS_KNN_BOX consecutive points
 * have a box (their min / max per axis).  A workgroup per query box, a lane per query point: it examines its own box, then the
 * other boxes outward from it in the sorted order (b - 1, b + 1, b - 2, b + 2, ...), and passes a box over when
 *     bound(A, B) > the largest best[k - 1] of the workgroup's lanes        (+inf while any lane has kept fewer than k)
 * THE BOUND uses d2's operations in d2's order.  Per axis g = max(fl(loB - hiA), 0, fl(loA - hiB)); then
 * fl(fl(fl(gx gx) + fl(gy gy)) + fl(gz gz)).  For a in A, b in B: where loB > hiA, b - a >= loB - hiA > 0 in the reals and
 * rounding is monotonic, so |fl(a - b)| >= g; where the intervals meet g = 0.  Squares of non-negatives, sums of non-negatives
 * and their roundings are monotonic, so the bound is <= d2(i, j) for EVERY member pair, and a box passed over holds no
 * candidate with d2 < kept for any lane.  (A lane additionally passes a staged box over by the same bound with A its own point.)
 * The walk order is fixed and nothing is atomic: two calls give the same bits in all three outputs.
 * box_visits[b] = the boxes the workgroup of query box b (sorted points [b GS_KNN_BOX, ...)) staged, its own included: how
 * much the bound saved, and a test's handle on it.  WORST CASE: all points coincident -- every code equal, every bound 0,
 * nothing passed over, n^2 pairs.  Not special-cased.
 * scratch: gs_knn_scratch_bytes(n) bytes of the caller's, on `device`, 16-byte aligned where possible (4 is enough); its
 * content afterwards is unspecified.  stream and synchronisation: as gs_densify_plan.  n == 0: success, nothing launched,
 * nothing touched.  The outputs must not overlap `points` or the scratch.
 * GS_ERR_INVALID, checked before any device is touched: points NULL with n != 0; n >= 2^31; k outside [1, GS_KNN_MAX_K];
 * all three outputs NULL; with n != 0, scratch NULL or scratch_bytes < gs_knn_scratch_bytes(n); a pointer that is not 4-byte
 * aligned (judged by its value alone). */
#define GS_KNN_MAX_K 8
#ifndef GS_KNN_BOX
#define GS_KNN_BOX 256u            /* sorted points per box = lanes per workgroup of the search */
#endif
uint64_t gs_knn_scratch_bytes(uint64_t n);      /* 0 for n == 0 */
int gs_knn_dist2(const float* points, uint64_t n, int k,
                 float* mean_dist2 /* [n], nullable */, float* dist2 /* [n][k], nullable */,
                 uint32_t* box_visits /* [ceil(n / GS_KNN_BOX)], nullable */,
                 void* scratch, uint64_t scratch_bytes, int device, void* stream);
/* Test hook (tests/test_gpu_expf.py): evaluate the blend's exp() implementations ON THE DEVICE over the binary32 values with
 * bit patterns [first_bits, first_bits + count) (the negative floats run from 0x80000000 = -0 to 0xFF800000 = -inf).
 * block_sums[j] = sum over block j of 2^20 consecutive patterns of  bits(expf(x)) * ((bits(x) * 0x9E3779B1) | 1)  mod 2^64,
 * expf = the kernels' restatement of glibc's expf (exp mode 2, with libm's underflow to 0 below -103.97): the host computes
 * the same sums with its libm and compares.  guard (nullable, 4 doubles): the measured premise of exp mode 3's guard --
 * [0] max over x in [-16, 0] of |v_exp_f32(fl(x log2e)) - expf(x)| / expf(x) - E1 |x|, [1] the same ratio's max over [-1, 0],
 * [2] the guard's E0 (must exceed [0] + 2^-23), [3] its E1. */
int gs_debug_expf_scan(int device, uint32_t first_bits, uint64_t count, uint64_t* block_sums, uint64_t blocks_capacity, double* guard);
/* Test hook (tests/test_gpu_device_arrays.py): the same checksums (block_sums[j] as defined above) of the exp() that
 * gs_scene_from_device_arrays activates scales and opacities with -- libm's expf on the whole domain: the function above
 * with glibc's overflow branch (x > 88.7228 -> +inf) in front -- so that the positive half is pinned on the device too. */
int gs_debug_activation_expf_scan(int device, uint32_t first_bits, uint64_t count, uint64_t* block_sums, uint64_t blocks_capacity);
/* Test hook (tests/test_gpu_antialiased.py): for every opacity with bit pattern in [first_bits, first_bits + count), compare ON
 * THE DEVICE the per-frame alpha cut of the antialiased mode with the load-time one (the full bisection); *mismatches = how
 * many differ, *first_mismatch = the lowest such pattern (0xFFFFFFFF if none). */
int gs_debug_alpha_cut_scan(int device, uint32_t first_bits, uint64_t count, uint64_t* mismatches, uint32_t* first_mismatch);
/* The hipStream_t the renderer enqueues on (for HIP-event timing by the caller). */
void* gs_renderer_stream(gs_renderer* r);

/* ---- multi-GPU: replicate the scene once, shard the camera poses (no per-frame collective) --------------------
 * One process per GPU.  Rank 0 calls gs_dist_unique_id and hands the 128 bytes to the other ranks out of band (a
 * file, a socket, MPI, torch.distributed ...); every rank calls gs_dist_create; the root loads the scene
 * (gs_scene_load_ply) and every rank calls gs_dist_broadcast_scene, which sends the Gaussian count and then the packed
 * scene blob with ONE ncclBroadcast over xGMI (RCCL, loaded on first use) and returns the rank's resident scene
 * (the root gets its own handle back; the others own a new scene with cov3D recomputed locally).  Pose i belongs
 * to rank i mod world.  No reference counterpart: the reference renders on one physical device
 * (VulkanContext.cpp:134-178, `-d`). */
#define GS_DIST_ID_BYTES 128
typedef struct gs_dist gs_dist;
int gs_dist_unique_id(uint8_t id[GS_DIST_ID_BYTES]);
int gs_dist_create(const uint8_t id[GS_DIST_ID_BYTES], int rank, int world, int device, gs_dist** out);
int gs_dist_rank(const gs_dist* d);
int gs_dist_world(const gs_dist* d);
uint64_t gs_dist_pose_count(const gs_dist* d, uint64_t poses);  /* how many of `poses` poses this rank renders */
int gs_dist_broadcast_scene(gs_dist* d, gs_scene* mine /* root only */, int root, gs_scene** out);
/* The same with flags.  The header message carries, beside the count, the scene's storage flags: a root scene quantised
 * with gs_scene_quantize_sh arrives quantised on every rank (rounded locally from the broadcast fp32 block), so that all
 * replicas render from the same coefficients.  GS_DIST_COPY_ON_ROOT: the root, too, receives into a NEW scene (out-of-place
 * broadcast from `mine`), which it owns beside `mine` -- every rank then runs the same receiving code. */
#define GS_DIST_COPY_ON_ROOT 1u
int gs_dist_broadcast_scene_ex(gs_dist* d, gs_scene* mine /* root only */, int root, unsigned flags, gs_scene** out);
/* Evidence that the collective saw every rank and that every rank holds the root's scene (collective: every rank calls it
 * after gs_dist_broadcast_scene): `ranks` = an ncclAllReduce(sum) of one per rank, `checksums_equal` = the ncclAllReduce min
 * and max of each rank's checksum of its replica (the sum of the blob's 32-bit patterns) coincide with this rank's,
 * `broadcast_ms` / `broadcast_bytes` = this rank's wall time and payload of its last scene broadcast. */
typedef struct {
    uint64_t ranks;            /* ranks that took part in the all-reduce (must equal world) */
    uint64_t world;
    uint64_t checksum;         /* of this rank's replica */
    uint64_t broadcast_bytes;
    double broadcast_ms;
    uint32_t checksums_equal;  /* 1: every rank's replica has this checksum */
    uint32_t rccl_version;     /* ncclGetVersion */
} gs_dist_report;
int gs_dist_verify(gs_dist* d, const gs_scene* scene, gs_dist_report* out);
void gs_dist_destroy(gs_dist* d);

#ifdef __cplusplus
}
#endif
#endif
