// gs_scene_host.cpp -- the scene object behind the gs_scene_* entry points of include/gs3d_hip.h: upload of
// GSScene::Vertex records into the blob (11 SoA planes + the SH block), the load-time passes (cov3D, alpha cuts, the
// optional copy in spatial order), downloads and SH quantisation.  Replaces GSScene::load's buffer creation and
// GSScene::precomputeCov3D (GSScene.cpp:26-97, 157-184).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>

#include "gs_internal.h"
#include "gs_sh_rotation.h"

using namespace gs_host;

// GSScene::precomputeCov3D, GSScene.cpp:157-184
void gs_scene::finish_load() {
    cov3d.alloc(6 * n);
    if (reinterpret_cast<uintptr_t>(blob) % 64 != 0)
        throw Error(GS_ERR_INVALID, "the scene blob must be 64-byte aligned (SH blocks are read as 16-byte vectors)");
    // best effort: the copy is an optimisation (a second blob in HBM, a host-side sort); if any of its allocations fails the
    // scene simply renders from the blob as loaded (advisor, round 4)
    try {
        make_spatial_copy();
    } catch (const std::bad_alloc&) {
        drop_spatial_copy();
    } catch (const Error& e) {
        if (e.code != GS_ERR_NOMEM) throw;
        drop_spatial_copy();
    }
    gs::launch_cov3d(render_blob(), cov3d.p, static_cast<uint32_t>(n), static_cast<uint32_t>(gs::blob_stride(n)), 0, static_cast<uint32_t>(n), nullptr);
    acut.alloc(n);
    DevBuf<uint32_t> beyond;
    beyond.alloc(1);
    HIP_CHECK(hipMemset(beyond.p, 0, sizeof(uint32_t)));
    gs::launch_alpha_cut(render_blob(), acut.p, static_cast<uint32_t>(n), static_cast<uint32_t>(gs::blob_stride(n)), beyond.p, nullptr);
    HIP_CHECK(hipGetLastError());
    uint32_t flag = 0;
    HIP_CHECK(hipMemcpy(&flag, beyond.p, sizeof flag, hipMemcpyDeviceToHost));  // (synchronises)
    unit_opacity = flag == 0;
}

void gs_scene::drop_spatial_copy() {
    (void)hipGetLastError();  // (a failed hipMalloc leaves its error behind)
    perm.release();
    spatial_blob.release();
    std::fprintf(stderr, "[gs3d] no memory for the scene's copy in spatial order: rendering from the blob as loaded\n");
}
// Spatial order: Morton code of the position (21 bits per axis over the scene's bounding box), ties by id (gs_host_math.h: spatial_order).
void gs_scene::make_spatial_copy() {
    uint64_t min_n = 1ull << 19;  // (4 Mi until the one-pass level 1, which needs this order: DESIGN.md section 10)
    if (const char* e = std::getenv("GS_SPATIAL_MIN")) min_n = std::strtoull(e, nullptr, 10);
    if (n == 0 || n < min_n) return;
    const size_t st = gs::blob_stride(n);
    std::vector<float> pos(3 * n);
    for (int k = 0; k < 3; ++k)
        HIP_CHECK(hipMemcpy(pos.data() + static_cast<size_t>(k) * n, blob + static_cast<size_t>(gs::P_POS + k) * st, n * sizeof(float), hipMemcpyDeviceToHost));
    const float* const planes[3] = {pos.data(), pos.data() + n, pos.data() + 2 * n};
    const std::vector<uint32_t> order = gs::host::spatial_order(planes, n);
    perm.alloc(n);
    HIP_CHECK(hipMemcpy(perm.p, order.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
    spatial_blob.alloc(gs::blob_floats(n));
    gs::launch_permute_blob(blob, perm.p, spatial_blob.p, static_cast<uint32_t>(n), static_cast<uint32_t>(st), nullptr);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(nullptr));
}

namespace gs_host {

void quantize_sh(gs_scene* s) {  // gs_scene_quantize_sh; also run on the receiving ranks of a quantised scene's broadcast
    if (s->sh_half) return;
    HIP_CHECK(hipSetDevice(s->device));
    s->sh16.alloc(48 * static_cast<size_t>(s->n));
    gs::launch_sh_to_half(s->render_blob(), s->sh16.p, static_cast<uint32_t>(gs::blob_stride(s->n)), 0, static_cast<uint32_t>(s->n), nullptr);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(nullptr));
    s->sh_half = true;  // read when a frame is enqueued: frames already in flight keep reading the fp32 block, which stays
}

void upload_vertices(gs_scene* s, const float* vertices, uint64_t n) {
    // AoS GSScene::Vertex[n] -> blob: 11 SoA planes (pos3, scale3, rot4, opacity) + AoS SH block (48 per Gaussian)
    if (n >= kMaxGaussians) throw Error(GS_ERR_INVALID, "too many Gaussians (limit 2^31)");
    s->n = n;
    const size_t st = gs::blob_stride(n);
    std::vector<float> planes(gs::blob_floats(n));
    parallel_for(n, [&](uint64_t lo, uint64_t hi) {
        for (uint64_t i = lo; i < hi; ++i) {
            const float* v = vertices + i * gs::host::kVertexFloats;
            for (int k = 0; k < 3; ++k) planes[(gs::P_POS + k) * st + i] = v[k];
            for (int k = 0; k < 3; ++k) planes[(gs::P_SCALE + k) * st + i] = v[4 + k];
            for (int k = 0; k < 4; ++k) planes[(gs::P_ROT + k) * st + i] = v[8 + k];
            planes[static_cast<size_t>(gs::P_OPACITY) * st + i] = v[7];
            std::memcpy(&planes[static_cast<size_t>(gs::P_SH) * st + i * 48], v + 12, 48 * sizeof(float));
        }
    });
    s->owned_blob.alloc(planes.size());
    s->blob = s->owned_blob.p;
    if (n) HIP_CHECK(hipMemcpy(s->blob, planes.data(), planes.size() * sizeof(float), hipMemcpyHostToDevice));
    s->finish_load();
}

void activate_and_upload(gs_scene* s, const float* records, uint64_t n) {
    std::vector<float> verts(static_cast<size_t>(n) * gs::host::kVertexFloats);
    parallel_for(n, [&](uint64_t lo, uint64_t hi) {
        for (uint64_t i = lo; i < hi; ++i)
            gs::host::activate_record(records + i * gs::host::kRecordFloats, verts.data() + i * gs::host::kVertexFloats);
    });
    upload_vertices(s, verts.data(), n);
}

// What gs_scene_from_device_arrays / gs_scene_update_from_device_arrays refuse before any device is touched.
// `build`: every member is required (sh_rest only with sh_rest_coeffs != 0); otherwise a null member means "keep".
void check_device_arrays(const gs_device_arrays* a, uint64_t rows, bool build) {
    if (!a) throw Error(GS_ERR_INVALID, "null argument");
    const uint32_t k = a->sh_rest_coeffs;
    if (k != 0 && k != 3 && k != 8 && k != 15) throw Error(GS_ERR_INVALID, "sh_rest_coeffs must be 0, 3, 8 or 15 (SH degree 0..3)");
    const struct {
        const float* p;
        const char* name;
        bool required;
    } members[6] = {{a->means, "means", true},   {a->log_scales, "log_scales", true}, {a->quats, "quats", true}, {a->opacity_logits, "opacity_logits", true},
                    {a->sh_dc, "sh_dc", true}, {a->sh_rest, "sh_rest", k != 0}};
    for (const auto& m : members) {
        if (build && m.required && !m.p && rows) throw Error(GS_ERR_INVALID, std::string("device array `") + m.name + "` is null");
        if (reinterpret_cast<uintptr_t>(m.p) % 4 != 0) throw Error(GS_ERR_INVALID, std::string("device array `") + m.name + "` is not 4-byte aligned");
    }
}

// What is derived from the blob's planes, redone after they were rewritten in place (the ingest of an update, the optimiser's
// step) -- whole planes, into the buffers the scene's renderers already hold -- on `stream`, which is synchronised at the end.
static void redo_derived(gs_scene* s, bool shape, bool sh, bool opacity, hipStream_t stream) {
    const uint32_t n = static_cast<uint32_t>(s->n), st = static_cast<uint32_t>(gs::blob_stride(s->n));
    if (s->spatial_blob.p) gs::launch_permute_blob(s->blob, s->perm.p, s->spatial_blob.p, n, st, stream);  // the order stays
    if (shape) gs::launch_cov3d(s->render_blob(), s->cov3d.p, n, st, 0, n, stream);
    if (s->sh_half && sh) gs::launch_sh_to_half(s->render_blob(), s->sh16.p, st, 0, n, stream);
    if (opacity) {
        DevBuf<uint32_t> beyond;
        beyond.alloc(1);
        HIP_CHECK(hipMemsetAsync(beyond.p, 0, sizeof(uint32_t), stream));
        gs::launch_alpha_cut(s->render_blob(), s->acut.p, n, st, beyond.p, stream);
        HIP_CHECK(hipGetLastError());
        uint32_t flag = 0;
        HIP_CHECK(hipMemcpyAsync(&flag, beyond.p, sizeof flag, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        s->unit_opacity = flag == 0;
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(stream));
}

// gs_scene_update_from_device_arrays: the ingest over the range, then whatever is derived from the members that changed.
void update_from_device_arrays(gs_scene* s, const gs_device_arrays& a, uint64_t first, uint64_t count, hipStream_t stream) {
    HIP_CHECK(hipSetDevice(s->device));
    const uint32_t st = static_cast<uint32_t>(gs::blob_stride(s->n));
    gs_device_arrays in = a;
    if (!in.sh_rest) in.sh_rest_coeffs = 0;
    gs::launch_ingest_arrays(in, s->blob, st, static_cast<uint32_t>(first), static_cast<uint32_t>(count), in.sh_rest != nullptr, stream);
    redo_derived(s, a.log_scales || a.quats, a.sh_dc || a.sh_rest, a.opacity_logits != nullptr, stream);
}

// What gs_scene_adam_step refuses before any device is touched; returns whether any group is given.
bool check_adam_step(const gs_adam_step* a) {
    if (!a) throw Error(GS_ERR_INVALID, "null argument");
    const uint32_t k = a->sh_rest_coeffs;
    if (k != 0 && k != 3 && k != 8 && k != 15) throw Error(GS_ERR_INVALID, "sh_rest_coeffs must be 0, 3, 8 or 15 (SH degree 0..3)");
    const struct {
        const gs_adam_group* g;
        const char* name;
    } groups[6] = {{&a->means, "means"}, {&a->log_scales, "log_scales"}, {&a->quats, "quats"}, {&a->opacity_logits, "opacity_logits"},
                   {&a->sh_dc, "sh_dc"}, {&a->sh_rest, "sh_rest"}};
    bool any = false;
    for (const auto& m : groups) {
        const gs_adam_group& g = *m.g;
        const int given = (g.param != nullptr) + (g.grad != nullptr) + (g.exp_avg != nullptr) + (g.exp_avg_sq != nullptr);
        if (given == 0) continue;
        const std::string name = std::string("group `") + m.name + "`";
        if (given != 4) throw Error(GS_ERR_INVALID, name + " has some but not all of param, grad, exp_avg, exp_avg_sq");
        for (const float* p : {g.param, g.exp_avg, g.exp_avg_sq})
            if (reinterpret_cast<uintptr_t>(p) % 4 != 0) throw Error(GS_ERR_INVALID, name + ": param, exp_avg and exp_avg_sq must be 4-byte aligned");
        if (reinterpret_cast<uintptr_t>(g.grad) % 8 != 0) throw Error(GS_ERR_INVALID, name + ": grad must be 8-byte aligned");
        if (!(std::isfinite(g.lr) && g.lr >= 0.0)) throw Error(GS_ERR_INVALID, name + ": lr must be finite and >= 0");
        any = true;
    }
    if (a->sh_rest.param && k == 0) throw Error(GS_ERR_INVALID, "group `sh_rest` is given with sh_rest_coeffs == 0");
    if (!(a->beta1 >= 0.0 && a->beta1 < 1.0) || !(a->beta2 >= 0.0 && a->beta2 < 1.0)) throw Error(GS_ERR_INVALID, "beta1 and beta2 must lie in [0, 1)");
    if (!(std::isfinite(a->eps) && a->eps >= 0.0)) throw Error(GS_ERR_INVALID, "eps must be finite and >= 0");
    if (!(a->bias_correction1 > 0.0 && a->bias_correction1 <= 1.0) || !(a->bias_correction2 > 0.0 && a->bias_correction2 <= 1.0))
        throw Error(GS_ERR_INVALID, "the bias corrections must lie in (0, 1]");
    return any;
}

// gs_scene_adam_step: the step over the whole scene (k_adam_step leaves the workgroups of unmasked Gaussians at once), then
// whatever is derived from the groups that were stepped, as an update of those members would redo it.
void adam_step(gs_scene* s, const gs_adam_step& a, hipStream_t stream) {
    HIP_CHECK(hipSetDevice(s->device));
    gs::AdamStep k{};
    const gs_adam_group* from[6] = {&a.means, &a.log_scales, &a.quats, &a.opacity_logits, &a.sh_dc, &a.sh_rest};
    gs::AdamGroup* to[6] = {&k.means, &k.log_scales, &k.quats, &k.opacity_logits, &k.sh_dc, &k.sh_rest};
    for (int i = 0; i < 6; ++i) *to[i] = gs::AdamGroup{from[i]->param, from[i]->grad, from[i]->exp_avg, from[i]->exp_avg_sq, from[i]->lr / a.bias_correction1};
    k.sh_rest_coeffs = a.sh_rest_coeffs;
    k.mask = a.mask;
    k.beta1 = a.beta1, k.beta2 = a.beta2, k.one_minus_beta1 = 1.0 - a.beta1, k.one_minus_beta2 = 1.0 - a.beta2;
    k.sqrt_bc2 = std::sqrt(a.bias_correction2);
    k.eps = a.eps;
    k.zero_grads = a.zero_grads != 0;
    gs::launch_adam_step(k, s->blob, static_cast<uint32_t>(gs::blob_stride(s->n)), static_cast<uint32_t>(s->n), stream);
    redo_derived(s, a.log_scales.param || a.quats.param, a.sh_dc.param || a.sh_rest.param, a.opacity_logits.param != nullptr, stream);
}

// gs_scene_transform: the kernel over the range, then what is derived from scales, rotations and SH -- over the range alone
// when the frames read the blob itself, whole planes when they read the copy in spatial order (a range of the scene is
// scattered there) -- all on `stream`, which is synchronised at the end.  Opacities stay, so do the alpha cuts.
void transform_scene(gs_scene* s, const gs_transform& t, uint64_t first, uint64_t count, hipStream_t stream) {
    HIP_CHECK(hipSetDevice(s->device));
    const ShRotation r = sh_rotation(t);
    gs::SceneTransform x;
    std::memcpy(x.R, r.R, sizeof x.R);
    std::memcpy(x.t, t.translation, sizeof x.t);
    x.s = t.scale;
    std::memcpy(x.q, r.q, sizeof x.q);
    std::memcpy(x.M, r.M, sizeof x.M);
    const uint32_t n = static_cast<uint32_t>(s->n), st = static_cast<uint32_t>(gs::blob_stride(s->n));
    uint32_t f = static_cast<uint32_t>(first), c = static_cast<uint32_t>(count);
    gs::launch_scene_transform(x, s->blob, st, f, c, stream);
    if (s->spatial_blob.p) {
        gs::launch_permute_blob(s->blob, s->perm.p, s->spatial_blob.p, n, st, stream);  // the order stays
        f = 0, c = n;
    }
    gs::launch_cov3d(s->render_blob(), s->cov3d.p, n, st, f, c, stream);
    if (s->sh_half) gs::launch_sh_to_half(s->render_blob(), s->sh16.p, st, f, c, stream);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(stream));
}

// What gs_scene_to_device_arrays refuses before any device is touched (the twin of check_device_arrays; every member is optional).
void check_device_arrays_out(const gs_device_arrays_out* a) {
    if (!a) throw Error(GS_ERR_INVALID, "null argument");
    const uint32_t k = a->sh_rest_coeffs;
    if (k != 0 && k != 3 && k != 8 && k != 15) throw Error(GS_ERR_INVALID, "sh_rest_coeffs must be 0, 3, 8 or 15 (SH degree 0..3)");
    const struct {
        const float* p;
        const char* name;
    } members[6] = {{a->means, "means"}, {a->log_scales, "log_scales"}, {a->quats, "quats"}, {a->opacity_logits, "opacity_logits"},
                    {a->sh_dc, "sh_dc"}, {a->sh_rest, "sh_rest"}};
    for (const auto& m : members)
        if (reinterpret_cast<uintptr_t>(m.p) % 4 != 0) throw Error(GS_ERR_INVALID, std::string("device array `") + m.name + "` is not 4-byte aligned");
}

// What gs_densify_plan and gs_densify_apply refuse about the model, its statistics and the rule before any device is touched.
void check_densify_input(const gs_densify_input* in, uint64_t n) {
    if (!in) throw Error(GS_ERR_INVALID, "null argument");
    if (n >= kMaxGaussians) throw Error(GS_ERR_INVALID, "too many Gaussians (limit 2^31)");
    check_device_arrays(&in->params, n, true);
    if (n && (!in->grad_sum || !in->count || !in->max_radius)) throw Error(GS_ERR_INVALID, "null statistic: grad_sum, count and max_radius are all required");
    if (n && !in->scratch) throw Error(GS_ERR_INVALID, "null scratch: 2 (n + 1) uint32 are required");
    if (reinterpret_cast<uintptr_t>(in->grad_sum) % 8 != 0) throw Error(GS_ERR_INVALID, "grad_sum is not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(in->count) % 4 != 0) throw Error(GS_ERR_INVALID, "count is not 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(in->max_radius) % 4 != 0) throw Error(GS_ERR_INVALID, "max_radius is not 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(in->scratch) % 4 != 0) throw Error(GS_ERR_INVALID, "scratch is not 4-byte aligned");
    const gs_densify_rule& r = in->rule;
    const struct {
        double v;
        const char* name;
    } members[5] = {{r.grad_threshold, "grad_threshold"}, {r.dense_extent, "dense_extent"}, {r.min_opacity, "min_opacity"},
                    {r.max_screen_radius, "max_screen_radius"}, {r.max_world_scale, "max_world_scale"}};
    for (const auto& m : members)
        if (std::isnan(m.v)) throw Error(GS_ERR_INVALID, std::string("rule member `") + m.name + "` is NaN");
}

// What gs_densify_apply refuses about its outputs before any device is touched.
void check_densify_output(const gs_densify_input* in, uint64_t n, const gs_densify_output* out) {
    if (!out) throw Error(GS_ERR_INVALID, "null argument");
    if (out->n_out > 2 * n || out->n_out >= kMaxGaussians) throw Error(GS_ERR_INVALID, "n_out is not a plan's: more than 2 n rows, or 2^31 and beyond");
    if (out->n_noise > n || 2 * out->n_noise > out->n_out) throw Error(GS_ERR_INVALID, "n_noise is not a plan's: more than n, or more than n_out / 2");
    if (out->n_noise && !out->noise) throw Error(GS_ERR_INVALID, "noise is null with n_noise != 0");
    if (reinterpret_cast<uintptr_t>(out->noise) % 4 != 0) throw Error(GS_ERR_INVALID, "noise is not 4-byte aligned");
    check_device_arrays_out(&out->params);
    if (out->params.sh_rest_coeffs != in->params.sh_rest_coeffs) throw Error(GS_ERR_INVALID, "the output's sh_rest_coeffs is not the input's");
    const float* const params[6] = {out->params.means, out->params.log_scales, out->params.quats, out->params.opacity_logits, out->params.sh_dc, out->params.sh_rest};
    static const char* const names[6] = {"means", "log_scales", "quats", "opacity_logits", "sh_dc", "sh_rest"};
    for (int g = 0; g < 6; ++g) {
        const bool needed = g < 5 || in->params.sh_rest_coeffs != 0;
        if (out->n_out && needed && !params[g]) throw Error(GS_ERR_INVALID, std::string("output array `") + names[g] + "` is null");
        const int given = (out->exp_avg[g] != nullptr) + (out->exp_avg_sq[g] != nullptr);
        const int given_out = (out->out_exp_avg[g] != nullptr) + (out->out_exp_avg_sq[g] != nullptr);
        const std::string name = std::string("group `") + names[g] + "`";
        if (given == 1 || given_out == 1 || (out->n_out && given != given_out)) throw Error(GS_ERR_INVALID, name + " has some but not all of its four moment pointers");
        if (given && !needed) throw Error(GS_ERR_INVALID, name + " has moments with sh_rest_coeffs == 0");
        for (const float* p : {out->exp_avg[g], out->exp_avg_sq[g], static_cast<const float*>(out->out_exp_avg[g]), static_cast<const float*>(out->out_exp_avg_sq[g])})
            if (reinterpret_cast<uintptr_t>(p) % 4 != 0) throw Error(GS_ERR_INVALID, name + ": a moment pointer is not 4-byte aligned");
    }
}

void export_records_streamed(const gs_scene* s, uint64_t first, uint64_t count, const std::function<void(const float*, uint64_t)>& sink) {
    if (count == 0) return;
    HIP_CHECK(hipSetDevice(s->device));
    uint64_t chunk = 1ull << 18;
    if (const char* e = std::getenv("GS_EXPORT_CHUNK")) chunk = std::max<uint64_t>(1, std::strtoull(e, nullptr, 10));
    chunk = std::min(chunk, count);
    const size_t floats = static_cast<size_t>(chunk) * gs::host::kRecordFloats;
    const uint32_t st = static_cast<uint32_t>(gs::blob_stride(s->n));
    DevBuf<float> dev[2];
    float* pinned[2] = {nullptr, nullptr};
    hipEvent_t arrived[2] = {nullptr, nullptr};
    hipStream_t down = nullptr;
    auto cleanup = [&] {
        if (down) (void)hipStreamSynchronize(down);  // (nothing may still be writing into what is freed)
        for (int k = 0; k < 2; ++k) {
            if (pinned[k]) (void)hipHostFree(pinned[k]);
            if (arrived[k]) (void)hipEventDestroy(arrived[k]);
        }
        if (down) (void)hipStreamDestroy(down);
    };
    try {
        HIP_CHECK(hipStreamCreateWithFlags(&down, hipStreamNonBlocking));
        for (int k = 0; k < 2; ++k) {
            dev[k].alloc(floats);
            HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&pinned[k]), floats * sizeof(float), hipHostMallocDefault));
            HIP_CHECK(hipEventCreateWithFlags(&arrived[k], hipEventDisableTiming));
        }
        const uint64_t chunks = (count + chunk - 1) / chunk;
        auto rows_of = [&](uint64_t c) { return std::min(chunk, count - c * chunk); };
        for (uint64_t c = 0; c <= chunks; ++c) {  // chunk c is enqueued, then chunk c - 1 consumed: its buffers are free again for c + 1
            if (c < chunks) {
                const uint64_t rows = rows_of(c);
                gs::launch_scene_export_records(dev[c & 1].p, s->blob, st, static_cast<uint32_t>(first + c * chunk), static_cast<uint32_t>(rows), down);
                HIP_CHECK(hipGetLastError());
                HIP_CHECK(hipMemcpyAsync(pinned[c & 1], dev[c & 1].p, static_cast<size_t>(rows) * gs::host::kRecordFloats * sizeof(float),
                                         hipMemcpyDeviceToHost, down));
                HIP_CHECK(hipEventRecord(arrived[c & 1], down));
            }
            if (c >= 1) {
                HIP_CHECK(hipEventSynchronize(arrived[(c - 1) & 1]));
                sink(pinned[(c - 1) & 1], rows_of(c - 1));
            }
        }
    } catch (...) {
        cleanup();
        throw;
    }
    cleanup();
}

}  // namespace gs_host

extern "C" {

int gs_deactivate_vertices(const float* vertices, uint64_t n, float* records) {
    return guarded([&] {
        if ((!vertices || !records) && n) throw Error(GS_ERR_INVALID, "null argument");
        parallel_for(n, [&](uint64_t lo, uint64_t hi) {
            for (uint64_t i = lo; i < hi; ++i)
                gs::host::deactivate_vertex(vertices + i * gs::host::kVertexFloats, records + i * gs::host::kRecordFloats);
        });
    });
}

int gs_scene_to_device_arrays(const gs_scene* s, const gs_device_arrays_out* a, uint64_t first, uint64_t count, void* stream) {
    return guarded([&] {
        check_device_arrays_out(a);
        if (!s) throw Error(GS_ERR_INVALID, "null argument");
        if (first > s->n || count > s->n - first) throw Error(GS_ERR_INVALID, "Gaussian range out of bounds");
        if (count == 0 || !(a->means || a->log_scales || a->quats || a->opacity_logits || a->sh_dc || (a->sh_rest && a->sh_rest_coeffs))) return;
        HIP_CHECK(hipSetDevice(s->device));
        const hipStream_t st = static_cast<hipStream_t>(stream);
        gs::launch_scene_export(*a, s->blob, static_cast<uint32_t>(gs::blob_stride(s->n)), static_cast<uint32_t>(first),
                                static_cast<uint32_t>(count), st);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(st));
    });
}

int gs_scene_download_records(const gs_scene* s, uint64_t first, uint64_t count, float* records) {
    return guarded([&] {
        if (!s || (!records && count)) throw Error(GS_ERR_INVALID, "null argument");
        if (first > s->n || count > s->n - first) throw Error(GS_ERR_INVALID, "Gaussian range out of bounds");
        float* out = records;
        export_records_streamed(s, first, count, [&](const float* rec, uint64_t rows) {
            std::memcpy(out, rec, static_cast<size_t>(rows) * gs::host::kRecordFloats * sizeof(float));
            out += rows * gs::host::kRecordFloats;
        });
    });
}

int gs_scene_transform(gs_scene* s, const gs_transform* t, uint64_t first, uint64_t count, void* stream) {
    return guarded([&] {
        if (const char* fault = transform_fault(t)) throw Error(GS_ERR_INVALID, fault);
        if (!s) throw Error(GS_ERR_INVALID, "null argument");
        if (first > s->n || count > s->n - first) throw Error(GS_ERR_INVALID, "Gaussian range out of bounds");
        if (count == 0) return;
        transform_scene(s, *t, first, count, static_cast<hipStream_t>(stream));
    });
}

int gs_transform_sh_matrices(const gs_transform* t, float out[83]) {
    return guarded([&] {
        if (const char* fault = transform_fault(t)) throw Error(GS_ERR_INVALID, fault);
        if (!out) throw Error(GS_ERR_INVALID, "null argument");
        const ShRotation r = sh_rotation(*t);
        std::memcpy(out, r.M, sizeof r.M);
    });
}

int gs_transform_camera(const gs_transform* t, const gs_camera* in, gs_camera* out) {
    return guarded([&] {
        if (const char* fault = transform_fault(t)) throw Error(GS_ERR_INVALID, fault);
        if (!in || !out) throw Error(GS_ERR_INVALID, "null argument");
        transform_camera(*t, *in, out);
    });
}

int gs_scene_from_device_arrays(const gs_device_arrays* a, uint64_t n, int device, void* stream, gs_scene** out) {
    return guarded([&] {
        if (!out) throw Error(GS_ERR_INVALID, "null argument");
        if (n >= kMaxGaussians) throw Error(GS_ERR_INVALID, "too many Gaussians (limit 2^31)");
        check_device_arrays(a, n, true);
        select_device(device);
        auto s = std::make_unique<gs_scene>();
        s->device = device;
        s->n = n;
        s->owned_blob.alloc(gs::blob_floats(n));
        s->blob = s->owned_blob.p;
        const hipStream_t st = static_cast<hipStream_t>(stream);
        // the planes' padding (up to 15 floats each) is part of the blob that gs_scene_blob hands out and gs_dist broadcasts: zero, as uploaded
        const size_t stride = gs::blob_stride(n);
        for (int p = 0; p < gs::P_SH && stride > n; ++p)
            HIP_CHECK(hipMemsetAsync(s->blob + p * stride + n, 0, (stride - n) * sizeof(float), st));
        gs::launch_ingest_arrays(*a, s->blob, static_cast<uint32_t>(stride), 0, static_cast<uint32_t>(n), true, st);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(st));
        s->finish_load();
        *out = s.release();
    });
}

int gs_scene_update_from_device_arrays(gs_scene* s, const gs_device_arrays* a, uint64_t first, uint64_t count, void* stream) {
    return guarded([&] {
        check_device_arrays(a, count, false);
        if (!s) throw Error(GS_ERR_INVALID, "null argument");
        if (first > s->n || count > s->n - first) throw Error(GS_ERR_INVALID, "Gaussian range out of bounds");
        if (count == 0 || !(a->means || a->log_scales || a->quats || a->opacity_logits || a->sh_dc || a->sh_rest)) return;
        update_from_device_arrays(s, *a, first, count, static_cast<hipStream_t>(stream));
    });
}

int gs_scene_adam_step(gs_scene* s, const gs_adam_step* a, void* stream) {
    return guarded([&] {
        const bool any = check_adam_step(a);
        if (!s) throw Error(GS_ERR_INVALID, "null argument");
        if (!any || s->n == 0) return;
        adam_step(s, *a, static_cast<hipStream_t>(stream));
    });
}

int gs_densify_plan(const gs_densify_input* in, uint64_t n, int device, void* stream, uint64_t* n_out, uint64_t* n_noise) {
    return guarded([&] {
        check_densify_input(in, n);
        if (!n_out || !n_noise) throw Error(GS_ERR_INVALID, "null argument");
        *n_out = *n_noise = 0;
        if (n == 0) return;
        select_device(device);
        const hipStream_t st = static_cast<hipStream_t>(stream);
        const uint32_t rows = static_cast<uint32_t>(n);
        DevBuf<uint32_t> parts;  // the partitions' sums: n / 1024 words
        parts.alloc(2 * gs::densify_partitions(rows));
        gs::launch_densify_plan(*in, rows, parts.p, st);
        HIP_CHECK(hipGetLastError());
        uint32_t totals[2] = {0, 0};
        HIP_CHECK(hipMemcpyAsync(&totals[0], in->scratch + n, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(&totals[1], in->scratch + 2 * n + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (totals[0] >= kMaxGaussians) throw Error(GS_ERR_INVALID, "the densified model would have more than 2^31 - 1 rows");
        *n_out = totals[0], *n_noise = totals[1];
    });
}

int gs_densify_apply(const gs_densify_input* in, uint64_t n, const gs_densify_output* out, int device, void* stream) {
    return guarded([&] {
        check_densify_input(in, n);
        check_densify_output(in, n, out);
        if (n == 0 || out->n_out == 0) return;
        select_device(device);
        const hipStream_t st = static_cast<hipStream_t>(stream);
        uint32_t totals[2] = {0, 0};
        HIP_CHECK(hipMemcpyAsync(&totals[0], in->scratch + n, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(&totals[1], in->scratch + 2 * n + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (totals[0] != out->n_out || totals[1] != out->n_noise)
            throw Error(GS_ERR_INVALID, "n_out / n_noise are not what the plan left in scratch: run gs_densify_plan on these inputs first");
        gs::launch_densify_apply(*in, static_cast<uint32_t>(n), *out, st);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(st));
    });
}

uint64_t gs_knn_scratch_bytes(uint64_t n) { return n == 0 || n >= kMaxGaussians ? 0 : gs::knn_scratch_bytes(n); }

int gs_knn_dist2(const float* points, uint64_t n, int k, float* mean_dist2, float* dist2, uint32_t* box_visits, void* scratch,
                 uint64_t scratch_bytes, int device, void* stream) {
    return guarded([&] {
        if (n >= kMaxGaussians) throw Error(GS_ERR_INVALID, "too many points (limit 2^31)");
        if (k < 1 || k > GS_KNN_MAX_K) throw Error(GS_ERR_INVALID, "k must be in [1, GS_KNN_MAX_K]");
        if (!mean_dist2 && !dist2 && !box_visits) throw Error(GS_ERR_INVALID, "no output: mean_dist2, dist2 and box_visits are all null");
        if (n && !points) throw Error(GS_ERR_INVALID, "null points");
        if (n && !scratch) throw Error(GS_ERR_INVALID, "null scratch: gs_knn_scratch_bytes(n) bytes are required");
        if (n && scratch_bytes < gs::knn_scratch_bytes(n)) throw Error(GS_ERR_INVALID, "scratch is smaller than gs_knn_scratch_bytes(n)");
        const struct {
            const void* p;
            const char* name;
        } members[5] = {{points, "points"}, {mean_dist2, "mean_dist2"}, {dist2, "dist2"}, {box_visits, "box_visits"}, {scratch, "scratch"}};
        for (const auto& m : members)
            if (reinterpret_cast<uintptr_t>(m.p) % 4 != 0) throw Error(GS_ERR_INVALID, std::string("`") + m.name + "` is not 4-byte aligned");
        if (n == 0) return;
        select_device(device);
        const hipStream_t st = static_cast<hipStream_t>(stream);
        const uint32_t rows = static_cast<uint32_t>(n);
        gs::launch_knn(points, rows, k, mean_dist2, dist2, box_visits, gs::knn_buffers(scratch, rows), st);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(st));
    });
}

int gs_activate_records(const float* records, uint64_t n, float* vertices) {
    return guarded([&] {
        if ((!records || !vertices) && n) throw Error(GS_ERR_INVALID, "null argument");
        parallel_for(n, [&](uint64_t lo, uint64_t hi) {
            for (uint64_t i = lo; i < hi; ++i)
                gs::host::activate_record(records + i * gs::host::kRecordFloats, vertices + i * gs::host::kVertexFloats);
        });
    });
}

int gs_scene_from_records(const float* records, uint64_t n, int device, gs_scene** out) {
    return guarded([&] {
        if ((!records && n) || !out) throw Error(GS_ERR_INVALID, "null argument");
        select_device(device);
        auto s = std::make_unique<gs_scene>();
        s->device = device;
        activate_and_upload(s.get(), records, n);
        *out = s.release();
    });
}

int gs_scene_from_vertices(const float* vertices, uint64_t n, int device, gs_scene** out) {
    return guarded([&] {
        if ((!vertices && n) || !out) throw Error(GS_ERR_INVALID, "null argument");
        select_device(device);
        auto s = std::make_unique<gs_scene>();
        s->device = device;
        upload_vertices(s.get(), vertices, n);
        *out = s.release();
    });
}

uint64_t gs_scene_blob_floats(uint64_t n) { return gs::blob_floats(n); }

int gs_scene_from_device_blob(float* d_blob, uint64_t n, int device, gs_scene** out) {
    return guarded([&] {
        if ((!d_blob && n) || !out) throw Error(GS_ERR_INVALID, "null argument");
        if (n >= kMaxGaussians) throw Error(GS_ERR_INVALID, "too many Gaussians (limit 2^31)");
        select_device(device);
        auto s = std::make_unique<gs_scene>();
        s->device = device;
        s->n = n;
        s->blob = d_blob;
        s->finish_load();
        *out = s.release();
    });
}

int gs_scene_blob(const gs_scene* s, float** d_blob, uint64_t* floats) {
    return guarded([&] {
        if (!s || !d_blob || !floats) throw Error(GS_ERR_INVALID, "null argument");
        *d_blob = s->blob;
        *floats = gs_scene_blob_floats(s->n);
    });
}

uint64_t gs_scene_num_vertices(const gs_scene* s) { return s ? s->n : 0; }

int gs_scene_quantize_sh(gs_scene* s) {
    return guarded([&] {
        if (!s) throw Error(GS_ERR_INVALID, "null argument");
        quantize_sh(s);
    });
}

int gs_scene_sh_bits(const gs_scene* s) { return s ? (s->sh_half ? 16 : 32) : 0; }

int gs_scene_download_vertex_range(const gs_scene* s, uint64_t first, uint64_t count, float* vertices) {
    return guarded([&] {
        if (!s || (!vertices && count)) throw Error(GS_ERR_INVALID, "null argument");
        if (first > s->n || count > s->n - first) throw Error(GS_ERR_INVALID, "vertex range out of bounds");
        HIP_CHECK(hipSetDevice(s->device));
        const size_t st = gs::blob_stride(s->n);
        std::vector<float> plane(count), sh(48 * static_cast<size_t>(count));
        auto fetch = [&](int p, int dst_slot) {
            if (count) HIP_CHECK(hipMemcpy(plane.data(), s->blob + static_cast<size_t>(p) * st + first, count * sizeof(float), hipMemcpyDeviceToHost));
            for (uint64_t i = 0; i < count; ++i) vertices[i * gs::host::kVertexFloats + dst_slot] = plane[i];
        };
        for (int k = 0; k < 3; ++k) fetch(gs::P_POS + k, k);
        for (uint64_t i = 0; i < count; ++i) vertices[i * gs::host::kVertexFloats + 3] = 1.0f;
        for (int k = 0; k < 3; ++k) fetch(gs::P_SCALE + k, 4 + k);
        fetch(gs::P_OPACITY, 7);
        for (int k = 0; k < 4; ++k) fetch(gs::P_ROT + k, 8 + k);
        if (count) HIP_CHECK(hipMemcpy(sh.data(), s->blob + static_cast<size_t>(gs::P_SH) * st + first * 48, sh.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < count; ++i) std::memcpy(vertices + i * gs::host::kVertexFloats + 12, sh.data() + i * 48, 48 * sizeof(float));
    });
}

int gs_scene_download_vertices(const gs_scene* s, float* vertices) {
    return guarded([&] {
        if (!s || (!vertices && s->n)) throw Error(GS_ERR_INVALID, "null argument");
        HIP_CHECK(hipSetDevice(s->device));
        const uint64_t n = s->n;
        const size_t st = gs::blob_stride(n);
        std::vector<float> planes(gs::blob_floats(n));
        if (n) HIP_CHECK(hipMemcpy(planes.data(), s->blob, planes.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < n; ++i) {
            float* v = vertices + i * gs::host::kVertexFloats;
            for (int k = 0; k < 3; ++k) v[k] = planes[(gs::P_POS + k) * st + i];
            v[3] = 1.0f;
            for (int k = 0; k < 3; ++k) v[4 + k] = planes[(gs::P_SCALE + k) * st + i];
            v[7] = planes[static_cast<size_t>(gs::P_OPACITY) * st + i];
            for (int k = 0; k < 4; ++k) v[8 + k] = planes[(gs::P_ROT + k) * st + i];
            for (int k = 0; k < 48; ++k) v[12 + k] = planes[static_cast<size_t>(gs::P_SH) * st + i * 48 + k];
        }
    });
}

int gs_scene_download_cov3d(const gs_scene* s, float* cov3d) {
    return guarded([&] {
        if (!s || (!cov3d && s->n)) throw Error(GS_ERR_INVALID, "null argument");
        HIP_CHECK(hipSetDevice(s->device));
        const uint64_t n = s->n;
        std::vector<float> planes(6 * static_cast<size_t>(n));
        if (n) HIP_CHECK(hipMemcpy(planes.data(), s->cov3d.p, planes.size() * sizeof(float), hipMemcpyDeviceToHost));
        std::vector<uint32_t> order;  // cov3D lives in the order the frame kernels read the scene in: back to the scene's own
        if (s->perm.p) {
            order.resize(n);
            HIP_CHECK(hipMemcpy(order.data(), s->perm.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
        }
        for (uint64_t i = 0; i < n; ++i)
            for (int k = 0; k < 6; ++k) cov3d[(order.empty() ? i : order[i]) * 6 + k] = planes[k * n + i];
    });
}

void gs_scene_destroy(gs_scene* s) { delete s; }

}  // extern "C"
