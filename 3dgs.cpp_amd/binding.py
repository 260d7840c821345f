"""ctypes binding of libgs3d_hip.so (include/gs3d_hip.h) for tests and bench.py.

Host-language note: the reference is a C++ library, so the host-side mirror of its API is C++
(csrc/host/, include/3dgs/).  This module is only the Python harness over the same C ABI: it adds
no arithmetic and never falls back to a CPU path -- if the HIP library or a GPU is missing, calls
raise GsError.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GS3D_HIP_LIB", os.path.join(_HERE, "libgs3d_hip.so"))  # override: instrumented builds

UNIFORMS_DT = np.dtype([("camera_position", "<f4", 4), ("proj_mat", "<f4", 16), ("view_mat", "<f4", 16),
                        ("width", "<u4"), ("height", "<u4"), ("tan_fovx", "<f4"), ("tan_fovy", "<f4")])
CAMERA_DT = np.dtype([("position", "<f4", 3), ("rotation", "<f4", 4), ("fov", "<f4"),
                      ("near_plane", "<f4"), ("far_plane", "<f4")])
VERTEX_FLOATS = 60
RECORD_FLOATS = 62
BLOB_PLANES = 59


# the device code of libgs3d_hip.so: one translation unit per stage + the shared device headers
KERNEL_SOURCES = ("gs_device.h", "gs_bin.h", "gs_tile_cull.h", "gs_scene.hip", "gs_preprocess.hip", "gs_radix.hip", "gs_bin_l1.hip", "gs_bin_l2.hip",
                  "gs_blend.hip", "gs_contrib.hip", "gs_features.hip", "gs_lift.hip", "gs_backward.hip", "gs_project_backward.hip", "gs_camera_backward.hip", "gs_loss.hip", "gs_optim.hip", "gs_densify.hip", "gs_knn.hip", "gs_knn_rules.h", "gs_project_chain.h",
                  "gs_wave_f64.h", "gs_kernels.h")


def library_source_hash():
    """sha256 over the KERNEL sources (comments and whitespace stripped) and the build flags libgs3d_hip.so is built from:
    ties a committed rocprofv3 counter file to the kernels it was collected on (bench.py refuses counters of other
    kernels; host-side or comment-only changes do not move a kernel's instruction or byte counts)."""
    import hashlib
    import re
    h = hashlib.sha256()
    for name in KERNEL_SOURCES + ("Makefile",):
        with open(os.path.join(_HERE, "csrc", name), "r") as f:
            text = f.read()
        if name != "Makefile":
            text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
            text = re.sub(r"//[^\n]*", " ", text)
        else:
            text = re.sub(r"#[^\n]*", " ", text)
        h.update(name.encode() + b"\0" + " ".join(text.split()).encode())
    return h.hexdigest()


STAGES = dict(tiles=(0, np.uint32), depth=(1, np.float32), radius=(2, np.float32), aabb=(3, np.uint16),
              conic_opacity=(4, np.float32), uv_rg=(5, np.float32), b=(6, np.float32),
              depth_order=(7, np.uint32), alpha_cut=(8, np.float32), sorted_tile=(11, np.uint32), sorted_gid=(12, np.uint32),
              ranges=(13, np.uint32), lists_raw=(14, np.uint32), ranges_raw=(15, np.uint32),
              lists_culled=(16, np.uint32), ranges_culled=(17, np.uint32))

# every symbol include/gs3d_hip.h declares
SYMBOLS = ["gs_last_error", "gs_device_count", "gs_read_ply", "gs_activate_records", "gs_scene_load_ply", "gs_scene_from_records",
           "gs_scene_from_vertices", "gs_scene_from_device_blob", "gs_scene_blob_floats", "gs_scene_blob",
           "gs_scene_from_device_arrays", "gs_scene_update_from_device_arrays", "gs_debug_activation_expf_scan",
           "gs_scene_transform", "gs_transform_sh_matrices", "gs_transform_camera",
           "gs_scene_num_vertices", "gs_scene_quantize_sh", "gs_scene_sh_bits", "gs_scene_download_vertex_range",
           "gs_scene_download_vertices", "gs_scene_download_cov3d",
           "gs_deactivate_vertices", "gs_write_ply", "gs_scene_to_device_arrays", "gs_scene_download_records", "gs_scene_save_ply",
           "gs_scene_destroy", "gs_renderer_create", "gs_renderer_destroy", "gs_camera_uniforms",
           "gs_render", "gs_render_host", "gs_synchronize", "gs_set_timing", "gs_set_frames_in_flight", "gs_set_sort_path", "gs_set_exp_mode", "gs_set_graph_mode", "gs_set_blend_lockstep", "gs_get_blend_lockstep", "gs_set_level1_fused", "gs_get_level1_fused", "gs_set_tile_cull", "gs_get_tile_cull", "gs_get_listed_instances", "gs_set_blend_contraction", "gs_set_antialiased", "gs_get_antialiased", "gs_get_timing_totals",
           "gs_get_frame_intervals", "gs_get_stats", "gs_poll_stats", "gs_debug_download", "gs_accumulate_contributions", "gs_blend_features", "gs_lift_pixels", "gs_blend_backward", "gs_project_backward", "gs_camera_backward", "gs_camera_uniforms_backward", "gs_photometric_loss", "gs_visible_mask", "gs_scene_adam_step", "gs_accumulate_densify_stats", "gs_densify_plan", "gs_densify_apply", "gs_knn_scratch_bytes", "gs_knn_dist2", "gs_debug_expf_scan", "gs_debug_alpha_cut_scan", "gs_renderer_stream",
           "gs_dist_unique_id", "gs_dist_create", "gs_dist_rank", "gs_dist_world", "gs_dist_pose_count",
           "gs_dist_broadcast_scene", "gs_dist_broadcast_scene_ex", "gs_dist_verify", "gs_dist_destroy"]


class FrameStats(C.Structure):
    _fields_ = [("num_gaussians", C.c_uint64), ("num_visible", C.c_uint64), ("num_instances", C.c_uint64),
                ("instance_capacity", C.c_uint64), ("ms_preprocess", C.c_float), ("ms_prefix_sum", C.c_float),
                ("ms_preprocess_sort", C.c_float), ("ms_sort", C.c_float), ("ms_tile_boundary", C.c_float),
                ("ms_render", C.c_float), ("ms_total", C.c_float), ("retries", C.c_uint32),
                ("num_bin_entries", C.c_uint32), ("max_bin_entries", C.c_uint32), ("sort_path", C.c_uint32),
                ("bin_tiles", C.c_uint32), ("sort_level", C.c_uint32), ("blend_redo", C.c_uint32), ("blend_resolved", C.c_uint32), ("pad_", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def debug_alpha_cut_scan(first_bits, count, device=0):
    """Test hook gs_debug_alpha_cut_scan: (mismatches, first mismatching pattern or None) of the antialiased mode's per-frame
    alpha cut against the load-time bisection, over the opacities with bit patterns [first_bits, first_bits + count)."""
    bad, first = C.c_uint64(0), C.c_uint32(0)
    _check(lib().gs_debug_alpha_cut_scan(C.c_int(device), C.c_uint32(first_bits), C.c_uint64(count), C.byref(bad), C.byref(first)))
    return int(bad.value), (None if bad.value == 0 else int(first.value))


def debug_expf_scan(first_bits, count, device=0):
    """Test hook gs_debug_expf_scan: (block checksums of the kernels' expf over the bit patterns, the guard's measured premise)."""
    blocks = (count + (1 << 20) - 1) >> 20
    sums = np.zeros(blocks, np.uint64)
    guard = np.zeros(4, np.float64)
    _check(lib().gs_debug_expf_scan(C.c_int(device), C.c_uint32(first_bits), C.c_uint64(count), _p(sums), C.c_uint64(blocks), _p(guard)))
    return sums, guard


def debug_activation_expf_scan(first_bits, count, device=0):
    """Test hook gs_debug_activation_expf_scan: block checksums (as debug_expf_scan forms them) of the exp() that the device-array
    ingest activates scales and opacities with, over the bit patterns [first_bits, first_bits + count)."""
    blocks = (count + (1 << 20) - 1) >> 20
    sums = np.zeros(blocks, np.uint64)
    _check(lib().gs_debug_activation_expf_scan(C.c_int(device), C.c_uint32(first_bits), C.c_uint64(count), _p(sums), C.c_uint64(blocks)))
    return sums


class DeviceArrays(C.Structure):
    """gs_device_arrays: a trainer's six device arrays (include/gs3d_hip.h)."""
    _fields_ = [("means", C.c_void_p), ("log_scales", C.c_void_p), ("quats", C.c_void_p), ("opacity_logits", C.c_void_p),
                ("sh_dc", C.c_void_p), ("sh_rest", C.c_void_p), ("sh_rest_coeffs", C.c_uint32)]


class Transform(C.Structure):
    """gs_transform: x -> scale * R(rotation) x + translation (include/gs3d_hip.h)."""
    _fields_ = [("rotation", C.c_float * 4), ("translation", C.c_float * 3), ("scale", C.c_float)]


def _transform(rotation, translation, scale):
    t = Transform()
    t.rotation[:] = [float(v) for v in rotation]
    t.translation[:] = [float(v) for v in translation]
    t.scale = float(scale)
    return t


PARAMETER_NAMES = ("means", "log_scales", "quats", "opacity_logits", "sh_dc", "sh_rest")  # Scene.from_tensors' keywords


def _parameter_shapes(rows, k):
    """The shapes of the six parameter tensors of `rows` Gaussians under PARAMETER_NAMES, sh_rest with k coefficients above the DC
    term (None: an extent _tensor_exact does not check)."""
    return dict(means=(rows, 3), log_scales=(rows, 3), quats=(rows, 4), opacity_logits=(rows,), sh_dc=(rows, 3), sh_rest=(rows, k, 3))


def _torch_device(dev):
    """The torch device of a scene on GPU `dev`: where the wrappers allocate what they are asked to."""
    return f"cuda:{int(dev)}"


def _tensor_shape(name, t, dtypes):
    """The first checks of a device tensor `t`: it has a tensor's attributes and one of `dtypes`.  Returns its shape."""
    if not all(hasattr(t, a) for a in ("data_ptr", "shape", "dtype", "is_contiguous", "device")):
        raise TypeError(f"{name}: a device tensor is needed (data_ptr, shape, dtype, is_contiguous, device), got {type(t).__name__}")
    if str(t.dtype).rsplit(".", 1)[-1] not in dtypes:
        raise TypeError(f"{name}: dtype must be {' or '.join(dtypes)}, not {t.dtype}")
    return tuple(int(d) for d in t.shape)


def _tensor_on_device(name, t, device, instead, holder):
    """The last checks of a device tensor `t`: it is on GPU `device`, where `holder` is; `instead` says what a CPU tensor misses."""
    dev = t.device
    kind, index = getattr(dev, "type", str(dev).split(":")[0]), getattr(dev, "index", None)
    if kind == "cpu":
        raise ValueError(f"{name}: the tensor is on the CPU; {instead}")
    if (0 if index is None else int(index)) != int(device):
        raise ValueError(f"{name}: the tensor is on device {index}, the {holder} on device {device}")


def _tensor_rows(name, t, trailing, device):
    """Rows of device tensor `t` after checking it is what gs_device_arrays takes: float32, contiguous, on GPU `device`, of
    shape (rows, *trailing) up to singleton axes (the Inria trainer keeps _features_dc as (N, 1, 3), _opacity as (N, 1)).
    `trailing` None: (rows, k, 3) with k in {0, 3, 8, 15}; returns (rows, k) then."""
    shape = _tensor_shape(name, t, ("float32",))
    if len(shape) < 1:
        raise ValueError(f"{name}: shape {shape} has no row axis")
    if not t.is_contiguous():
        raise ValueError(f"{name}: the tensor must be contiguous (dense rows); call .contiguous()")
    rows, rest = shape[0], tuple(d for d in shape[1:] if d != 1) if trailing is not None else shape[1:]
    if trailing is None:
        if len(rest) != 2 or rest[1] != 3 or rest[0] not in (0, 3, 8, 15):
            raise ValueError(f"{name}: shape {shape} is not (rows, k, 3) with k in 0, 3, 8, 15")
        rows = (rows, rest[0])
    elif rest != tuple(d for d in trailing if d != 1):
        raise ValueError(f"{name}: shape {shape} is not (rows, {', '.join(map(str, trailing))})")
    _tensor_on_device(name, t, device, "Scene.from_records takes host data", "scene")
    return rows


def _tensor_exact(name, t, dtypes, shape, device, owner="Renderer.contributions"):
    """data_ptr of device tensor `t` after checking it is what gs_contributions / gs_feature_maps take: one of `dtypes`,
    contiguous, on GPU `device`, of exactly `shape` (a None extent is not checked)."""
    got = _tensor_shape(name, t, dtypes)
    if len(got) != len(shape) or any(w is not None and g != w for g, w in zip(got, shape)):
        raise ValueError(f"{name}: shape {got} is not ({', '.join('?' if w is None else str(w) for w in shape)})")
    if not t.is_contiguous():
        raise ValueError(f"{name}: the tensor must be contiguous; call .contiguous()")
    _tensor_on_device(name, t, device, f"the arrays of {owner} live on the renderer's device", "renderer")
    return t.data_ptr() if all(got) else None


def _device_arrays(tensors, device, require):
    """(DeviceArrays, rows) from {member: tensor or None}; every check of the tensors happens here, before C is called."""
    shapes = _parameter_shapes(None, None)
    a, rows = DeviceArrays(), None
    for name, t in tensors.items():
        if t is None:
            if require and name != "sh_rest":
                raise TypeError(f"{name} is required")
            continue
        r = _tensor_rows(name, t, None if name == "sh_rest" else shapes[name][1:] or (1,), device)
        if name == "sh_rest":
            r, a.sh_rest_coeffs = r
            if a.sh_rest_coeffs == 0:
                continue  # (rows, 0, 3): degree 0, no pointer
        if rows is not None and r != rows:
            raise ValueError(f"{name} has {r} rows, the arrays before it {rows}")
        rows = r
        setattr(a, name, t.data_ptr() if r else None)
    return a, (rows or 0)


class Contributions(C.Structure):
    """gs_contributions: the mask and the three outputs of gs_accumulate_contributions (include/gs3d_hip.h)."""
    _fields_ = [("mask", C.c_void_p), ("weight", C.c_void_p), ("pixels", C.c_void_p), ("top_id", C.c_void_p)]


class FeatureMaps(C.Structure):
    """gs_feature_maps: the per-Gaussian channels and the four per-pixel outputs of gs_blend_features (include/gs3d_hip.h)."""
    _fields_ = [("features", C.c_void_p), ("channels", C.c_uint32), ("out_features", C.c_void_p), ("out_alpha", C.c_void_p),
                ("out_depth", C.c_void_p), ("out_depth_median", C.c_void_p)]


FEATURE_CHANNELS_MAX = 256  # GS_FEATURE_CHANNELS_MAX


class PixelLift(C.Structure):
    """gs_pixel_lift: the per-pixel channels, the mask and the two per-Gaussian sums of gs_lift_pixels (include/gs3d_hip.h)."""
    _fields_ = [("values", C.c_void_p), ("channels", C.c_uint32), ("mask", C.c_void_p), ("out", C.c_void_p),
                ("out_weight", C.c_void_p)]


LIFT_CHANNELS_MAX = 256  # GS_LIFT_CHANNELS_MAX


class BlendGrads(C.Structure):
    """gs_blend_grads: the two per-pixel gradient maps and the four per-Gaussian sums of gs_blend_backward (include/gs3d_hip.h)."""
    _fields_ = [("grad_rgb", C.c_void_p), ("grad_alpha", C.c_void_p), ("d_colour", C.c_void_p), ("d_opacity", C.c_void_p),
                ("d_conic", C.c_void_p), ("d_uv", C.c_void_p)]



class ProjectGrads(C.Structure):
    """gs_project_grads: the four per-Gaussian input gradients and the six parameter-gradient sums of gs_project_backward
    (include/gs3d_hip.h)."""
    _fields_ = [("d_colour", C.c_void_p), ("d_opacity", C.c_void_p), ("d_conic", C.c_void_p), ("d_uv", C.c_void_p),
                ("d_means", C.c_void_p), ("d_log_scales", C.c_void_p), ("d_quats", C.c_void_p), ("d_opacity_logits", C.c_void_p),
                ("d_sh_dc", C.c_void_p), ("d_sh_rest", C.c_void_p), ("sh_rest_coeffs", C.c_uint32)]


class CameraGrads(C.Structure):
    """gs_camera_grads: the four per-Gaussian input gradients and the three uniform-gradient sums of gs_camera_backward
    (include/gs3d_hip.h)."""
    _fields_ = [("d_colour", C.c_void_p), ("d_opacity", C.c_void_p), ("d_conic", C.c_void_p), ("d_uv", C.c_void_p),
                ("d_view_mat", C.c_void_p), ("d_proj_mat", C.c_void_p), ("d_camera_position", C.c_void_p)]


class PhotoLoss(C.Structure):
    """gs_photo_loss: the two images, their size and pixel strides, lambda and the two outputs of gs_photometric_loss
    (include/gs3d_hip.h)."""
    _fields_ = [("image", C.c_void_p), ("target", C.c_void_p), ("width", C.c_int), ("height", C.c_int),
                ("image_stride", C.c_int), ("target_stride", C.c_int), ("lambda_dssim", C.c_double),
                ("terms", C.c_void_p), ("grad_rgb", C.c_void_p)]


class AdamGroup(C.Structure):
    """gs_adam_group: one parameter tensor of the trainer with its gradient and moments, and its learning rate."""
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("lr", C.c_double)]


class AdamStep(C.Structure):
    """gs_adam_step: the six groups, the mask and the constants of gs_scene_adam_step (include/gs3d_hip.h)."""
    _fields_ = [("means", AdamGroup), ("log_scales", AdamGroup), ("quats", AdamGroup), ("opacity_logits", AdamGroup),
                ("sh_dc", AdamGroup), ("sh_rest", AdamGroup), ("sh_rest_coeffs", C.c_uint32), ("mask", C.c_void_p),
                ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double),
                ("bias_correction1", C.c_double), ("bias_correction2", C.c_double), ("zero_grads", C.c_int)]


class DensifyStats(C.Structure):
    """gs_densify_stats: blend_backward's uv sum and the three statistic arrays of gs_accumulate_densify_stats (include/gs3d_hip.h)."""
    _fields_ = [("d_uv", C.c_void_p), ("grad_sum", C.c_void_p), ("count", C.c_void_p), ("max_radius", C.c_void_p)]


class DensifyRule(C.Structure):
    """gs_densify_rule: the thresholds of gs_densify_plan (include/gs3d_hip.h); max_screen_radius, max_world_scale <= 0: off."""
    _fields_ = [("grad_threshold", C.c_double), ("dense_extent", C.c_double), ("min_opacity", C.c_double),
                ("max_screen_radius", C.c_double), ("max_world_scale", C.c_double)]


class DensifyInput(C.Structure):
    """gs_densify_input: the model, its statistics, the rule and the scratch of gs_densify_plan / gs_densify_apply."""
    _fields_ = [("params", DeviceArrays), ("grad_sum", C.c_void_p), ("count", C.c_void_p), ("max_radius", C.c_void_p),
                ("rule", DensifyRule), ("scratch", C.c_void_p)]


class DensifyOutput(C.Structure):
    """gs_densify_output: the moments in, the noise, the plan's two counts and every output array of gs_densify_apply."""
    _fields_ = [("exp_avg", C.c_void_p * 6), ("exp_avg_sq", C.c_void_p * 6), ("noise", C.c_void_p), ("n_noise", C.c_uint64),
                ("n_out", C.c_uint64), ("params", DeviceArrays), ("out_exp_avg", C.c_void_p * 6), ("out_exp_avg_sq", C.c_void_p * 6)]


DENSIFY_PARTITION = 2048  # GS_DENSIFY_PARTITION: parents per workgroup of the plan's scan
DENSIFY_BLOCK = 256       # GS_DENSIFY_BLOCK: parents per workgroup of the apply
DENSIFY_LOG_1_6 = float.fromhex("0x1.e148a1a2726cep-2")  # GS_DENSIFY_LOG_1_6
DENSIFY_STATS = dict(grad_sum=("float64",), count=("int32", "uint32"), max_radius=("float32",))  # the statistic's tensors and dtypes


PHOTO_LOSS_MAX_EXTENT = 16384   # GS_PHOTO_LOSS_MAX_EXTENT: width and height of gs_photometric_loss
CAMERA_BACKWARD_LANES = 131072  # GS_CAMERA_BACKWARD_LANES: a scene with more Gaussians is strided over by gs_camera_backward's lanes

_AUTOGRAD = None  # the torch.autograd.Functions of Renderer.differentiable_*, defined when first asked for (_autograd)


def _complete_callers_work(*tensors):
    """gs_lift_pixels, gs_blend_backward (and gs_blend_features under autograd) run on the renderer's own stream, which is non-blocking: nothing
    orders it behind the stream the caller's tensors were produced on.  If any of `tensors` is a torch device tensor, wait on the
    host for torch's CURRENT stream of that device: a fill, a copy, an optimizer step or a backward kernel still queued there has
    then finished before the pass reads or adds to the tensor.  (The pass returns synchronised, so later work on torch's stream
    is ordered behind it without more.)  Work queued on other streams is the caller's to order."""
    import sys
    torch = sys.modules.get("torch")
    if torch is None:
        return
    for t in tensors:
        if getattr(t, "is_cuda", False) is True:
            torch.cuda.current_stream(t.device).synchronize()
            return


def _record_shapes(n):
    """The shapes of the four float64 gradients per Gaussian with respect to a frame's records: what blend_backward sums and
    project_backward and camera_backward take."""
    return dict(colour=(n, 3), opacity=(n,), conic=(n, 3), uv=(n, 2))


def _record_gradients(struct, owner, n, device, **given):
    """Set the d_colour / d_opacity / d_conic / d_uv inputs of `struct` from the tensors `given` under those names; None = zeros."""
    for name, shape in _record_shapes(n).items():
        if given[name] is not None:
            setattr(struct, "d_" + name, _tensor_exact(name, given[name], ("float64",), shape, device, owner))


def _output(value, member, dtype, shape, zeros=False, key=None):
    """One output of a pass, for _outputs: `value` is a tensor to fill, True to have one allocated, or None to skip; `member` of the
    C struct takes its pointer; it has `dtype` and exactly `shape`, and holds zeros, or nothing yet, when it is allocated here; the
    result holds it under `key` (None: under the name it is checked by)."""
    return value, member, dtype, shape, zeros, key


def _outputs(struct, owner, device, outputs):
    """The passes' output protocol over {name: _output(...)}: an output that is None is skipped, one that is True is allocated on
    the scene's device, each is checked as `owner`'s tensor `name` (_tensor_exact) and its pointer set in `struct`.  Returns
    {key: tensor} of the outputs that were asked for."""
    result = {}
    for name, (t, member, dtype, shape, zeros, key) in outputs.items():
        if t is None:
            continue
        if t is True:
            import torch
            t = (torch.zeros if zeros else torch.empty)(shape, dtype=getattr(torch, dtype), device=_torch_device(device))
        setattr(struct, member, _tensor_exact(name, t, (dtype,), shape, device, owner))
        result[name if key is None else key] = t
    return result


def _autograd():
    """The torch.autograd.Functions behind Renderer.differentiable_feature_maps, _render, _render_posed and _photometric_loss, as
    the attributes feature_maps, render, render_posed and photometric_loss; torch is imported here, not with the module."""
    global _AUTOGRAD
    if _AUTOGRAD is not None:
        return _AUTOGRAD
    import types

    import torch

    def render_frame(ctx, renderer, uniforms, want_alpha, params, refresh):
        """The forward of both render functions from the uniforms on: the scene refreshed from `params` if `refresh`, the frame
        rendered into a fresh tensor and synchronised, what the backward needs kept in ctx; rgb, and alpha if wanted."""
        renderer.synchronize()  # (no frame of this renderer may straddle the update)
        if refresh:
            renderer.scene.update_from_tensors(0, **{k: (None if v is None else v.detach().contiguous()) for k, v in params.items()})
        h, w = int(uniforms["height"][0]), int(uniforms["width"][0])
        rgba = torch.empty((h, w, 4), dtype=torch.float32, device=_torch_device(renderer.scene.device))
        renderer.render(uniforms, rgba.data_ptr())
        renderer.synchronize()
        ctx.renderer, ctx.frame = renderer, renderer._frames
        ctx.shapes = {k: (None if v is None else tuple(v.shape)) for k, v in params.items()}
        rgb = rgba[..., :3].contiguous()
        if not want_alpha:
            return rgb
        return rgb, renderer.feature_maps(alpha=True)["alpha"]

    def record_gradients(ctx, method, grad_rgb, grad_alpha):
        """The backward of both render functions as far as the records: blend_backward of the frame the forward rendered."""
        rend = ctx.renderer
        if rend._frames != ctx.frame:
            raise RuntimeError(f"{method}: the forward rendered frame {ctx.frame} of this renderer, which has "
                               f"rendered frame {rend._frames} since; the gradient of another frame is not returned")
        if grad_rgb is None:
            grad_rgb = torch.zeros(rend._frame_hw + (3,), dtype=torch.float32, device=_torch_device(rend.scene.device))
        return rend.blend_backward(grad_rgb.contiguous().float(), None if grad_alpha is None else grad_alpha.contiguous().float(),
                                   colour=True, opacity=True, conic=True, uv=True)

    def parameter_gradients(ctx, d, want):
        """project_backward of the record gradients `d` into float64 zeros for the names that `want` marks (PARAMETER_NAMES' order),
        rounded to float32 in the shapes the forward was given; None for a name not wanted or not given.  sh_rest of k = 0 has no
        array in C: its gradient is float32 zeros."""
        rend, dev = ctx.renderer, _torch_device(ctx.renderer.scene.device)
        rest = ctx.shapes["sh_rest"]
        k = 0 if rest is None else int(rest[-2])
        shapes = _parameter_shapes(int(rend.scene.num_vertices), k)
        out = {name: torch.zeros(shapes[name], dtype=torch.float64, device=dev)
               for name, need in zip(PARAMETER_NAMES, want) if need and (name != "sh_rest" or k)}
        rend.project_backward(out=out, **d)
        grads = [out[name].to(torch.float32).reshape(ctx.shapes[name]) if name in out and ctx.shapes[name] is not None else None
                 for name in PARAMETER_NAMES]
        if want[5] and rest is not None and not k:
            grads[5] = torch.zeros(rest, dtype=torch.float32, device=dev)
        return grads

    class FeatureMapsFunction(torch.autograd.Function):
        """out = feature_maps(features) of the renderer's last frame; d/dfeatures only -- the frame is a constant."""

        @staticmethod
        def forward(ctx, renderer, features):
            ctx.renderer, ctx.frame = renderer, renderer._frames
            _complete_callers_work(features)  # (an optimizer step on the features may still be queued on torch's stream)
            return renderer.feature_maps(features=features.detach().contiguous(), out=True)["out"]

        @staticmethod
        def backward(ctx, grad):
            rend = ctx.renderer
            if rend._frames != ctx.frame:
                raise RuntimeError(f"differentiable_feature_maps: the forward blended frame {ctx.frame} of this renderer, which has "
                                   f"rendered frame {rend._frames} since; the gradient of another frame is not returned")
            lifted = rend.lift_pixels(grad.contiguous().float(), out=True)["out"]
            return None, lifted.to(torch.float32)

    class RenderFunction(torch.autograd.Function):
        """rgb (and alpha) of one frame of the renderer's scene, refreshed from the six parameter tensors; the backward is
        blend_backward then project_backward, at the frame's values, rounded to float32."""

        @staticmethod
        def forward(ctx, renderer, uniforms, want_alpha, means, log_scales, quats, opacity_logits, sh_dc, sh_rest):
            params = dict(zip(PARAMETER_NAMES, (means, log_scales, quats, opacity_logits, sh_dc, sh_rest)))
            return render_frame(ctx, renderer, uniforms, want_alpha, params, refresh=True)

        @staticmethod
        def backward(ctx, grad_rgb, grad_alpha=None):
            d = record_gradients(ctx, "differentiable_render", grad_rgb, grad_alpha)
            return (None, None, None, *parameter_gradients(ctx, d, want=(True,) * 6))

    class RenderPosedFunction(torch.autograd.Function):
        """rgb (and alpha) of one frame seen from the pose (position, rotation); the backward is blend_backward, then
        camera_backward and camera_pose_gradient for the pose, and project_backward only for scene tensors that ask."""

        @staticmethod
        def forward(ctx, renderer, width, height, fov, near, far, want_alpha, position, rotation, means, log_scales, quats,
                    opacity_logits, sh_dc, sh_rest):
            params = dict(zip(PARAMETER_NAMES, (means, log_scales, quats, opacity_logits, sh_dc, sh_rest)))
            pose = [np.ascontiguousarray(t.detach().to("cpu", torch.float32).numpy().reshape(-1)) for t in (position, rotation)]
            if pose[0].shape != (3,) or pose[1].shape != (4,):
                raise ValueError(f"position must hold 3 values and rotation 4 (w x y z), not {pose[0].shape[0]} and {pose[1].shape[0]}")
            cam = make_camera(position=pose[0], rotation=pose[1], fov=fov, near=near, far=far)
            ctx.cam, ctx.size = cam, (int(width), int(height))
            ctx.pose = [(t.dtype, t.device, tuple(t.shape)) for t in (position, rotation)]
            return render_frame(ctx, renderer, camera_uniforms(cam, int(width), int(height)), want_alpha, params,
                                refresh=any(v is not None for v in params.values()))

        @staticmethod
        def backward(ctx, grad_rgb, grad_alpha=None):
            d = record_gradients(ctx, "differentiable_render_posed", grad_rgb, grad_alpha)
            pose, grads = [None, None], [None] * 6
            if ctx.needs_input_grad[7] or ctx.needs_input_grad[8]:
                found = camera_pose_gradient(ctx.cam, ctx.size[0], ctx.size[1], ctx.renderer.camera_backward(**d))
                pose = [torch.as_tensor(g).to(device=device, dtype=dtype).reshape(shape) if need else None
                        for g, (dtype, device, shape), need in zip(found, ctx.pose, ctx.needs_input_grad[7:9])]
            if any(ctx.needs_input_grad[9:]):
                grads = parameter_gradients(ctx, d, want=ctx.needs_input_grad[9:])
            return (None, None, None, None, None, None, None, *pose, *grads)

    class PhotoLossFunction(torch.autograd.Function):
        """loss(image, target) as a 0-dim float64 tensor; the forward's one call also finds d loss / d image, which the
        backward scales.  The target carries no gradient.  Nothing of the renderer's last frame is involved."""

        @staticmethod
        def forward(ctx, renderer, lambda_dssim, image, target):
            got = renderer.photometric_loss(image.detach().contiguous(), target.detach().contiguous(), lambda_dssim, grad=True, terms=True)
            ctx.save_for_backward(got["grad_rgb"])
            ctx.image = (tuple(image.shape), image.dtype)
            return got["loss"].clone()

        @staticmethod
        def backward(ctx, grad_output):
            (saved,) = ctx.saved_tensors
            shape, dtype = ctx.image
            g = grad_output.float() * saved
            if shape[-1] == 4:   # (an RGBA image: the fourth float is not read, its gradient is zero)
                g = torch.cat([g, torch.zeros(shape[:2] + (1,), dtype=g.dtype, device=g.device)], dim=2)
            return None, None, g.to(dtype), None

    _AUTOGRAD = types.SimpleNamespace(feature_maps=FeatureMapsFunction, render=RenderFunction, render_posed=RenderPosedFunction,
                                      photometric_loss=PhotoLossFunction)
    return _AUTOGRAD


def camera_pose_gradient(cam, width, height, d):
    """(d_position (3,), d_rotation (4,)) float64 numpy: the gradients with respect to a camera's position and RAW quaternion
    (w x y z; a caller who keeps it unit projects onto the sphere's tangent themselves) from `d`, the dict of
    Renderer.camera_backward -- view_mat (16,), proj_mat (16,), camera_position (3,), float64; a missing or None entry is zeros;
    device tensors are brought to the host here (gs_camera_uniforms_backward: host arithmetic, binary64)."""
    def host(name, count):
        t = d.get(name)
        if t is None:
            return np.zeros(count, np.float64)
        a = np.ascontiguousarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, np.float64).reshape(-1)
        if a.shape != (count,):
            raise ValueError(f"{name}: {a.shape[0]} values, {count} are needed")
        return a
    unknown = sorted(set(d) - {"view_mat", "proj_mat", "camera_position"})
    if unknown:
        raise TypeError(f"d: unknown member(s) {unknown}")
    gv, gp, gc = host("view_mat", 16), host("proj_mat", 16), host("camera_position", 3)
    cam = np.ascontiguousarray(cam, CAMERA_DT)
    d_position, d_rotation = np.zeros(3, np.float64), np.zeros(4, np.float64)
    _check(lib().gs_camera_uniforms_backward(_p(cam), C.c_uint32(int(width)), C.c_uint32(int(height)), _p(gv), _p(gp), _p(gc),
                                             _p(d_position), _p(d_rotation)))
    return d_position, d_rotation


def _stream_handle(stream):
    """hipStream_t for the C ABI: an int / None-able handle, a torch stream (its cuda_stream), or -- None -- torch's current
    stream when torch is imported (work then orders itself behind the trainer's), else the default stream."""
    import sys
    if stream is None:
        torch = sys.modules.get("torch")
        if torch is None or not torch.cuda.is_available():
            return None
        stream = torch.cuda.current_stream()
    return C.c_void_p(int(getattr(stream, "cuda_stream", stream)) or None)


class GsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"[{code}] {msg}")
        self.code = code


_LIB = None


def lib():
    """Load libgs3d_hip.so; raises (never falls back) when it has not been built."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise GsError(-3, f"{LIB_PATH} is missing: run __graft_entry__.build() (hipcc, gfx950)")
        L = C.CDLL(LIB_PATH)
        L.gs_last_error.restype = C.c_char_p
        L.gs_scene_num_vertices.restype = C.c_uint64
        L.gs_scene_num_vertices.argtypes = [C.c_void_p]
        L.gs_scene_blob_floats.restype = C.c_uint64
        L.gs_scene_blob_floats.argtypes = [C.c_uint64]
        L.gs_renderer_stream.restype = C.c_void_p
        L.gs_renderer_stream.argtypes = [C.c_void_p]
        L.gs_scene_destroy.argtypes = [C.c_void_p]
        L.gs_renderer_destroy.argtypes = [C.c_void_p]
        L.gs_scene_destroy.restype = None
        L.gs_renderer_destroy.restype = None
        _LIB = L
    return _LIB


def _check(rc):
    if rc != 0:
        raise GsError(rc, lib().gs_last_error().decode(errors="replace"))


def _p(a):
    """Pointer to a numpy array's data for the duration of a call (the caller holds the array).  NOT `a.ctypes.data_as(...)`: that
    builds a reference cycle per call (the pointer object keeps the array, the array's ctypes helper keeps the pointer), i.e. two
    objects of cyclic garbage per gs_render -- enough to trigger Python's full (generation-2) collection once per ~2 000 frames,
    which in a process that has imported torch walks ~170 000 objects and holds the frame loop for 35-45 ms: the "once per run"
    stall of bench.py's rounds 2-4 (profiles/r05_stall_hunt.txt).

    CONTRACT: the returned pointer does NOT keep `a` alive.  Pass a NAMED array that outlives the C call -- never a temporary
    (`_p(np.ascontiguousarray(x))` would hand C a dangling pointer).  What can be checked here is: an ndarray, C-contiguous."""
    if not isinstance(a, np.ndarray) or not a.flags["C_CONTIGUOUS"]:
        raise TypeError("_p() takes a C-contiguous numpy array that the caller keeps alive for the duration of the call")
    return C.c_void_p(a.ctypes.data)


def device_count():
    n = C.c_int(0)
    _check(lib().gs_device_count(C.byref(n)))
    return n.value


def make_camera(position=(0, 0, 0), rotation=(1, 0, 0, 0), fov=45.0, near=0.1, far=1000.0):
    """Renderer::Camera with the reference defaults (Renderer.h:79-85)."""
    cam = np.zeros(1, CAMERA_DT)
    cam["position"] = position
    cam["rotation"] = rotation
    cam["fov"], cam["near_plane"], cam["far_plane"] = fov, near, far
    return cam


def camera_uniforms(cam, width, height):
    out = np.zeros(1, UNIFORMS_DT)
    _check(lib().gs_camera_uniforms(_p(cam), C.c_uint32(width), C.c_uint32(height), _p(out)))
    return out


def transform_camera(cam, rotation=(1, 0, 0, 0), translation=(0, 0, 0), scale=1.0):
    """The camera that sees a scene moved by Scene.transform(rotation, translation, scale) exactly as `cam` saw it before
    (gs_transform_camera; host only)."""
    t, out = _transform(rotation, translation, scale), np.zeros(1, CAMERA_DT)
    cam = np.ascontiguousarray(cam, CAMERA_DT)
    _check(lib().gs_transform_camera(C.byref(t), _p(cam), _p(out)))
    return out


def sh_rotation_matrices(rotation=(1, 0, 0, 0)):
    """The matrices that rotate the SH bands 1, 2, 3 with the quaternion (w, x, y, z): float32 arrays of shape (3, 3), (5, 5),
    (7, 7), c' = M @ c over a band's coefficients of one channel (gs_transform_sh_matrices; host only)."""
    t, out = _transform(rotation, (0, 0, 0), 1.0), np.zeros(83, np.float32)
    _check(lib().gs_transform_sh_matrices(C.byref(t), _p(out)))
    return out[0:9].reshape(3, 3).copy(), out[9:34].reshape(5, 5).copy(), out[34:83].reshape(7, 7).copy()


def activate_records(records):
    """GSScene::load's record conversion on the host (no GPU needed): (n, 62) -> (n, 60)."""
    records = np.ascontiguousarray(records, np.float32).reshape(-1, RECORD_FLOATS)
    out = np.zeros((len(records), VERTEX_FLOATS), np.float32)
    _check(lib().gs_activate_records(_p(records), C.c_uint64(len(records)), _p(out)))
    return out


def read_ply(path):
    """loadPlyHeader + payload (host only): raw (n, 62) records."""
    n = C.c_uint64()
    _check(lib().gs_read_ply(os.fsencode(path), None, C.c_uint64(0), C.byref(n)))
    out = np.zeros((n.value, RECORD_FLOATS), np.float32)
    _check(lib().gs_read_ply(os.fsencode(path), _p(out), C.c_uint64(n.value), C.byref(n)))
    return out


def deactivate_vertices(vertices):
    """The inverse of activate_records on the host (no GPU needed): (n, 60) -> (n, 62) PLY records (gs_deactivate_vertices)."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, VERTEX_FLOATS)
    out = np.zeros((len(v), RECORD_FLOATS), np.float32)
    _check(lib().gs_deactivate_vertices(_p(v), C.c_uint64(len(v)), _p(out)))
    return out


def write_ply(path, records):
    """(n, 62) records as the reference's binary PLY (host only; gs_write_ply)."""
    records = np.ascontiguousarray(records, np.float32).reshape(-1, RECORD_FLOATS)
    _check(lib().gs_write_ply(os.fsencode(path), _p(records), C.c_uint64(len(records))))


SH_REST_COEFFS = {0: 0, 1: 3, 2: 8, 3: 15}  # SH degree -> coefficients above the DC term


def _densify_stats(struct, stats, n, device, owner):
    """Set grad_sum / count / max_radius of `struct` from the dict `stats` after checking its three tensors; returns them."""
    unknown = sorted(set(stats) - set(DENSIFY_STATS))
    if unknown:
        raise TypeError(f"stats: unknown member(s) {unknown}")
    used = []
    for name, dtypes in DENSIFY_STATS.items():
        if stats.get(name) is None:
            raise TypeError(f"stats[{name!r}] is required")
        setattr(struct, name, _tensor_exact(f"stats[{name!r}]", stats[name], dtypes, (n,), device, owner))
        used.append(stats[name])
    return used


def densify_stats_zeros(scene):
    """The three tensors Renderer.densify_stats accumulates into and densify decides by, zeroed, on the scene's device:
    {grad_sum: float64 (N,), count: int32 (N,), max_radius: float32 (N,)}."""
    import torch
    n, dev = int(scene.num_vertices), _torch_device(scene.device)
    return dict(grad_sum=torch.zeros(n, dtype=torch.float64, device=dev), count=torch.zeros(n, dtype=torch.int32, device=dev),
                max_radius=torch.zeros(n, dtype=torch.float32, device=dev))


def _densify_rule(rule):
    """DensifyRule from a DensifyRule or a dict of its members (max_screen_radius and max_world_scale default to 0 = off)."""
    if isinstance(rule, DensifyRule):
        return rule
    names = [f[0] for f in DensifyRule._fields_]
    unknown = sorted(set(rule) - set(names))
    if unknown:
        raise TypeError(f"rule: unknown member(s) {unknown}")
    r = DensifyRule()
    for name in names:
        if name not in rule and name not in ("max_screen_radius", "max_world_scale"):
            raise TypeError(f"rule[{name!r}] is required")
        v = float(rule.get(name, 0.0))
        if v != v:
            raise ValueError(f"rule[{name!r}] is NaN")
        setattr(r, name, v)
    return r


def densify(scene, params, rule, stats, state=None, noise=None, stream=None):
    """Adaptive density control of a trainer's model on the device (gs_densify_plan + gs_densify_apply): clone
    the Gaussians whose average screen-space gradient norm reaches rule['grad_threshold'] and whose largest scale is at most
    rule['dense_extent'], split the larger ones in two (scales / 1.6, means drawn from the parent), then prune over the extended
    set -- opacity below rule['min_opacity'], a screen radius above rule['max_screen_radius'], a scale above
    rule['max_world_scale'] (<= 0 or absent: off).
    scene: the scene the model belongs to (its device and Gaussian count; it is not changed).  params: the six tensors of
    Scene.from_tensors under its keyword names (sh_rest may be absent or None).  stats: what Renderer.densify_stats accumulated.
    state: None, or {'exp_avg': {name: tensor}, 'exp_avg_sq': {name: tensor}} -- Adam's moments, float32, shaped as the
    parameters; a name absent from BOTH has no moments to carry.  noise: float32 (rows, 2, 3) standard-normal draws with at least
    as many rows as parents are split (n rows always suffice; rows beyond are not read), None: torch.randn.  The kernels hold no
    random number generator: with given noise the result is a pure function of the inputs, bit for bit.
    Returns (new_params, new_state, info): tensors of n_out rows allocated here, ordered by PARENT (a parent's survivors adjacent,
    the original before its copy); survivors keep parameters and moments bit for bit, new rows have zero moments; new_state is
    None when state is.  info: n_in, n_out, n_noise (= parents_split) and the parents by outcome -- parents_removed (no row left),
    parents_single, parents_cloned (two rows, not split), parents_split (two children) -- and the plan's two int32 tensors
    row_offset and noise_offset (n + 1 each): parent i's rows are [row_offset[i], row_offset[i + 1]) of the outputs, which carries
    any other per-Gaussian array of the caller's along.  The caller builds
    Scene.from_tensors(**new_params) and a new Renderer.  Waits for torch's current stream first; runs on `stream` (None:
    torch's current stream) and returns synchronised."""
    owner = "densify"
    dev, n = scene.device, int(scene.num_vertices)
    unknown = sorted(set(params) - set(PARAMETER_NAMES))
    if unknown:
        raise TypeError(f"params: unknown member(s) {unknown}")
    inp = DensifyInput()
    inp.params, rows = _device_arrays({name: params.get(name) for name in PARAMETER_NAMES}, dev, require=True)
    if rows != n:
        raise ValueError(f"params have {rows} rows, the scene {n} Gaussians")
    k = int(inp.params.sh_rest_coeffs)
    given = [name for name in PARAMETER_NAMES if params.get(name) is not None and (name != "sh_rest" or k)]
    used = [params[name] for name in given] + _densify_stats(inp, stats, n, dev, owner)
    inp.rule = _densify_rule(rule)
    out = DensifyOutput()
    moments = {}
    if state is not None:
        unknown = sorted(set(state) - {"exp_avg", "exp_avg_sq"})
        if unknown or "exp_avg" not in state or "exp_avg_sq" not in state:
            raise TypeError(f"state: a dict of exp_avg and exp_avg_sq is needed, got {sorted(state)}")
        for what in ("exp_avg", "exp_avg_sq"):
            unknown = sorted(set(state[what]) - set(PARAMETER_NAMES))
            if unknown:
                raise TypeError(f"state[{what!r}]: unknown member(s) {unknown}")
        for g, name in enumerate(PARAMETER_NAMES):
            have = [what for what in ("exp_avg", "exp_avg_sq") if state[what].get(name) is not None]
            if not have:
                continue
            if len(have) != 2:
                raise ValueError(f"{name}: a partial pair of moments -- given in {have[0]} only")
            if name not in given:
                raise ValueError(f"{name}: moments without the parameter")
            shape = tuple(int(d) for d in params[name].shape)
            for what in have:
                t = state[what][name]
                getattr(out, what)[g] = _tensor_exact(f"state[{what!r}][{name!r}]", t, ("float32",), shape, dev, owner)
                used.append(t)
            moments[name] = g
    if noise is not None:
        _tensor_exact("noise", noise, ("float32",), (None, 2, 3), dev, owner)
        used.append(noise)
    import torch
    L = lib()
    plan, apply = L.gs_densify_plan, L.gs_densify_apply   # (every check above comes before C, and before anything is allocated)
    _complete_callers_work(*used)
    handle = _stream_handle(stream)
    tdev = _torch_device(dev)
    scratch = torch.empty(2 * (n + 1), dtype=torch.int32, device=tdev)
    inp.scratch = scratch.data_ptr()
    n_out, n_noise = C.c_uint64(0), C.c_uint64(0)
    _check(plan(C.byref(inp), C.c_uint64(n), C.c_int(dev), handle, C.byref(n_out), C.byref(n_noise)))
    n_out, n_noise = int(n_out.value), int(n_noise.value)
    if noise is None:
        noise = torch.randn((n_noise, 2, 3), dtype=torch.float32, device=tdev)
        torch.cuda.current_stream(noise.device).synchronize()
    elif int(noise.shape[0]) < n_noise:
        raise ValueError(f"noise has {int(noise.shape[0])} rows, {n_noise} parents are split")
    out.noise, out.n_noise, out.n_out = (noise.data_ptr() if n_noise else None), n_noise, n_out
    out.params.sh_rest_coeffs = k
    new_params, new_state = {}, (None if state is None else dict(exp_avg={}, exp_avg_sq={}))
    for name in given:
        shape = (n_out,) + tuple(int(d) for d in params[name].shape[1:])
        new_params[name] = torch.empty(shape, dtype=torch.float32, device=tdev)
        setattr(out.params, name, new_params[name].data_ptr() if n_out else None)
        if name in moments:
            for what in ("exp_avg", "exp_avg_sq"):
                t = torch.empty(shape, dtype=torch.float32, device=tdev)
                new_state[what][name] = t
                getattr(out, "out_" + what)[moments[name]] = t.data_ptr() if n_out else None
    if "sh_rest" in params and params["sh_rest"] is not None and not k:
        new_params["sh_rest"] = torch.empty((n_out, 0, 3), dtype=torch.float32, device=tdev)
    _check(apply(C.byref(inp), C.c_uint64(n), C.byref(out), C.c_int(dev), handle))
    info = dict(n_in=n, n_out=n_out, n_noise=n_noise, parents_removed=0, parents_single=0, parents_cloned=0, parents_split=n_noise,
                row_offset=scratch[:n + 1], noise_offset=scratch[n + 1:])
    if n:
        rows_of = scratch[1:n + 1] - scratch[0:n]
        split = (scratch[n + 2:2 * n + 2] - scratch[n + 1:2 * n + 1]) != 0
        info["parents_removed"] = int((rows_of == 0).sum())
        info["parents_single"] = int((rows_of == 1).sum())
        info["parents_cloned"] = int(((rows_of == 2) & ~split).sum())
    return new_params, new_state, info


KNN_MAX_K = 8   # GS_KNN_MAX_K
KNN_BOX = 256   # GS_KNN_BOX: sorted points per box of the search = rows of box_visits per 256 points
SH_C0 = 0.28209479177387814  # the DC basis function: colour = 0.5 + SH_C0 sh_dc


def _device_index(t):
    """The GPU a tensor says it is on (0 where it does not say: _tensor_rows then judges the rest)."""
    index = getattr(getattr(t, "device", None), "index", None)
    return int(index) if isinstance(index, int) and not isinstance(index, bool) else 0


def knn_dist2(points, k=3, mean=True, dist2=False, visits=False, stream=None):
    """The squared distances of every point of a cloud to its k nearest neighbours, exact in binary32 (gs_knn_dist2;
    INTEGRATION.md, 3m): what a trainer derives its initial scales from (simple_knn.distCUDA2 for k = 3).
    points: float32 (n, 3) on a GPU, every coordinate finite (ValueError otherwise: one synchronising check, nothing is launched).
    Returns a dict of tensors on the points' device, allocated here: 'mean_dist2' float32 (n,) where `mean`, 'dist2' float32 (n, k),
    ascending, +inf beyond n - 1 neighbours, where `dist2`, 'box_visits' int32 (ceil(n / KNN_BOX),) where `visits` -- how many
    boxes of KNN_BOX Morton-sorted points each query box had to scan.  The values are those of the brute force over all pairs, bit
    for bit (tests/knn_reference.py).  Waits for torch's current stream first; runs on `stream` (None: torch's current stream) and
    returns synchronised."""
    dev = _device_index(points)
    n = _tensor_rows("points", points, (3,), dev)
    if isinstance(k, bool) or not isinstance(k, int):
        raise TypeError(f"k must be an int, not {type(k).__name__}")
    if not 1 <= k <= KNN_MAX_K:
        raise ValueError(f"k = {k} is outside [1, {KNN_MAX_K}]")
    if not (mean or dist2 or visits):
        raise ValueError("nothing asked for: mean, dist2 and visits are all false")
    import torch
    L = lib()
    call, scratch_bytes = L.gs_knn_dist2, L.gs_knn_scratch_bytes
    scratch_bytes.restype, scratch_bytes.argtypes = C.c_uint64, [C.c_uint64]
    if not bool(torch.isfinite(points).all()):   # (synchronises: the points are complete from here on)
        raise ValueError("points: a coordinate is NaN or infinite")
    _complete_callers_work(points)
    tdev = _torch_device(dev)
    out = {}
    if mean:
        out["mean_dist2"] = torch.empty((n,), dtype=torch.float32, device=tdev)
    if dist2:
        out["dist2"] = torch.empty((n, k), dtype=torch.float32, device=tdev)
    if visits:
        out["box_visits"] = torch.empty(((n + KNN_BOX - 1) // KNN_BOX,), dtype=torch.int32, device=tdev)
    if n == 0:
        return out
    scratch = torch.empty((int(scratch_bytes(C.c_uint64(n))),), dtype=torch.uint8, device=tdev)
    pointer = lambda name: C.c_void_p(out[name].data_ptr()) if name in out else None
    _check(call(C.c_void_p(points.data_ptr()), C.c_uint64(n), C.c_int(k), pointer("mean_dist2"), pointer("dist2"), pointer("box_visits"),
                C.c_void_p(scratch.data_ptr()), C.c_uint64(scratch.numel()), C.c_int(dev), _stream_handle(stream)))
    return out


def init_from_points(points, colours=None, k=3, opacity=0.1, sh_degree=3, min_dist2=1e-7, stream=None):
    """A model from a point cloud, as the Inria trainer's create_from_pcd makes it: the six float32 tensors
    under PARAMETER_NAMES, on the points' device, ready for Scene.from_tensors(**params) and Adam.
    means = points; log_scales = log(sqrt(clamp_min(mean_dist2, min_dist2))) on all three axes, mean_dist2 = knn_dist2(points, k);
    quats = (1, 0, 0, 0); opacity_logits = log(opacity / (1 - opacity)); sh_dc = (colours - 0.5) / SH_C0 with colours float32
    (n, 3) in [0, 1] (None: 0.5, i.e. zeros); sh_rest = zeros of (n, SH_REST_COEFFS[sh_degree], 3).  The distances are the
    kernels'; the rest is plain float32 torch arithmetic on the device."""
    if sh_degree not in SH_REST_COEFFS:
        raise ValueError(f"sh_degree = {sh_degree!r} is not one of {sorted(SH_REST_COEFFS)}")
    if not 0.0 < float(opacity) < 1.0:
        raise ValueError(f"opacity = {opacity!r} is not inside (0, 1)")
    if not float(min_dist2) > 0.0:
        raise ValueError(f"min_dist2 = {min_dist2!r} is not positive")
    dev = _device_index(points)
    n = _tensor_rows("points", points, (3,), dev)
    if colours is not None and _tensor_rows("colours", colours, (3,), dev) != n:
        raise ValueError(f"colours have {int(colours.shape[0])} rows, the points {n}")
    import math
    import torch
    mean_dist2 = knn_dist2(points, k=k, stream=stream)["mean_dist2"]
    tdev = points.device
    means = points.reshape(n, 3).clone()
    log_scales = torch.log(torch.sqrt(torch.clamp_min(mean_dist2, float(min_dist2)))).reshape(n, 1).repeat(1, 3)
    quats = torch.zeros((n, 4), dtype=torch.float32, device=tdev)
    quats[:, 0] = 1.0
    logit = math.log(float(opacity) / (1.0 - float(opacity)))
    opacity_logits = torch.full((n,), logit, dtype=torch.float32, device=tdev)
    if colours is None:
        sh_dc = torch.zeros((n, 3), dtype=torch.float32, device=tdev)
    else:
        sh_dc = (colours.reshape(n, 3) - 0.5) / SH_C0
    sh_rest = torch.zeros((n, SH_REST_COEFFS[sh_degree], 3), dtype=torch.float32, device=tdev)
    return dict(zip(PARAMETER_NAMES, (means, log_scales, quats, opacity_logits, sh_dc, sh_rest)))


class Scene:
    """GSScene counterpart (SoA in HBM)."""

    def __init__(self, handle, keepalive=None, device=0):
        self._h = handle
        self._keepalive = keepalive
        self.device = device

    @classmethod
    def load_ply(cls, path, device=0):
        h = C.c_void_p()
        _check(lib().gs_scene_load_ply(os.fsencode(path), C.c_int(device), C.byref(h)))
        return cls(h, device=device)

    @classmethod
    def from_records(cls, records, device=0):
        records = np.ascontiguousarray(records, np.float32).reshape(-1, RECORD_FLOATS)
        h = C.c_void_p()
        _check(lib().gs_scene_from_records(_p(records), C.c_uint64(len(records)), C.c_int(device), C.byref(h)))
        return cls(h, device=device)

    @classmethod
    def from_vertices(cls, vertices, device=0):
        """vertices: (n, 60) float32 or the structured GSScene::Vertex array."""
        v = np.ascontiguousarray(vertices).view(np.float32).reshape(-1, VERTEX_FLOATS)
        h = C.c_void_p()
        _check(lib().gs_scene_from_vertices(_p(v), C.c_uint64(len(v)), C.c_int(device), C.byref(h)))
        return cls(h, device=device)

    @classmethod
    def from_device_blob(cls, ptr, n, device=0, keepalive=None):
        h = C.c_void_p()
        _check(lib().gs_scene_from_device_blob(C.c_void_p(ptr), C.c_uint64(n), C.c_int(device), C.byref(h)))
        return cls(h, keepalive, device=device)

    @classmethod
    def from_tensors(cls, means, log_scales, quats, opacity_logits, sh_dc, sh_rest=None, stream=None, device=0):
        """A scene from a trainer's parameters as they lie on the GPU (gs_scene_from_device_arrays): float32, contiguous device
        tensors (anything with data_ptr / shape / dtype / is_contiguous / device) -- means (n, 3), log_scales (n, 3), quats
        (n, 4) w x y z, opacity_logits (n,) or (n, 1), sh_dc (n, 3) or (n, 1, 3), sh_rest (n, k, 3) with k in 0, 3, 8, 15 or
        None.  Activated on the device, bit for bit as from_records activates; nothing is copied to the host."""
        a, n = _device_arrays(dict(means=means, log_scales=log_scales, quats=quats, opacity_logits=opacity_logits, sh_dc=sh_dc,
                                   sh_rest=sh_rest), device, require=True)
        h = C.c_void_p()
        _check(lib().gs_scene_from_device_arrays(C.byref(a), C.c_uint64(n), C.c_int(device), _stream_handle(stream), C.byref(h)))
        return cls(h, device=device)

    def update_from_tensors(self, first, means=None, log_scales=None, quats=None, opacity_logits=None, sh_dc=None, sh_rest=None,
                            stream=None, device=0):
        """Overwrite Gaussians [first, first + rows) in place from such tensors (gs_scene_update_from_device_arrays); None keeps
        what the scene holds.  Synchronize every renderer of the scene first."""
        a, rows = _device_arrays(dict(means=means, log_scales=log_scales, quats=quats, opacity_logits=opacity_logits, sh_dc=sh_dc,
                                      sh_rest=sh_rest), device, require=False)
        _check(lib().gs_scene_update_from_device_arrays(self._h, C.byref(a), C.c_uint64(first), C.c_uint64(rows), _stream_handle(stream)))

    def adam_step(self, params, grads, exp_avg, exp_avg_sq, lr, betas=(0.9, 0.999), eps=1e-15, step=1, mask=None, zero_grads=True,
                  stream=None):
        """One sparse Adam step on the device, in the trainer's tensors and in this scene (gs_scene_adam_step): the thin layer
        over the C call.  params, grads, exp_avg, exp_avg_sq: dicts under from_tensors' keyword names; a name is a GROUP and is
        stepped when params holds a tensor for it -- then all four dicts must (a name absent or None in all four is not stepped
        and the scene keeps what it holds for it).  params and the moments are float32, grads float64 (what project_backward
        adds to), all contiguous on the scene's device, one row per Gaussian: means (n, 3), log_scales (n, 3), quats (n, 4),
        opacity_logits (n,), sh_dc (n, 3), sh_rest (n, k, 3) with k in 3, 8, 15 (k = 0: nothing to step).  lr: a float, or a dict
        per name.  step: t >= 1, the number of this step; the bias corrections are 1 - beta ** step in Python floats.
        mask: a uint8 tensor (n,) by scene id, nonzero = step this Gaussian (Renderer.visible_mask), None = every Gaussian.
        zero_grads: the gradient elements that were consumed are set to +0.0.  Parameters, moments and the scene's planes of
        every stepped group are updated for the masked Gaussians only; what is derived is redone.  Waits for torch's current
        stream first; runs on `stream` (None: torch's current stream) and returns synchronised.  Synchronize every renderer of
        the scene first."""
        owner = "Scene.adam_step"
        n, dev = int(self.num_vertices), self.device
        dicts = dict(params=params, grads=grads, exp_avg=exp_avg, exp_avg_sq=exp_avg_sq)
        for what, d in dicts.items():
            unknown = sorted(set(d) - set(PARAMETER_NAMES))
            if unknown:
                raise TypeError(f"{what}: unknown member(s) {unknown}")
        beta1, beta2 = (float(b) for b in betas)
        if int(step) != step or step < 1:
            raise ValueError(f"step must be an integer >= 1, not {step!r}")
        a = AdamStep()
        shapes = _parameter_shapes(n, None)
        members = dict(params=("param", "float32"), grads=("grad", "float64"), exp_avg=("exp_avg", "float32"), exp_avg_sq=("exp_avg_sq", "float32"))
        used = []
        for name in PARAMETER_NAMES:
            have = [what for what, d in dicts.items() if d.get(name) is not None]
            if not have:
                continue
            if len(have) != 4:
                raise ValueError(f"{name}: a partial group -- given in {', '.join(have)} but not in "
                                 f"{', '.join(w for w in dicts if w not in have)}")
            group, shape = getattr(a, name), shapes[name]
            for what, (member, dtype) in members.items():
                t = dicts[what][name]
                ptr = _tensor_exact(f"{what}[{name!r}]", t, (dtype,), shape, dev, owner)
                if name == "sh_rest":
                    k = int(t.shape[1])
                    if k not in SH_REST_COEFFS.values():
                        raise ValueError(f"{what}['sh_rest']: shape {tuple(int(d) for d in t.shape)} is not (rows, k, 3) with k in 0, 3, 8, 15")
                    if what != "params" and k != a.sh_rest_coeffs:
                        raise ValueError(f"{what}['sh_rest']: shape {tuple(int(d) for d in t.shape)} is not params['sh_rest']'s")
                    a.sh_rest_coeffs = k
                setattr(group, member, ptr)
                used.append(t)
            rate = lr[name] if isinstance(lr, dict) else lr
            group.lr = float(rate)
        if mask is not None:
            a.mask = _tensor_exact("mask", mask, ("uint8",), (n,), dev, owner)
            used.append(mask)
        a.beta1, a.beta2, a.eps = beta1, beta2, float(eps)
        a.bias_correction1, a.bias_correction2 = 1.0 - beta1 ** int(step), 1.0 - beta2 ** int(step)
        a.zero_grads = 1 if zero_grads else 0
        _complete_callers_work(*used)
        _check(lib().gs_scene_adam_step(self._h, C.byref(a), _stream_handle(stream)))

    def transform(self, rotation=(1, 0, 0, 0), translation=(0, 0, 0), scale=1.0, first=0, count=None, stream=None):
        """Move Gaussians [first, first + count) (count None: to the end) by x -> scale * R(rotation) x + translation, in place
        on the device: positions, scales, rotations and the SH bands, rotated with the splats (gs_scene_transform).
        rotation: quaternion (w, x, y, z), normalised by the library.  Synchronize every renderer of the scene first."""
        t = _transform(rotation, translation, scale)
        if count is None:
            count = max(0, self.num_vertices - int(first))
        _check(lib().gs_scene_transform(self._h, C.byref(t), C.c_uint64(first), C.c_uint64(count), _stream_handle(stream)))

    def to_tensors(self, first=0, count=None, sh_degree=3, stream=None, out=None):
        """Gaussians [first, first + count) (count None: to the end) as the PLY-domain tensors from_tensors takes, on the scene's
        device and without a host copy (gs_scene_to_device_arrays): a dict with from_tensors' keyword names -- means (count, 3),
        log_scales (count, 3), quats (count, 4), opacity_logits (count,), sh_dc (count, 3), sh_rest (count, k, 3) with k = 0, 3,
        8, 15 for sh_degree 0 .. 3 (higher bands are dropped).  Scales and opacities are the pre-activation values that
        activate to the stored bits; the rotation is the stored, normalised one.
        out: a dict of preallocated tensors under those names (float32, contiguous, on the scene's device, `count` rows each,
        shapes as from_tensors takes them); a name it lacks is not exported, sh_degree is then sh_rest's.  Returns out."""
        if count is None:
            count = max(0, self.num_vertices - int(first))
        if out is None:
            if sh_degree not in SH_REST_COEFFS:
                raise ValueError(f"sh_degree must be 0, 1, 2 or 3, not {sh_degree!r}")
            import torch
            out = {k: torch.empty(shape, dtype=torch.float32, device=_torch_device(self.device))
                   for k, shape in _parameter_shapes(count, SH_REST_COEFFS[sh_degree]).items()}
        unknown = sorted(set(out) - set(PARAMETER_NAMES))
        if unknown:
            raise TypeError(f"out: unknown member(s) {unknown}")
        a, rows = _device_arrays({k: out.get(k) for k in PARAMETER_NAMES}, self.device, require=False)
        given = [k for k in PARAMETER_NAMES if out.get(k) is not None and not (k == "sh_rest" and a.sh_rest_coeffs == 0)]
        if given and rows != count:
            raise ValueError(f"out: the tensors have {rows} rows, the range {count}")
        _check(lib().gs_scene_to_device_arrays(self._h, C.byref(a), C.c_uint64(first), C.c_uint64(count), _stream_handle(stream)))
        return out

    def download_records(self, first=0, count=None):
        """Gaussians [first, first + count) (count None: to the end) as (count, 62) PLY records on the host
        (gs_scene_download_records): deactivate_vertices(download_vertex_range(first, count)), bit for bit."""
        if count is None:
            count = max(0, self.num_vertices - int(first))
        out = np.zeros((count, RECORD_FLOATS), np.float32)
        _check(lib().gs_scene_download_records(self._h, C.c_uint64(first), C.c_uint64(count), _p(out)))
        return out

    def save_ply(self, path):
        """The scene as the reference's binary PLY, streamed from the device (gs_scene_save_ply)."""
        _check(lib().gs_scene_save_ply(self._h, os.fsencode(path)))

    @property
    def num_vertices(self):
        return lib().gs_scene_num_vertices(self._h)

    def blob(self):
        """(device pointer, float count) of the packed SoA blob."""
        p = C.c_void_p()
        n = C.c_uint64()
        _check(lib().gs_scene_blob(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def download_vertices(self):
        out = np.zeros((self.num_vertices, VERTEX_FLOATS), np.float32)
        _check(lib().gs_scene_download_vertices(self._h, _p(out)))
        return out

    def quantize_sh(self):
        """Round the SH coefficients to binary16 storage (opt-in; gs_scene_quantize_sh)."""
        _check(lib().gs_scene_quantize_sh(self._h))

    @property
    def sh_bits(self):
        return lib().gs_scene_sh_bits(self._h)

    def download_vertex_range(self, first, count):
        out = np.zeros((count, VERTEX_FLOATS), np.float32)
        _check(lib().gs_scene_download_vertex_range(self._h, C.c_uint64(first), C.c_uint64(count), _p(out)))
        return out

    def download_cov3d(self):
        out = np.zeros((self.num_vertices, 6), np.float32)
        _check(lib().gs_scene_download_cov3d(self._h, _p(out)))
        return out

    def close(self):
        if self._h:
            lib().gs_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Renderer:
    """Renderer counterpart: one stream, one frame in flight."""

    def __init__(self, scene):
        self.scene = scene
        self._h = C.c_void_p()
        self._frame_hw = None  # (height, width) of the last frame handed to render / render_host: what contributions() checks against
        self._frames = 0       # frames handed to render / render_host: what a backward of differentiable_feature_maps checks against
        _check(lib().gs_renderer_create(scene._h, C.byref(self._h)))

    def render(self, uniforms, rgba_ptr=0, bgra_ptr=0):
        """Enqueue one frame into device buffers (raw pointers, e.g. tensor.data_ptr())."""
        _check(lib().gs_render(self._h, _p(uniforms), C.c_void_p(rgba_ptr), C.c_void_p(bgra_ptr)))
        self._frame_hw = (int(uniforms["height"][0]), int(uniforms["width"][0]))
        self._frames += 1

    def _frame_extent(self, entry, struct, asked=()):
        """(height, width) of the last frame for the checks of a pass over it; before any frame (None, None), extents that are not
        checked -- C refuses the call.  If one of `asked` is True then, there is no frame to size the allocation by: the refusal
        is obtained at once, from the pass's C entry point `entry` with an empty `struct`."""
        if self._frame_hw is not None:
            return self._frame_hw
        if any(v is True for v in asked):
            _check(getattr(lib(), entry)(self._h, C.byref(struct())))
        return None, None

    def contributions(self, weight=None, pixels=None, top_id=None, mask=None):
        """What every Gaussian contributed to the last frame (gs_accumulate_contributions), into torch tensors on the renderer's
        device, contiguous: weight int64 (N,) and pixels int32 (N,) are ADDED to -- the sum over the counted pixels that blend a
        Gaussian of q = round(alpha T 2^24), and the number of those pixels; top_id int32 (H, W) is overwritten with the scene id
        of the Gaussian of largest alpha T at each pixel, -1 where nothing was blended or the mask is 0; mask uint8 or bool
        (H, W): only pixels where it is not 0 are counted.  N = the scene's Gaussians, (H, W) = the last frame.  The arithmetic
        is the reference's (exp mode 2) whatever mode the frame was blended in.  Returns synchronised."""
        n = int(self.scene.num_vertices)
        h, w = self._frame_extent("gs_accumulate_contributions", Contributions)
        dev = self.scene.device
        c = Contributions()
        if weight is not None:
            c.weight = _tensor_exact("weight", weight, ("int64",), (n,), dev)
        if pixels is not None:
            c.pixels = _tensor_exact("pixels", pixels, ("int32",), (n,), dev)
        if top_id is not None:
            c.top_id = _tensor_exact("top_id", top_id, ("int32",), (h, w), dev)
        if mask is not None:
            c.mask = _tensor_exact("mask", mask, ("uint8", "bool"), (h, w), dev)
        _check(lib().gs_accumulate_contributions(self._h, C.byref(c)))

    def feature_maps(self, features=None, out=None, alpha=None, depth=None, median_depth=None):
        """Per-pixel maps of the last frame (gs_blend_features), into float32 torch tensors on the renderer's device, contiguous:
        out (H, W, C) = the rows of features (N, C) blended exactly as the colour is, alpha (H, W) = 1 - T, depth (H, W) = the
        expected view-space depth (NOT normalised: divide by alpha where alpha > 0), median_depth (H, W) = the depth of the entry
        that takes T below one half, +inf where none does.  Each output is a tensor to fill, True to have it allocated, or None
        to skip; all are overwritten.  N = the scene's Gaussians, (H, W) = the last frame, C <= 256.  The arithmetic is the
        reference's (exp mode 2) whatever mode the frame was blended in.  Returns synchronised, with a dict of the outputs
        that were asked for (keys out, alpha, depth, median_depth)."""
        owner = "Renderer.feature_maps"
        n = int(self.scene.num_vertices)
        dev = self.scene.device
        h, w = self._frame_extent("gs_blend_features", FeatureMaps, (out, alpha, depth, median_depth))
        m = FeatureMaps()
        channels = 0
        if features is not None:
            m.features = _tensor_exact("features", features, ("float32",), (n, None), dev, owner)
            channels = int(features.shape[1])
            if channels > FEATURE_CHANNELS_MAX:
                raise ValueError(f"features: {channels} channels, at most {FEATURE_CHANNELS_MAX} are blended in one call")
            if out is None:
                raise ValueError("out: features are given but no output for them (pass a tensor or True)")
        elif out is not None:
            raise ValueError("out: an output for blended features needs features")
        m.channels = channels
        result = _outputs(m, owner, dev, dict(out=_output(out, "out_features", "float32", (h, w, channels)),
                                              alpha=_output(alpha, "out_alpha", "float32", (h, w)),
                                              depth=_output(depth, "out_depth", "float32", (h, w)),
                                              median_depth=_output(median_depth, "out_depth_median", "float32", (h, w))))
        _check(lib().gs_blend_features(self._h, C.byref(m)))
        return result

    def lift_pixels(self, values, out=None, weight=None, mask=None):
        """Per-pixel values of the last frame carried back onto its Gaussians (gs_lift_pixels), the transpose of feature_maps:
        out (N, C) float64 += the sum over the counted pixels p that blend a Gaussian of w(p) * values[p], weight (N,) float64
        += the sum of w itself, w = fl32(alpha T) as in contributions.  values float32 (H, W, C), or None for a weights-only
        call; mask uint8 or bool (H, W): only pixels where it is not 0 are counted.  out and weight are each a tensor to ADD
        into, True to have zeros allocated, or None to skip.  All are contiguous torch tensors on the renderer's device -- plain
        device allocations, the adds are hardware float64 atomics.  N = the scene's Gaussians, (H, W) = the last frame,
        C <= 256.  The order of the adds is unspecified: two calls agree to rounding, not bit for bit.  The arithmetic is the
        reference's (exp mode 2) whatever mode the frame was blended in.  The pass runs on the renderer's own stream: the
        wrapper first waits for torch's current stream, so that whatever was queued there to produce values, mask, out or weight
        (the zeros of `True` included) is complete; producers on other streams are the caller's to order.  Returns
        synchronised, with a dict of what was asked for (keys out, weight)."""
        owner = "Renderer.lift_pixels"
        n = int(self.scene.num_vertices)
        dev = self.scene.device
        h, w = self._frame_extent("gs_lift_pixels", PixelLift, (out, weight))
        l = PixelLift()
        channels = 0
        if values is not None:
            l.values = _tensor_exact("values", values, ("float32",), (h, w, None), dev, owner)
            channels = int(values.shape[2])
            if channels > LIFT_CHANNELS_MAX:
                raise ValueError(f"values: {channels} channels, at most {LIFT_CHANNELS_MAX} are lifted in one call")
            if out is None and channels > 0:  # (values of no channels: there is nothing to lift, a weights-only call)
                raise ValueError("out: values are given but no output for them (pass a tensor or True)")
        elif out is not None:
            raise ValueError("out: an output for lifted values needs values")
        l.channels = channels
        if mask is not None:
            l.mask = _tensor_exact("mask", mask, ("uint8", "bool"), (h, w), dev, owner)
        result = _outputs(l, owner, dev, dict(out=_output(out, "out", "float64", (n, channels), zeros=True),
                                              weight=_output(weight, "out_weight", "float64", (n,), zeros=True)))
        _complete_callers_work(values, mask, *result.values())  # (the zeros allocated above among them: their fill is queued too)
        _check(lib().gs_lift_pixels(self._h, C.byref(l)))
        return result

    def blend_backward(self, grad_rgb, grad_alpha=None, colour=None, opacity=None, conic=None, uv=None):
        """The backward of the last frame's blend (gs_blend_backward): from grad_rgb float32 (H, W, 3) = dL/d(image RGB) and
        grad_alpha float32 (H, W) = dL/d(alpha of feature_maps), or None for zeros, the float64 sums per Gaussian colour (N, 3),
        opacity (N,), conic (N, 3) = c00 c01 c11 and uv (N, 2): the gradients with respect to the splat's rgb, its opacity, its
        conic and its screen position AS THE FRAME HOLDS THEM (stage("conic_opacity"), stage("uv_rg"), stage("b")), the walk's
        decisions taken as constants.  Each output is a tensor to ADD into, True to have zeros allocated, or None to skip; the
        conventions, the stream and the wait for torch's current stream are lift_pixels's.  The order of the adds is unspecified:
        two calls agree to rounding.  project_backward takes these four sums on to the trainer's parameters, and
        differentiable_render is both passes behind one autograd function.  Returns synchronised,
        with a dict of what was asked for (keys colour, opacity, conic, uv)."""
        owner = "Renderer.blend_backward"
        n = int(self.scene.num_vertices)
        dev = self.scene.device
        asked = dict(colour=colour, opacity=opacity, conic=conic, uv=uv)
        h, w = self._frame_extent("gs_blend_backward", BlendGrads, asked.values())
        g = BlendGrads()
        if grad_rgb is not None:
            g.grad_rgb = _tensor_exact("grad_rgb", grad_rgb, ("float32",), (h, w, 3), dev, owner)
        elif any(v is not None for v in asked.values()):
            raise ValueError("grad_rgb: an output is asked for but there is no grad_rgb")
        if grad_alpha is not None:
            g.grad_alpha = _tensor_exact("grad_alpha", grad_alpha, ("float32",), (h, w), dev, owner)
        result = _outputs(g, owner, dev, {name: _output(asked[name], "d_" + name, "float64", shape, zeros=True)
                                          for name, shape in _record_shapes(n).items()})
        _complete_callers_work(grad_rgb, grad_alpha, *result.values())  # (the zeros allocated above among them)
        _check(lib().gs_blend_backward(self._h, C.byref(g)))
        return result

    def project_backward(self, colour=None, opacity=None, conic=None, uv=None, out=None, sh_degree=3):
        """The projection half of the last frame's backward (gs_project_backward): from the float64 gradients per Gaussian with
        respect to its record -- colour (N, 3), opacity (N,), conic (N, 3), uv (N, 2), exactly what blend_backward returns; None =
        zeros -- the float64 gradients with respect to the six tensors Scene.to_tensors() returns.  out: a dict under
        from_tensors' keyword names (means (N, 3), log_scales (N, 3), quats (N, 4), opacity_logits (N,), sh_dc (N, 3), sh_rest
        (N, k, 3) with k in 0, 3, 8, 15) holding float64 tensors to ADD into -- a name it lacks or holds None for is skipped -- or
        None, and zeros are allocated for all six, sh_rest with the k of sh_degree.  Only the Gaussians the frame found visible
        are touched; the gradient is the one AT THE FRAME'S VALUES with the frame's decisions (culls, the clamp's branch, red's
        max(0, .)) as constants, and the scene must still hold what the frame rendered.  The stream and the wait for torch's
        current stream are lift_pixels's.  Returns synchronised, with the dict."""
        owner = "Renderer.project_backward"
        n = int(self.scene.num_vertices)
        dev = self.scene.device
        g = ProjectGrads()
        if out is None:
            if sh_degree not in SH_REST_COEFFS:
                raise ValueError(f"sh_degree must be 0, 1, 2 or 3, not {sh_degree!r}")
        else:
            unknown = sorted(set(out) - set(PARAMETER_NAMES))
            if unknown:
                raise TypeError(f"out: unknown member(s) {unknown}")
        _record_gradients(g, owner, n, dev, colour=colour, opacity=opacity, conic=conic, uv=uv)
        if out is None:
            import torch
            out = {name: torch.zeros(shape, dtype=torch.float64, device=_torch_device(dev))
                   for name, shape in _parameter_shapes(n, SH_REST_COEFFS[sh_degree]).items()}
        shapes = _parameter_shapes(n, None)
        for name in PARAMETER_NAMES:
            t = out.get(name)
            if t is None:
                continue
            ptr = _tensor_exact(name, t, ("float64",), shapes[name], dev, owner)
            if name == "sh_rest":
                k = int(t.shape[1])
                if k not in SH_REST_COEFFS.values():
                    raise ValueError(f"sh_rest: shape {tuple(int(d) for d in t.shape)} is not (rows, k, 3) with k in 0, 3, 8, 15")
                g.sh_rest_coeffs = k if ptr else 0
            setattr(g, "d_" + name, ptr)
        _complete_callers_work(colour, opacity, conic, uv, *[t for t in out.values() if t is not None])
        _check(lib().gs_project_backward(self._h, C.byref(g)))
        return out

    def visible_mask(self, out=None, accumulate=False):
        """The last frame's visibility as Scene.adam_step's mask (gs_visible_mask): a uint8 tensor (N,) on the scene's device, by
        scene id, 1 where stage("tiles") != 0.  out: the tensor to write (None: a new one); accumulate: OR into what `out` holds
        -- the union over a camera set (zero it once).  The stream and the wait for torch's current stream are lift_pixels's;
        raises GsError before any frame was rendered.  Returns synchronised, with the tensor."""
        n, dev = int(self.scene.num_vertices), self.scene.device
        mask = C.c_void_p()  # (its .value is the one member of this call's "struct")
        out = _outputs(mask, "Renderer.visible_mask", dev, dict(out=_output(True if out is None else out, "value", "uint8", (n,), zeros=True)))["out"]
        if mask.value is None:  # a scene of no Gaussians has no mask to write
            return out
        _complete_callers_work(out)
        _check(lib().gs_visible_mask(self._h, mask, C.c_int(1 if accumulate else 0)))
        return out

    def densify_stats(self, uv, stats):
        """The last frame's share of the statistic densify decides by (gs_accumulate_densify_stats): for every Gaussian the frame
        saw, grad_sum += the norm of its row of `uv` -- blend_backward's float64 (N, 2) sum for this frame -- scaled by half the
        frame's width and height (the Inria trainer's viewspace gradient norm), count += 1, max_radius = max(max_radius, its
        screen radius).  stats: the dict densify_stats_zeros(scene) allocates -- grad_sum float64 (N,), count int32 (N,) (uint32 is
        taken too: the same bits), max_radius float32 (N,).  An invisible Gaussian's elements are neither read nor written.  The
        stream and the wait for torch's current stream are lift_pixels's; raises GsError before any frame was rendered.  Returns
        synchronised, with stats."""
        owner = "Renderer.densify_stats"
        n, dev = int(self.scene.num_vertices), self.scene.device
        st = DensifyStats()
        st.d_uv = _tensor_exact("uv", uv, ("float64",), (n, 2), dev, owner)
        used = [uv] + _densify_stats(st, stats, n, dev, owner)
        if n == 0:  # a scene of no Gaussians has no statistic to keep
            return stats
        _complete_callers_work(*used)
        _check(lib().gs_accumulate_densify_stats(self._h, C.byref(st)))
        return stats

    def differentiable_render(self, uniforms, means, log_scales, quats, opacity_logits, sh_dc, sh_rest=None, want_alpha=False):
        """One frame as a torch.autograd.Function of the trainer's six parameter tensors (float32, on the renderer's device, as
        Scene.from_tensors takes them, one row per Gaussian of the scene): the forward refreshes the scene from them
        (update_from_tensors(0, ...); sh_rest None keeps the bands the scene holds), renders `uniforms` into a fresh tensor and
        synchronises; it returns rgb (H, W, 3), and with want_alpha also alpha (H, W) of feature_maps.  The backward is
        blend_backward then project_backward and returns the six gradients ROUNDED TO FLOAT32: the gradient AT THE FRAME'S VALUES
        -- the stored binary32 parameters, the records the frame holds -- WITH ITS DECISIONS AS CONSTANTS (visibility, the tile
        lists, the 1/255 and 1e-4 cuts, the 0.99 clamp, the Jacobian clamp's branch, red's max(0, .)).  The camera carries no
        gradient.  A backward after this renderer has been handed another frame raises RuntimeError instead of returning the
        gradient of a different frame; so one backward per forward, before the next forward."""
        return _autograd().render.apply(self, uniforms, bool(want_alpha), means, log_scales, quats, opacity_logits, sh_dc, sh_rest)

    def camera_backward(self, colour=None, opacity=None, conic=None, uv=None, view_mat=True, proj_mat=True, camera_position=True):
        """The camera half of the last frame's backward (gs_camera_backward): from the same four float64 per-Gaussian gradients
        project_backward takes (what blend_backward returns; None = zeros) the float64 gradients with respect to the frame's
        uniforms, summed over its visible Gaussians: view_mat (16,) and proj_mat (16,) laid out as the uniforms' matrices
        (element 4 c + r; row 3 of view_mat and row 2 of proj_mat are not touched), camera_position (3,).  Each output is a
        tensor to ADD into, True to have zeros allocated, or None to skip.  The gradient is the one AT THE FRAME'S VALUES with the
        frame's decisions as constants; the intrinsics carry none.  No atomics: two calls give the same bits.  The stream and the
        wait for torch's current stream are lift_pixels's.  camera_pose_gradient carries the result on to a camera's position
        and rotation; differentiable_render_posed is all of it behind one autograd function.  Returns
        synchronised, with a dict of what was asked for (keys view_mat, proj_mat, camera_position)."""
        owner = "Renderer.camera_backward"
        n = int(self.scene.num_vertices)
        dev = self.scene.device
        g = CameraGrads()
        _record_gradients(g, owner, n, dev, colour=colour, opacity=opacity, conic=conic, uv=uv)
        result = _outputs(g, owner, dev, dict(view_mat=_output(view_mat, "d_view_mat", "float64", (16,), zeros=True),
                                              proj_mat=_output(proj_mat, "d_proj_mat", "float64", (16,), zeros=True),
                                              camera_position=_output(camera_position, "d_camera_position", "float64", (3,), zeros=True)))
        _complete_callers_work(colour, opacity, conic, uv, *result.values())  # (the zeros allocated above among them)
        _check(lib().gs_camera_backward(self._h, C.byref(g)))
        return result

    def photometric_loss(self, image, target, lambda_dssim=0.2, grad=True, terms=True):
        """The trainer's loss of `image` against `target` and its image gradient (gs_photometric_loss):
        loss = (1 - lambda_dssim) L1 + lambda_dssim (1 - SSIM), 11 x 11 Gaussian window of sigma 1.5, zeros outside the image
        (the Inria loss_utils.ssim / fused-ssim convention), evaluated in binary64.  image and target: float32 device tensors
        (H, W, 3) or (H, W, 4), contiguous, of one H and W; the pixel stride is the last dimension, so a frame rendered into an
        RGBA tensor goes in uncopied (its fourth float is never read).  The size is NOT tied to the renderer's last frame, which
        the call neither reads nor changes.  grad: a float32 (H, W, 3) tensor to WRITE d loss / d image into -- exactly what
        blend_backward takes --, True to have one allocated, or None: forward only.  terms: a float64 (4,) tensor to WRITE
        loss, l1, ssim, mse into, True, or None.  lambda_dssim == 0 runs one pass without the window and writes ssim as NaN.
        No atomics: two calls give the same bits.  The call is ordered behind this renderer's queued frames (so `image` may be
        the target of a render that has not been synchronised) and waits for torch's current stream as lift_pixels does.
        Returns synchronised, with a dict: loss (a 0-dim float64 view of terms[0]; None without terms), terms, grad_rgb."""
        owner = "Renderer.photometric_loss"
        dev = self.scene.device
        lam = float(lambda_dssim)
        if not 0.0 <= lam <= 1.0:
            raise ValueError(f"lambda_dssim must lie in [0, 1], not {lambda_dssim!r}")
        l = PhotoLoss()
        l.lambda_dssim = lam
        shape = tuple(int(d) for d in getattr(image, "shape", ()))
        if len(shape) != 3 or shape[2] not in (3, 4):
            raise ValueError(f"image: shape {shape} is not (H, W, 3) or (H, W, 4)")
        h, w = shape[:2]
        if not (1 <= h <= PHOTO_LOSS_MAX_EXTENT and 1 <= w <= PHOTO_LOSS_MAX_EXTENT):
            raise ValueError(f"image: height and width must be 1 .. {PHOTO_LOSS_MAX_EXTENT}, not {h} and {w}")
        tshape = tuple(int(d) for d in getattr(target, "shape", ()))
        if len(tshape) != 3 or tshape[2] not in (3, 4):
            raise ValueError(f"target: shape {tshape} is not ({h}, {w}, 3) or ({h}, {w}, 4)")
        l.image = _tensor_exact("image", image, ("float32",), (h, w, shape[2]), dev, owner)
        l.target = _tensor_exact("target", target, ("float32",), (h, w, tshape[2]), dev, owner)
        l.width, l.height, l.image_stride, l.target_stride = w, h, shape[2], tshape[2]
        result = dict(loss=None, terms=None, grad_rgb=None)
        result.update(_outputs(l, owner, dev, dict(grad=_output(grad, "grad_rgb", "float32", (h, w, 3), key="grad_rgb"),
                                                   terms=_output(terms, "terms", "float64", (4,)))))
        _complete_callers_work(image, target, result["grad_rgb"], result["terms"])
        _check(lib().gs_photometric_loss(self._h, C.byref(l)))
        if terms is not None:
            result["loss"] = result["terms"][0]
        return result

    def differentiable_photometric_loss(self, image, target, lambda_dssim=0.2):
        """photometric_loss as a torch.autograd.Function of `image`: returns the loss as a 0-dim float64 device tensor; the
        forward makes ONE call for the loss and d loss / d image and keeps the gradient, the backward returns
        grad_output.float() * that gradient for `image` (zeros for the fourth float of an RGBA image) and nothing for `target`.
        It does not involve the renderer's last frame, so the "one backward per forward" rule of differentiable_render does not
        bind it.  A trainer's step:
            rgb = rend.differentiable_render(u, **params)
            rend.differentiable_photometric_loss(rgb, photo).backward()"""
        return _autograd().photometric_loss.apply(self, float(lambda_dssim), image, target)

    def differentiable_render_posed(self, width, height, position, rotation, means=None, log_scales=None, quats=None, opacity_logits=None,
                                    sh_dc=None, sh_rest=None, fov=45.0, near=0.1, far=1000.0, want_alpha=False):
        """One frame as a torch.autograd.Function of the camera's pose -- position (3,) and rotation (4,) (w x y z), torch tensors
        on any device, float32 or float64 -- and, where given, of the six scene tensors of differentiable_render.  The forward
        builds make_camera / camera_uniforms from the pose's values ROUNDED TO FLOAT32 (the quaternion as it is, not normalised),
        refreshes the scene from whichever of the six tensors are given (all None: the scene stays as it is), renders and
        synchronises; it returns rgb (H, W, 3), and with want_alpha also alpha (H, W).  The backward is blend_backward, then
        camera_backward and camera_pose_gradient for the pose, returned in the leaves' dtype and on their device, and
        project_backward only if a scene tensor requires a gradient.  The gradient is the one AT THE FRAME'S VALUES with its
        decisions as constants, as differentiable_render states it; rotation's is that of the RAW quaternion (an optimiser that
        normalises after each step needs no more; fov, near and far carry none).  One backward per forward, before the next
        forward: a backward after this renderer has been handed another frame raises RuntimeError."""
        return _autograd().render_posed.apply(self, int(width), int(height), float(fov), float(near), float(far), bool(want_alpha),
                                              position, rotation, means, log_scales, quats, opacity_logits, sh_dc, sh_rest)

    def differentiable_feature_maps(self, features):
        """feature_maps(features)["out"] as a torch.autograd.Function: features (N, C) float32 on the renderer's device -> the
        (H, W, C) blended map of the last frame, differentiable with respect to `features` ONLY.  The frame -- positions,
        opacities, covariances, the camera -- is a constant: the map is linear in features, and the backward is its transpose,
        lift_pixels of the incoming gradient, rounded to float32.  A backward after this renderer has been handed another frame
        raises RuntimeError instead of returning the gradient of a different frame."""
        return _autograd().feature_maps.apply(self, features)

    def render_host(self, uniforms, want_rgba=True, want_bgra=False):
        h, w = int(uniforms["height"][0]), int(uniforms["width"][0])
        rgba = np.zeros((h, w, 4), np.float32) if want_rgba else None
        bgra = np.zeros((h, w, 4), np.uint8) if want_bgra else None
        _check(lib().gs_render_host(self._h, _p(uniforms), _p(rgba) if want_rgba else None,
                                    _p(bgra) if want_bgra else None))
        self._frame_hw = (h, w)
        self._frames += 1
        return rgba, bgra

    def synchronize(self):
        _check(lib().gs_synchronize(self._h))

    def set_timing(self, enabled):
        _check(lib().gs_set_timing(self._h, C.c_int(int(enabled))))

    def set_frames_in_flight(self, frames):
        _check(lib().gs_set_frames_in_flight(self._h, C.c_int(int(frames))))

    def set_exp_mode(self, mode):
        """3 (default) v_exp_f32 under the guard of render.comp:82 (the reference's decisions, its pixels to rounding noise), 2 libm's expf
        restated in binary64 (the reference's bits), 0 pipeline-defined polynomial, 1 v_exp_f32 unguarded (gs_set_exp_mode)."""
        _check(lib().gs_set_exp_mode(self._h, C.c_int(int(mode))))

    def set_blend_contraction(self, enabled):
        """False (default): render.comp:66,87 as written; True: the three FMA contractions GLSL permits (gs_set_blend_contraction)."""
        _check(lib().gs_set_blend_contraction(self._h, C.c_int(int(bool(enabled)))))

    def set_antialiased(self, enabled):
        """True: the antialiased mode -- each splat's opacity scaled by sqrt(det(cov2D) / det(cov2D + 0.3 I)), as scenes trained
        with antialiased rasterisation expect; False (default): the reference's pipeline (gs_set_antialiased)."""
        _check(lib().gs_set_antialiased(self._h, C.c_int(int(bool(enabled)))))

    @property
    def antialiased(self):
        """Whether the antialiased mode is on (gs_get_antialiased)."""
        rc = lib().gs_get_antialiased(self._h)
        _check(min(rc, 0))
        return bool(rc)

    def set_fast_blend(self, fast):
        """True: both opt-in relaxations (polynomial exp, contractions); False: exp mode 2 as written, bit-identical to the reference text."""
        self.set_exp_mode(0 if fast else 2)
        self.set_blend_contraction(bool(fast))

    def set_graph_mode(self, enabled):
        """Replay frames as captured HIP graphs (gs_set_graph_mode)."""
        _check(lib().gs_set_graph_mode(self._h, C.c_int(int(bool(enabled)))))

    def set_blend_lockstep(self, mode):
        """-1 automatic (measured), 0 off, 1 on: the tile's four waves take every chunk together (gs_set_blend_lockstep)."""
        _check(lib().gs_set_blend_lockstep(self._h, C.c_int(int(mode))))

    def blend_lockstep(self):
        """(the setting the next frame runs with, whether the measurement has settled)."""
        settled = C.c_int(0)
        now = lib().gs_get_blend_lockstep(self._h, C.byref(settled))
        if now < 0:
            _check(now)
        return bool(now), bool(settled.value)

    def set_level1_fused(self, mode):
        """-1 by rule, 0 off, 1 on: k_preprocess files the level-1 candidates itself (gs_set_level1_fused; GS_L1_FUSED at creation)."""
        _check(lib().gs_set_level1_fused(self._h, C.c_int(int(mode))))

    def level1_fused(self):
        """True: the most recently enqueued frame took the one-pass level 1 (gs_get_level1_fused)."""
        now = lib().gs_get_level1_fused(self._h)
        if now < 0:
            _check(now)
        return bool(now)

    def set_tile_cull(self, on):
        """The alpha-cut tile cull (gs_set_tile_cull; GS_TILE_CULL at creation, default on)."""
        _check(lib().gs_set_tile_cull(self._h, C.c_int(1 if on else 0)))

    def tile_cull(self):
        """(the switch, whether the most recently enqueued frame's lists are culled) (gs_get_tile_cull)."""
        culled = C.c_int(0)
        now = lib().gs_get_tile_cull(self._h, C.byref(culled))
        if now < 0:
            _check(now)
        return bool(now), bool(culled.value)

    def listed_instances(self):
        """Tile instances in the last frame's lists as the blend walked them (gs_get_listed_instances)."""
        out = C.c_uint64(0)
        _check(lib().gs_get_listed_instances(self._h, C.byref(out)))
        return int(out.value)

    def set_sort_path(self, mode):
        """0 automatic, 1 global depth order, 2 bin-local (gs_set_sort_path)."""
        _check(lib().gs_set_sort_path(self._h, C.c_int(int(mode))))

    def timing_totals(self, reset=True):
        """(sums of per-pass ms as FrameStats, number of frames summed)."""
        st = FrameStats()
        n = C.c_uint64()
        _check(lib().gs_get_timing_totals(self._h, C.byref(st), C.byref(n), C.c_int(int(reset))))
        return st, n.value

    def frame_intervals(self, reset=True, capacity=8192):
        """ms between the completions of consecutive frames (GPU timestamps), oldest first."""
        out = np.zeros(capacity, np.float32)
        n = C.c_uint64()
        _check(lib().gs_get_frame_intervals(self._h, _p(out), C.c_uint64(capacity), C.byref(n), C.c_int(int(reset))))
        return out[:min(capacity, n.value)].copy()

    def stats(self):
        st = FrameStats()
        _check(lib().gs_get_stats(self._h, C.byref(st)))
        return st

    def poll_stats(self):
        """(stats of the most recently retired frame, frames retired so far) without waiting (gs_poll_stats)."""
        st = FrameStats()
        n = C.c_uint64()
        _check(lib().gs_poll_stats(self._h, C.byref(st), C.byref(n)))
        return st, n.value

    def stage(self, name, uniforms=None):
        """Download a stage buffer of the last frame as a numpy array."""
        code, dt = STAGES[name]
        st = self.stats()
        n, v, d = st.num_gaussians, st.num_visible, min(st.num_instances, st.instance_capacity)
        count = {"tiles": n, "depth": n, "radius": n, "aabb": 4 * n, "conic_opacity": 4 * n, "uv_rg": 4 * n,
                 "b": n, "alpha_cut": n, "depth_order": v, "sorted_tile": d, "sorted_gid": d, "lists_raw": d}.get(name)
        if name == "lists_culled":
            count = min(self.listed_instances(), st.instance_capacity)
        if name in ("ranges", "ranges_raw", "ranges_culled"):
            w, h = int(uniforms["width"][0]), int(uniforms["height"][0])
            count = 2 * ((w + 15) // 16) * ((h + 15) // 16)
        out = np.zeros(max(int(count), 1), dt)
        _check(lib().gs_debug_download(self._h, C.c_int(code), _p(out), C.c_uint64(int(count) * out.itemsize)))
        return out[:int(count)]

    @property
    def stream(self):
        return lib().gs_renderer_stream(self._h)

    def close(self):
        if self._h:
            lib().gs_renderer_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Adam:
    """The optimiser of a trainer on this rasteriser: the moments and the step count around Scene.adam_step.
    params: {name: float32 device tensor} under from_tensors' names -- the tensors the scene was built from; they are updated
    in place and the scene with them.  lr: a float or a dict per name.  A sparse Adam: step(mask=...) moves the masked Gaussians
    only and the others' moments do not decay."""

    def __init__(self, scene, params, lr, betas=(0.9, 0.999), eps=1e-15):
        import torch
        self.scene, self.lr, self.betas, self.eps, self.t = scene, lr, tuple(betas), eps, 0
        self.params = {k: v for k, v in params.items() if v is not None}
        self.state = dict(exp_avg={k: torch.zeros_like(v, dtype=torch.float32) for k, v in self.params.items()},
                          exp_avg_sq={k: torch.zeros_like(v, dtype=torch.float32) for k, v in self.params.items()})

    def step(self, grads, mask=None, zero_grads=True):
        """One step with the float64 gradients `grads` (a dict under the same names as params); see Scene.adam_step."""
        self.t += 1
        try:
            self.scene.adam_step(self.params, grads, self.state["exp_avg"], self.state["exp_avg_sq"], self.lr, self.betas, self.eps,
                                 self.t, mask=mask, zero_grads=zero_grads)
        except Exception:
            self.t -= 1  # a refused step is no step
            raise

    def densify(self, rule, stats, noise=None):
        """Adaptive density control of the optimiser's model (densify): the parameters and the moments are
        replaced by the densified ones, a NEW scene is built from them (Scene.from_tensors) and returned; self.scene, self.params
        and self.state are replaced, the step count stays.  The old scene and its renderers stay valid until the caller closes
        them; make a new Renderer and new statistics (densify_stats_zeros) for the new scene.  The optimiser must hold the whole
        model (every tensor Scene.from_tensors requires), since all of it is compacted.  What happened: self.densify_info."""
        new_params, new_state, info = densify(self.scene, self.params, rule, stats, self.state, noise)
        scene = Scene.from_tensors(**new_params, device=self.scene.device)
        self.scene, self.params, self.state, self.densify_info = scene, new_params, new_state, info
        return scene

    def reset_opacity(self, ceiling=0.01):
        """The trainers' opacity reset: opacity_logits <- min(logit, logit(ceiling)), both opacity moments zeroed, the scene's
        opacity plane refreshed (Scene.update_from_tensors).  Synchronize every renderer of the scene first."""
        import math
        if not 0.0 < float(ceiling) < 1.0:
            raise ValueError(f"ceiling must lie in (0, 1), not {ceiling!r}")
        logits = self.params["opacity_logits"]
        logits.clamp_(max=math.log(float(ceiling) / (1.0 - float(ceiling))))
        self.state["exp_avg"]["opacity_logits"].zero_()
        self.state["exp_avg_sq"]["opacity_logits"].zero_()
        self.scene.update_from_tensors(0, opacity_logits=logits, device=self.scene.device)


class Dist:
    """One process per GPU: RCCL communicator + the one scene broadcast (gs_dist_*, include/gs3d_hip.h)."""

    ID_BYTES = 128

    @staticmethod
    def unique_id():
        buf = (C.c_uint8 * Dist.ID_BYTES)()
        _check(lib().gs_dist_unique_id(buf))
        return bytes(buf)

    def __init__(self, unique_id, rank, world, device=0):
        h = C.c_void_p()
        buf = (C.c_uint8 * Dist.ID_BYTES).from_buffer_copy(unique_id)
        _check(lib().gs_dist_create(buf, C.c_int(rank), C.c_int(world), C.c_int(device), C.byref(h)))
        self._h = h
        lib().gs_dist_pose_count.restype = C.c_uint64

    @property
    def rank(self):
        return lib().gs_dist_rank(self._h)

    @property
    def world(self):
        return lib().gs_dist_world(self._h)

    def pose_count(self, poses):
        return int(lib().gs_dist_pose_count(self._h, C.c_uint64(poses)))

    def broadcast_scene(self, scene=None, root=0, copy_on_root=False):
        """Root passes its Scene and gets it back (or, with copy_on_root, a new replica like every other rank); the other
        ranks get a new Scene holding the received blob.  A quantised root scene arrives quantised."""
        out = C.c_void_p()
        _check(lib().gs_dist_broadcast_scene_ex(self._h, scene._h if scene is not None else None, C.c_int(root),
                                                C.c_uint(1 if copy_on_root else 0), C.byref(out)))
        if scene is not None and out.value == scene._h.value:
            return scene
        return Scene(out)

    def close(self):
        if self._h:
            lib().gs_dist_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
