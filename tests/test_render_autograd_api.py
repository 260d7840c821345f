"""Renderer.differentiable_render and Renderer.differentiable_render_posed without a GPU: which methods of the renderer the two
autograd functions call, in which order and with what, and what they return for every input.  The renderer's seven methods are
recording stubs that return small fixed tensors (in the manner of _dense_renderer in tests/test_lift_api.py), the tensors live
on the CPU (binding._torch_device is patched), and only the host arithmetic of the C library (camera_uniforms,
camera_pose_gradient) is real.  The numbers are pinned on the GPU (tests/test_gpu_project_backward.py, section 7;
tests/test_gpu_camera_backward.py, section 4)."""
import ctypes as C

import numpy as np
import pytest

from helpers import hand_made_renderer

torch = pytest.importorskip("torch")

N, H, W = 5, 3, 4
NAMES = ("means", "log_scales", "quats", "opacity_logits", "sh_dc", "sh_rest")
FIVE = NAMES[:5]
RECORD = dict(colour=(N, 3), opacity=(N,), conic=(N, 3), uv=(N, 2))
UNIFORM_GRADS = dict(view_mat=(16,), proj_mat=(16,), camera_position=(3,))
F32, F64 = torch.float32, torch.float64


def _fixed(shape, seed):
    """A float64 tensor no element of which is a float32: what the stubs add, so that the rounding of the result shows."""
    count = int(np.prod(shape, dtype=np.int64))
    return ((torch.arange(count, dtype=F64) + seed) * (1.0 + 2.0 ** -30) + 2.0 ** -40).reshape(shape)


def _rounded(name, shape, into):
    """The gradient the functions must return for parameter `name`: what the project_backward stub added, rounded to float32."""
    want = _fixed(shape, NAMES.index(name) + 1)
    assert not torch.equal(want.to(F32).double(), want)
    return want.to(F32).reshape(into)


def _stub_renderer(pkg, monkeypatch):
    """(renderer, calls): calls is the list of (method, what it was given) in the order the methods were reached."""
    monkeypatch.setattr(pkg.binding, "_torch_device", lambda dev: "cpu")
    rend = hand_made_renderer(pkg, n=N, frame_hw=None, frames=0)
    calls = []

    def synchronize():
        calls.append(("synchronize", None))

    def update_from_tensors(first, **given):
        assert first == 0 and tuple(given) == NAMES
        assert all(t is None or (not t.requires_grad and t.is_contiguous()) for t in given.values())
        calls.append(("update_from_tensors", tuple(k for k, t in given.items() if t is not None)))

    def render(uniforms, rgba_ptr=0, bgra_ptr=0):
        h, w = int(uniforms["height"][0]), int(uniforms["width"][0])
        C.memset(rgba_ptr, 0, h * w * 16)            # the frame is a fresh float32 (h, w, 4) tensor: black
        rend._frame_hw, rend._frames = (h, w), rend._frames + 1
        calls.append(("render", (h, w)))

    def feature_maps(features=None, out=None, alpha=None, depth=None, median_depth=None):
        assert features is None and out is None and alpha is True and depth is None and median_depth is None
        calls.append(("feature_maps", None))
        return dict(alpha=_fixed(rend._frame_hw, 3).to(F32))

    def blend_backward(grad_rgb, grad_alpha=None, colour=None, opacity=None, conic=None, uv=None):
        assert (colour, opacity, conic, uv) == (True, True, True, True)
        for g, shape in ((grad_rgb, rend._frame_hw + (3,)), (grad_alpha, rend._frame_hw)):
            assert g is None or (g.dtype == F32 and g.is_contiguous() and tuple(g.shape) == shape and g.device.type == "cpu")
        calls.append(("blend_backward", (grad_rgb.clone(), None if grad_alpha is None else grad_alpha.clone())))
        return {name: _fixed(shape, 7) for name, shape in RECORD.items()}

    def check_record(d):
        assert tuple(d) == tuple(RECORD)
        assert all(torch.equal(d[name], _fixed(shape, 7)) for name, shape in RECORD.items())

    def project_backward(colour=None, opacity=None, conic=None, uv=None, out=None, sh_degree=3):
        check_record(dict(colour=colour, opacity=opacity, conic=conic, uv=uv))
        for name, t in out.items():                  # float64 zeros on the scene's device, one row per Gaussian
            assert t.dtype == F64 and t.device.type == "cpu" and t.shape[0] == N and not t.any(), name
            t += _fixed(tuple(t.shape), NAMES.index(name) + 1)
        calls.append(("project_backward", {name: tuple(t.shape) for name, t in out.items()}))
        return out

    def camera_backward(colour=None, opacity=None, conic=None, uv=None, view_mat=True, proj_mat=True, camera_position=True):
        check_record(dict(colour=colour, opacity=opacity, conic=conic, uv=uv))
        assert (view_mat, proj_mat, camera_position) == (True, True, True)
        calls.append(("camera_backward", None))
        return {name: _fixed(shape, 11) for name, shape in UNIFORM_GRADS.items()}

    for stub in (synchronize, render, feature_maps, blend_backward, project_backward, camera_backward):
        monkeypatch.setattr(rend, stub.__name__, stub, raising=False)
    monkeypatch.setattr(rend.scene, "update_from_tensors", update_from_tensors, raising=False)
    return rend, calls


def _params(k=3, requires=NAMES, flat=True):
    """The six parameter tensors; sh_rest with k coefficients (None: no sh_rest); flat False: the Inria trainer's (N, 1) and (N, 1, 3)."""
    shapes = dict(means=(N, 3), log_scales=(N, 3), quats=(N, 4), opacity_logits=(N,) if flat else (N, 1),
                  sh_dc=(N, 3) if flat else (N, 1, 3), sh_rest=None if k is None else (N, k, 3))
    return {name: None if shape is None else torch.ones(shape, dtype=F32, requires_grad=name in requires) for name, shape in shapes.items()}


def _names(calls):
    return [name for name, _ in calls]


def _uniforms(pkg):
    return pkg.camera_uniforms(pkg.make_camera(), W, H)


# ------------------------------------------------------------------------------------------------ differentiable_render
PLAIN = {"all six": dict(k=3), "the trainer's shapes": dict(k=15, flat=False), "means only": dict(k=8, requires=("means",)),
         "sh_rest of k = 0": dict(k=0), "no sh_rest": dict(k=None), "sh_rest only": dict(k=3, requires=("sh_rest",))}


@pytest.mark.parametrize("case", sorted(PLAIN))
@pytest.mark.parametrize("want_alpha", [False, True], ids=["rgb", "rgb and alpha"])
def test_render_calls_the_renderer_in_order_and_returns_every_given_gradient(pkg, monkeypatch, case, want_alpha):
    rend, calls = _stub_renderer(pkg, monkeypatch)
    params = _params(**PLAIN[case])
    k = PLAIN[case]["k"]
    given = tuple(name for name in NAMES if params[name] is not None)
    got = rend.differentiable_render(_uniforms(pkg), **params, want_alpha=want_alpha)
    forward = ["synchronize", "update_from_tensors", "render", "synchronize"] + (["feature_maps"] if want_alpha else [])
    assert _names(calls) == forward
    assert calls[1][1] == given and calls[2][1] == (H, W)       # the scene is refreshed always, from every tensor given
    rgb, alpha = got if want_alpha else (got, None)
    assert rgb.shape == (H, W, 3) and rgb.dtype == F32 and rgb.is_contiguous() and rgb.requires_grad and not rgb.detach().any()
    if want_alpha:
        assert torch.equal(alpha.detach(), _fixed((H, W), 3).to(F32)) and alpha.requires_grad
    leaves = [params[name] for name in given if params[name].requires_grad]
    asked = [name for name in given if params[name].requires_grad]
    g_rgb, g_alpha = _fixed((W, H, 3), 5).to(F32).permute(1, 0, 2), _fixed((H, W), 6).to(F32)   # (not contiguous: made so on the way)
    if want_alpha:
        grads = torch.autograd.grad([rgb, alpha], leaves, [g_rgb, g_alpha], allow_unused=True)
    else:
        grads = torch.autograd.grad([rgb], leaves, [g_rgb], allow_unused=True)
    assert _names(calls) == forward + ["blend_backward", "project_backward"]
    seen_rgb, seen_alpha = calls[-2][1]
    assert torch.equal(seen_rgb, g_rgb) and (torch.equal(seen_alpha, g_alpha) if want_alpha else seen_alpha is None)
    # zeros are allocated for the five and, unless it has no coefficients, for a given sh_rest -- whether or not each asks
    want_out = {name: tuple(params[name].reshape(N, -1, 3).shape) if name == "sh_rest" else (N,) + {"quats": (4,), "opacity_logits": ()}.get(name, (3,))
                for name in given if name != "sh_rest" or k}
    assert calls[-1][1] == want_out and list(calls[-1][1]) == list(want_out)
    for name, g in zip(asked, grads):
        assert g is not None and g.dtype == F32 and g.shape == params[name].shape and g.device.type == "cpu", name
        if name == "sh_rest" and not k:
            assert g.shape == (N, 0, 3)                         # no coefficients: float32 zeros, nothing of project_backward
        else:
            assert torch.equal(g, _rounded(name, want_out[name], params[name].shape)), name


def test_render_with_only_alpha_used_hands_blend_backward_zeros_for_rgb(pkg, monkeypatch):
    rend, calls = _stub_renderer(pkg, monkeypatch)
    params = _params()
    rgb, alpha = rend.differentiable_render(_uniforms(pkg), **params, want_alpha=True)
    (g,) = torch.autograd.grad([alpha], [params["means"]], [torch.ones(H, W, dtype=F32)])
    seen_rgb, seen_alpha = calls[-2][1]
    assert seen_rgb.shape == (H, W, 3) and seen_rgb.dtype == F32 and not seen_rgb.any()
    assert seen_alpha.dtype == F32 and torch.equal(seen_alpha, torch.ones(H, W))
    assert torch.equal(g, _rounded("means", (N, 3), (N, 3)))


def test_a_render_backward_after_another_frame_raises(pkg, monkeypatch):
    rend, calls = _stub_renderer(pkg, monkeypatch)
    params, u = _params(), _uniforms(pkg)
    rgb = rend.differentiable_render(u, **params)
    other = torch.empty((H, W, 4), dtype=F32)
    rend.render(u, other.data_ptr())             # another frame: the lists the forward walked are gone
    with pytest.raises(RuntimeError) as e:
        rgb.sum().backward()
    assert str(e.value) == ("differentiable_render: the forward rendered frame 1 of this renderer, which has rendered frame 2 since; "
                            "the gradient of another frame is not returned")
    assert "blend_backward" not in _names(calls) and params["means"].grad is None
    rend.differentiable_render(u, **params).sum().backward()   # forward again on the new frame: the backward goes through
    assert _names(calls)[-2:] == ["blend_backward", "project_backward"] and params["means"].grad is not None


# ------------------------------------------------------------------------------------------------ differentiable_render_posed
def _pose(dtype=F32, requires=(True, True), row=False):
    position = torch.tensor([[0.25, -0.5, 1.0]] if row else [0.25, -0.5, 1.0], dtype=dtype, requires_grad=requires[0])
    rotation = torch.tensor([0.9, 0.1, -0.2, 0.3], dtype=dtype, requires_grad=requires[1])
    return position, rotation


def _pose_gradient(pkg, position, rotation):
    """What camera_pose_gradient makes of the camera_backward stub's sums at this pose."""
    cam = pkg.make_camera(position=position.detach().float().numpy().reshape(-1), rotation=rotation.detach().float().numpy(), fov=50.0)
    return pkg.binding.camera_pose_gradient(cam, W, H, {name: _fixed(shape, 11) for name, shape in UNIFORM_GRADS.items()})


POSED = {"pose only": dict(pose={}, k=None, requires=(), scene=False),
         "pose only, float64 row": dict(pose=dict(dtype=F64, row=True), k=None, requires=(), scene=False),
         "position only": dict(pose=dict(requires=(True, False)), k=None, requires=(), scene=False),
         "scene only": dict(pose=dict(requires=(False, False)), k=3, requires=("means", "quats", "sh_rest")),
         "scene given, pose asks": dict(pose={}, k=3, requires=()),
         "pose and scene": dict(pose=dict(dtype=F64), k=15, requires=NAMES, flat=False),
         "sh_rest of k = 0": dict(pose={}, k=0, requires=("sh_dc", "sh_rest")),
         "no sh_rest": dict(pose=dict(requires=(False, True)), k=None, requires=FIVE)}


@pytest.mark.parametrize("case", sorted(POSED))
@pytest.mark.parametrize("want_alpha", [False, True], ids=["rgb", "rgb and alpha"])
def test_render_posed_calls_the_renderer_in_order_and_returns_what_is_asked_for(pkg, monkeypatch, case, want_alpha):
    rend, calls = _stub_renderer(pkg, monkeypatch)
    spec = POSED[case]
    k = spec["k"]
    position, rotation = _pose(**spec["pose"])
    params = _params(k, spec["requires"], spec.get("flat", True)) if spec.get("scene", True) else dict.fromkeys(NAMES)
    given = tuple(name for name in NAMES if params[name] is not None)
    got = rend.differentiable_render_posed(W, H, position, rotation, **params, fov=50.0, want_alpha=want_alpha)
    # the scene is refreshed only if a tensor is given
    forward = ["synchronize"] + (["update_from_tensors"] if given else []) + ["render", "synchronize"] + (["feature_maps"] if want_alpha else [])
    assert _names(calls) == forward
    assert not given or calls[1][1] == given
    assert dict(calls)["render"] == (H, W)
    rgb, alpha = got if want_alpha else (got, None)
    assert rgb.shape == (H, W, 3) and rgb.dtype == F32 and rgb.requires_grad
    asked = [name for name in given if params[name].requires_grad]
    leaves = [t for t in (position, rotation) if t.requires_grad] + [params[name] for name in asked]
    g_rgb, g_alpha = _fixed((W, H, 3), 5).to(F32).permute(1, 0, 2), _fixed((H, W), 6).to(F32)
    if want_alpha:
        grads = list(torch.autograd.grad([rgb, alpha], leaves, [g_rgb, g_alpha], allow_unused=True))
    else:
        grads = list(torch.autograd.grad([rgb], leaves, [g_rgb], allow_unused=True))
    pose_asks = position.requires_grad or rotation.requires_grad
    assert _names(calls) == forward + ["blend_backward"] + (["camera_backward"] if pose_asks else []) + (["project_backward"] if asked else [])
    seen_rgb, seen_alpha = dict(calls)["blend_backward"]
    assert torch.equal(seen_rgb, g_rgb) and (torch.equal(seen_alpha, g_alpha) if want_alpha else seen_alpha is None)
    # the pose's gradients: camera_pose_gradient of camera_backward's sums, in the leaves' dtype, shape and device
    found = _pose_gradient(pkg, position, rotation)
    for leaf, want in zip((position, rotation), found):
        if leaf.requires_grad:
            g = grads.pop(0)
            assert g.dtype == leaf.dtype and g.shape == leaf.shape and g.device == leaf.device
            assert torch.equal(g, torch.as_tensor(want).to(leaf.dtype).reshape(leaf.shape)) and g.abs().sum() > 0
    # zeros are allocated only where a gradient is asked for, and not for an sh_rest of no coefficients
    if asked:
        want_out = {name: tuple(params[name].reshape(N, -1, 3).shape) if name == "sh_rest" else (N,) + {"quats": (4,), "opacity_logits": ()}.get(name, (3,))
                    for name in asked if name != "sh_rest" or k}
        assert calls[-1][1] == want_out and list(calls[-1][1]) == list(want_out)
    assert len(grads) == len(asked)
    for name, g in zip(asked, grads):
        assert g is not None and g.dtype == F32 and g.shape == params[name].shape and g.device.type == "cpu", name
        if name == "sh_rest" and not k:
            assert g.shape == (N, 0, 3)
        else:
            assert torch.equal(g, _rounded(name, want_out[name], params[name].shape)), name


def test_render_posed_with_only_alpha_used_hands_blend_backward_zeros_for_rgb(pkg, monkeypatch):
    rend, calls = _stub_renderer(pkg, monkeypatch)
    position, rotation = _pose()
    rgb, alpha = rend.differentiable_render_posed(W, H, position, rotation, fov=50.0, want_alpha=True)
    (g,) = torch.autograd.grad([alpha], [position], [torch.ones(H, W, dtype=F32)])
    seen_rgb, seen_alpha = dict(calls)["blend_backward"]
    assert seen_rgb.shape == (H, W, 3) and seen_rgb.dtype == F32 and not seen_rgb.any()
    assert seen_alpha.dtype == F32 and torch.equal(seen_alpha, torch.ones(H, W))
    assert torch.equal(g, torch.as_tensor(_pose_gradient(pkg, position, rotation)[0]).float())


def test_render_posed_refuses_a_pose_of_other_sizes(pkg, monkeypatch):
    rend, calls = _stub_renderer(pkg, monkeypatch)
    with pytest.raises(ValueError, match="position must hold 3 values and rotation 4"):
        rend.differentiable_render_posed(W, H, torch.zeros(4), torch.ones(4))
    assert calls == []


def test_a_render_posed_backward_after_another_frame_raises(pkg, monkeypatch):
    rend, calls = _stub_renderer(pkg, monkeypatch)
    position, rotation = _pose()
    rgb = rend.differentiable_render_posed(W, H, position, rotation)
    other = torch.empty((H, W, 4), dtype=F32)
    rend.render(_uniforms(pkg), other.data_ptr())
    with pytest.raises(RuntimeError) as e:
        rgb.sum().backward()
    assert str(e.value) == ("differentiable_render_posed: the forward rendered frame 1 of this renderer, which has rendered frame 2 since; "
                            "the gradient of another frame is not returned")
    assert "blend_backward" not in _names(calls) and position.grad is None
    rend.differentiable_render_posed(W, H, position, rotation).sum().backward()
    assert _names(calls)[-2:] == ["blend_backward", "camera_backward"] and position.grad is not None and rotation.grad is not None
