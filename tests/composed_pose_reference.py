"""The whole backward with the camera's POSE as the leaves: pose -> uniforms -> record -> image.  Two statements, as
tests/composed_reference.py has them for the scene's parameters:

  chained()             tests/camera_backward_reference.py fed with the sums of tests/backward_reference.py (the definition's
                        binary32 walk: what the device is compared with), carried to the pose by torch.autograd of
                        camera_record_torch.pose_uniforms alone -- the yardsticks chained as differentiable_render_posed chains
                        the kernels;
  composed_autograd()   ONE float64 torch function from position and rotation to rgb and alpha -- pose_uniforms feeding the record
                        function of tests/camera_record_torch.py feeding the dense blend of tests/test_blend_backward_api.py --
                        differentiated by torch.autograd.  Every decision of the frame is a constant; uniforms and record enter as
                        value32.detach() + (F - F.detach()), so the gradient is evaluated at the frame's binary32 values.

reference_descent() is the pose-refinement loop of tests/test_gpu_camera_backward.py on the CPU: the oracle's frame, chained()'s
gradient, torch's Adam on a float64 pose."""
import numpy as np

import backward_cameras as bc
import backward_reference as bref
import camera_backward_reference as cref
import camera_record_torch as crt
import project_backward_reference as pref
from composed_reference import INS, RENDER_SCENE

POSE_LR, POSE_STEPS = 5e-4, 16
POSE_TWIST = dict(position=(0.015, -0.01, 0.0125), rotation=(0.0, 0.006, -0.005, 0.004))   # added to C1's position and quaternion
# What reference_descent gives (asserted by tests/test_camera_backward_api.py): the loss falls at each of its first 10 steps
# (37.7 -> 1.94) and the pose error after 16 steps is 0.801 of the start's (0.0307 -> 0.0246; the loss is steep across the
# valley in which a small translation and a small rotation of the camera compensate, and flat along it).  The device loop
# (tests/test_gpu_camera_backward.py) runs float32 parameters: it is held to the first POSE_MONOTONE = 8 steps falling and to
# POSE_DEVICE_FACTOR -- the reference's factor plus 0.02, two hundred times what sixteen roundings of the pose to 2^-24 move it.
POSE_REFERENCE_MONOTONE, POSE_REFERENCE_FACTOR = 10, 0.801
POSE_MONOTONE, POSE_DEVICE_FACTOR = 8, 0.82


def pose_chain(cam, w, h, d):
    """(d_position, d_rotation): torch.autograd of pose_uniforms at the camera's binary32 values, contracted with
    d = dict(view_mat [16], proj_mat [16], camera_position [3])."""
    import torch
    c = cam[0] if getattr(cam, "shape", ()) else cam
    p = torch.tensor(np.asarray(c["position"], np.float64), requires_grad=True)
    q = torch.tensor(np.asarray(c["rotation"], np.float64), requires_grad=True)
    view, proj, pos = crt.pose_uniforms(p, q, float(c["fov"]), float(c["near_plane"]), float(c["far_plane"]), w, h)
    T = lambda a: torch.tensor(np.asarray(a, np.float64))  # noqa: E731
    ((T(d["view_mat"]).reshape(4, 4).T * view).sum() + (T(d["proj_mat"]).reshape(4, 4).T * proj).sum() + (T(d["camera_position"]) * pos).sum()).backward()
    return p.grad.numpy().copy(), q.grad.numpy().copy()


def pose_jacobian_abs(cam, w, h):
    """|d uniform / d pose|: (view [16][7], proj [16][7]) absolute Jacobians (uniforms' layout, pose = position then rotation), by
    autograd of pose_uniforms -- what carries a bound on the uniforms' gradients to a bound on the pose's."""
    import torch
    c = cam[0] if getattr(cam, "shape", ()) else cam
    x = torch.tensor(np.concatenate([np.asarray(c["position"], np.float64), np.asarray(c["rotation"], np.float64)]))

    def f(x):
        view, proj, _ = crt.pose_uniforms(x[:3], x[3:], float(c["fov"]), float(c["near_plane"]), float(c["far_plane"]), w, h)
        return torch.cat([view.T.reshape(16), proj.T.reshape(16)])
    J = torch.autograd.functional.jacobian(f, x).numpy()
    return np.abs(J[:16]), np.abs(J[16:])


def chained(oracle, verts, cam, u, ref, G, ga, antialiased=False):
    """(d_position, d_rotation, margin [7], want): the chained references' pose gradient of sum(G rgb) + sum(ga alpha), and the
    bound on how far another evaluation within the references' bounds may lie from it: the camera reference's bound plus its
    magnitudes of the blend's own bounds, carried to the pose by the absolute Jacobian of the uniforms."""
    w, h = int(u["width"][0]), int(u["height"][0])
    blend = bref.backward(oracle, ref, w, h, G, ga)
    fields = pref.unpack_vertices(verts)
    vis, red = ref["tiles"] != 0, ref["attr"]["color_radii"][:, 0] > 0
    args = lambda g: dict(colour=g["colour"], opacity_grad=g["opacity"], conic=g["conic"], uv=g["uv"], antialiased=antialiased)  # noqa: E731
    want = cref.backward(*fields, u, vis, red, **args({k: blend[k] for k in INS}))
    spread = cref.backward(*fields, u, vis, red, **args({k: bref.bound(blend, k) for k in INS}))["A"]
    dp, dq = pose_chain(cam, w, h, want)
    Jv, Jp = pose_jacobian_abs(cam, w, h)
    lim = {k: cref.bound(want, k) + spread[k] for k in cref.OUTPUTS}
    margin = lim["view_mat"] @ Jv + lim["proj_mat"] @ Jp
    margin[:3] += lim["camera_position"]
    return dp, dq, margin, want


def composed_autograd(oracle, verts, cam, u, ref, G, ga, antialiased=False):
    """torch.autograd's (d_position, d_rotation) of the one float64 function from the pose to sum(G rgb) + sum(ga alpha)."""
    import torch
    from test_blend_backward_api import _dense_loss
    w, h = int(u["width"][0]), int(u["height"][0])
    c = cam[0] if getattr(cam, "shape", ()) else cam
    attr = ref["attr"]
    pairs = bref.backward(oracle, ref, w, h, G, ga)["pairs"]
    p = torch.tensor(np.asarray(c["position"], np.float64), requires_grad=True)
    q = torch.tensor(np.asarray(c["rotation"], np.float64), requires_grad=True)
    view64, proj64, pos64 = crt.pose_uniforms(p, q, float(c["fov"]), float(c["near_plane"]), float(c["far_plane"]), w, h)
    u0 = u[0]
    T = lambda a: torch.tensor(np.asarray(a, np.float64))  # noqa: E731
    at32 = lambda v32, F: v32 + (F - F.detach())  # noqa: E731
    view = at32(T(u0["view_mat"]).reshape(4, 4).T, view64)
    proj = at32(T(u0["proj_mat"]).reshape(4, 4).T, proj64)
    pos = at32(T(np.asarray(u0["camera_position"]).reshape(-1)[:3]), pos64)
    f = crt.forward(verts, u, ref["tiles"] != 0, attr["color_radii"][:, 0] > 0, antialiased, False, view, proj, pos)
    idx = torch.as_tensor(f["idx"].astype(np.int64))

    def at_frame(rec32, F):
        base = T(rec32)
        return base.index_add(0, idx, (F - F.detach()).reshape((len(idx),) + tuple(base.shape[1:])))
    ga = np.zeros((h, w), np.float32) if ga is None else ga
    _dense_loss(at_frame(attr["conic_opacity"][:, :3], f["conic"]), at_frame(attr["conic_opacity"][:, 3], f["opacity"]),
                at_frame(attr["uv"][:, :2], f["uv"]), at_frame(attr["color_radii"][:, :3], f["rgb"]), ref, w, h, pairs, G, ga).backward()
    return p.grad.numpy().copy(), q.grad.numpy().copy()


def descent_start(pkg):
    """(C1's pose, the displaced pose the descent starts from) as float64 (position [3], rotation [4])."""
    c1 = bc.camera(pkg, "C1")[0]
    p0, q0 = np.asarray(c1["position"], np.float64), np.asarray(c1["rotation"], np.float64)
    return (p0, q0), (p0 + np.asarray(POSE_TWIST["position"]), q0 + np.asarray(POSE_TWIST["rotation"]))


def pose_error(pose, target):
    """|position - target| + |rotation / |rotation| - target rotation| (the sign fixed: a small twist)."""
    q = pose[1] / np.linalg.norm(pose[1])
    return float(np.linalg.norm(pose[0] - target[0]) + np.linalg.norm(q - target[1] / np.linalg.norm(target[1])))


def reference_descent(pkg, oracle, lr=POSE_LR, steps=POSE_STEPS):
    """(losses before each Adam step and after the last, pose errors likewise) on the CPU: RENDER_SCENE held, the target rendered
    at C1 by the oracle, the pose started POSE_TWIST away; the oracle's frame at the pose rounded to binary32, chained()'s
    gradient with grad_rgb = 2 (rgb - target), torch's Adam on the float64 pose."""
    import torch
    n, w, h = RENDER_SCENE
    verts = oracle.activate_records(pkg.synth.synth_records(n, seed=9, kind="A"))
    target_pose, start = descent_start(pkg)
    fov = bc.CAMERAS["C1"]["fov"]
    target = oracle.stages(verts, oracle.camera_uniforms(bc.camera(oracle, "C1"), w, h))["image"][..., :3].astype(np.float32)
    p, q = torch.tensor(start[0], requires_grad=True), torch.tensor(start[1], requires_grad=True)
    opt = torch.optim.Adam([p, q], lr=lr)
    losses, errors = [], []
    for step in range(steps + 1):
        cam = oracle.default_camera(position=p.detach().numpy(), rotation=q.detach().numpy(), fov=fov)
        u = oracle.camera_uniforms(cam, w, h)
        ref = oracle.stages(verts, u)
        diff = ref["image"][..., :3].astype(np.float32) - target
        losses.append(float((diff ** 2).sum()))
        errors.append(pose_error((p.detach().numpy(), q.detach().numpy()), target_pose))
        if step == steps:
            break
        dp, dq, _, _ = chained(oracle, verts, cam, u, ref, (2.0 * diff).astype(np.float32), None)
        opt.zero_grad()
        p.grad, q.grad = torch.tensor(dp), torch.tensor(dq)
        opt.step()
    return losses, errors
