"""The record function F of gs_camera_backward (include/gs3d_hip.h) as a FORWARD function in torch float64 over the visible
Gaussians with the frame's uniforms -- view_mat, proj_mat, camera_position -- as the leaves and the Gaussians' stored values as
constants: written independently of tests/camera_backward_reference.py's chain rule, so that torch.autograd's gradients of it pin
that module (tests/test_camera_backward_api.py).  The frame's branches are constants taken as the frame took them: visibility and
red's flow come in from the oracle, the clamps' branches from project_backward_reference.clamp_branches (the binary32
restatement of k_preprocess); that module is used for nothing else but unpacking the vertices and its binary32 constants.

pose_uniforms() is the exact real function behind gs_camera_uniforms in torch float64 with the camera's position and raw
quaternion as leaves: with it in front, the same forward is a function of the pose.  A plain module: torch is imported by the
functions."""
import numpy as np

import project_backward_reference as pref


def pose_uniforms(position, rotation, fov, near, far, width, height):
    """(view [4][4], proj [4][4] as [row][column] -- the uniforms' matrices, flips included -- and camera_position [3]) in torch
    float64 from position [3] and rotation [4] (w x y z, NOT normalised, as the forward takes it): M = T(position)
    mat4_cast(rotation), view = M^-1, proj = persp view, the y and z rows of view and the y row of proj negated."""
    import torch
    w, x, y, z = rotation.unbind()
    one = torch.ones((), dtype=torch.float64)
    R = torch.stack([torch.stack([one - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)]),
                     torch.stack([2 * (x * y + w * z), one - 2 * (x * x + z * z), 2 * (y * z - w * x)]),
                     torch.stack([2 * (x * z - w * y), 2 * (y * z + w * x), one - 2 * (x * x + y * y)])])
    M = torch.cat([torch.cat([R, position.reshape(3, 1)], dim=1), torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=torch.float64)], dim=0)
    view = torch.linalg.inv(M)
    tan_x = np.tan(np.float64(np.float32(fov)) * 0.01745329251994329576923690768489 / 2.0)
    tan_y = tan_x * height / width
    n_, f_ = float(np.float32(near)), float(np.float32(far))
    persp = torch.tensor([[1.0 / tan_x, 0, 0, 0], [0, 1.0 / tan_y, 0, 0], [0, 0, -(f_ + n_) / (f_ - n_), -(2.0 * f_ * n_) / (f_ - n_)],
                          [0, 0, -1.0, 0]], dtype=torch.float64)
    proj = persp @ view
    flip_v = torch.tensor([1.0, -1.0, -1.0, 1.0], dtype=torch.float64).reshape(4, 1)
    flip_p = torch.tensor([1.0, -1.0, 1.0, 1.0], dtype=torch.float64).reshape(4, 1)
    return view * flip_v, proj * flip_p, position


def leaves_of(u):
    """The three leaves at a uniforms record's binary32 values: view [4][4], proj [4][4] ([row][column]), camera_position [3]."""
    import torch
    u0 = u[0] if getattr(u, "shape", ()) else u
    T = lambda a: torch.tensor(np.asarray(a, np.float64))  # noqa: E731
    view = T(u0["view_mat"]).reshape(4, 4).T.contiguous().requires_grad_()
    proj = T(u0["proj_mat"]).reshape(4, 4).T.contiguous().requires_grad_()
    cam = T(np.asarray(u0["camera_position"]).reshape(-1)[:3]).requires_grad_()
    return view, proj, cam


def forward(verts, u, visible, red_flows, antialiased, sh16, view, proj, cam):
    """dict(idx; uv [nv][2], conic [nv][3], opacity [nv] (after the antialiased factor), rgb [nv][3] (red's clamp as the frame took
    it)) as functions of view, proj ([row][column] float64 tensors) and cam [3].  width, height, the tangents and the clamp's
    limits are constants of `u`; so is every branch."""
    import torch
    pos, scale, quat, opac, sh = pref.unpack_vertices(verts, sh16=sh16)
    idx = np.nonzero(visible)[0]
    u0 = u[0] if getattr(u, "shape", ()) else u
    T = lambda a: torch.tensor(np.asarray(a, np.float64))  # noqa: E731
    _, ratio, clamped, _ = pref.clamp_branches(pos, u0)
    binds, cconst = torch.as_tensor(clamped[idx] != ratio[idx]), T(clamped[idx])
    nv = len(idx)
    p, s, q, o, shc = T(pos[idx]), T(scale[idx]), T(quat[idx]), T(opac[idx]), T(sh[idx])
    W, H = float(u0["width"]), float(u0["height"])
    tan_x, tan_y = float(np.float32(u0["tan_fovx"])), float(np.float32(u0["tan_fovy"]))
    ph = torch.cat([p, torch.ones((nv, 1), dtype=torch.float64)], dim=1)
    hh = ph @ proj.T
    t = (ph @ view.T)[:, :3]
    uv = torch.stack([((hh[:, 0] / hh[:, 3] + 1.0) * W - 1.0) / 2.0, ((hh[:, 1] / hh[:, 3] + 1.0) * H - 1.0) / 2.0], dim=1)
    txy = torch.where(binds, cconst * t[:, 2:3], t[:, :2])
    fx, fy = W / (2.0 * tan_x), H / (2.0 * tan_y)
    zero = torch.zeros(nv, dtype=torch.float64)
    J = torch.stack([torch.stack([fx / t[:, 2], zero, -fx * txy[:, 0] / t[:, 2] ** 2], dim=1),
                     torch.stack([zero, fy / t[:, 2], -fy * txy[:, 1] / t[:, 2] ** 2], dim=1)], dim=1)
    A = J @ view[:3, :3]
    qh = q / q.norm(dim=1, keepdim=True)
    w_, x_, y_, z_ = qh.unbind(dim=1)
    R = torch.stack([torch.stack([1 - 2 * (y_ * y_ + z_ * z_), 2 * (x_ * y_ - z_ * w_), 2 * (x_ * z_ + y_ * w_)], dim=1),
                     torch.stack([2 * (x_ * y_ + z_ * w_), 1 - 2 * (x_ * x_ + z_ * z_), 2 * (y_ * z_ - x_ * w_)], dim=1),
                     torch.stack([2 * (x_ * z_ - y_ * w_), 2 * (y_ * z_ + x_ * w_), 1 - 2 * (x_ * x_ + y_ * y_)], dim=1)], dim=1)
    cov = A @ (R @ torch.diag_embed(s * s) @ R.transpose(1, 2)) @ A.transpose(1, 2)
    dil = float(np.float32(0.3))
    m00, m11, m01 = cov[:, 0, 0] + dil, cov[:, 1, 1] + dil, cov[:, 0, 1]
    det = m00 * m11 - m01 * m01
    conic = torch.stack([m11 / det, -m01 / det, m00 / det], dim=1)
    op = o
    if antialiased:
        det_raw = cov[:, 0, 0] * cov[:, 1, 1] - cov[:, 0, 1] * cov[:, 0, 1]
        positive = det_raw.detach() > 0
        comp = torch.sqrt(torch.where(positive, det_raw, torch.ones_like(det_raw)) / det)
        op = torch.where(positive, o * comp, torch.zeros_like(o))
    rel = p - cam
    d = rel / rel.norm(dim=1, keepdim=True)
    x, y, z = d.unbind(dim=1)
    c0, c1, c2, c3 = pref.SH_C0, pref.SH_C1, pref.SH_C2, pref.SH_C3
    B = torch.stack([torch.full_like(x, c0), -c1 * y, c1 * z, -c1 * x,
                     c2[0] * x * y, c2[1] * y * z, c2[2] * (2 * z * z - x * x - y * y), c2[3] * z * x, c2[4] * (x * x - y * y),
                     c3[0] * (3 * x * x - y * y) * y, c3[1] * x * y * z, c3[2] * (4 * z * z - x * x - y * y) * y,
                     c3[3] * z * (2 * z * z - 3 * x * x - 3 * y * y), c3[4] * x * (4 * z * z - x * x - y * y),
                     c3[5] * (x * x - y * y) * z, c3[6] * x * (x * x - 3 * y * y)], dim=1)
    rgb = 0.5 + torch.einsum("nj,njk->nk", B, shc)
    flows = torch.ones((nv, 3), dtype=torch.bool)
    flows[:, 0] = torch.as_tensor(np.asarray(red_flows, bool)[idx])
    rgb = torch.where(flows, rgb, torch.zeros_like(rgb))
    return dict(idx=idx, uv=uv, conic=conic, opacity=op, rgb=rgb)


def loss(f, g):
    """sum_x g_x x over the nine record values of the visible Gaussians: g = dict(colour, opacity, conic, uv) of [n][..] arrays."""
    import torch
    idx = f["idx"]
    T = lambda a: torch.tensor(np.asarray(a, np.float64))  # noqa: E731
    return ((T(g["conic"][idx]) * f["conic"]).sum() + (T(g["opacity"][idx]) * f["opacity"]).sum() + (T(g["uv"][idx]) * f["uv"]).sum()
            + (T(g["colour"][idx]) * f["rgb"]).sum())


def gradients(view, proj, cam):
    """The three leaves' gradients laid out as gs_camera_grads: view_mat [16], proj_mat [16] (element 4 c + r), camera_position [3]."""
    z = lambda t: np.zeros(tuple(t.shape)) if t.grad is None else t.grad.numpy()  # noqa: E731
    return dict(view_mat=np.ascontiguousarray(z(view).T).reshape(16), proj_mat=np.ascontiguousarray(z(proj).T).reshape(16),
                camera_position=z(cam).reshape(3).copy())
