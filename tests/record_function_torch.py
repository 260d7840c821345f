"""The record function F of gs_project_backward (include/gs3d_hip.h) restated as a FORWARD function in torch float64 over the
visible Gaussians, the frame's branches as constants: written independently of tests/project_backward_reference.py's chain rule,
so that torch.autograd's gradients of it pin that module (tests/test_project_backward_api.py), and composed with the dense blend
of tests/test_blend_backward_api.py into one function from parameters to image (tests/test_backward_cameras_api.py).

The parameters enter so that the stored values are reproduced exactly: s = s_stored exp(0), o = o e^0 / ((1 - o) + o e^0),
q^ = q / |q|.  A plain module: torch is imported by the function."""
import numpy as np

import project_backward_reference as pref

LEAVES = ("means", "log_scales", "quats", "opacity_logits", "sh")


def forward(verts, u, visible, red_flows, antialiased, sh16):
    """Returns dict(idx = the visible ids; leaves = {means [nv][3], log_scales [nv][3] (zeros: the offset from the stored log
    scale), quats [nv][4], opacity_logits [nv] (zeros: the offset from the stored logit), sh [nv][16][3]}, each requiring a
    gradient; uv [nv][2], conic [nv][3], opacity [nv] (after the antialiased factor), rgb [nv][3] (red's clamp applied as the frame
    took it)): torch float64 tensors in one graph."""
    import torch
    pos, scale, quat, opac, sh = pref.unpack_vertices(verts, sh16=sh16)
    idx = np.nonzero(visible)[0]
    u0 = u[0] if getattr(u, "shape", ()) else u
    T = lambda a: torch.tensor(np.asarray(a, np.float64))  # noqa: E731
    _, ratio, clamped, _ = pref.clamp_branches(pos, u0)
    binds, cconst = torch.as_tensor(clamped[idx] != ratio[idx]), T(clamped[idx])
    p = T(pos[idx]).requires_grad_()
    dls = torch.zeros((len(idx), 3), dtype=torch.float64, requires_grad=True)
    dlogit = torch.zeros(len(idx), dtype=torch.float64, requires_grad=True)
    q = T(quat[idx]).requires_grad_()
    shl = T(sh[idx]).requires_grad_()
    s = T(scale[idx]) * torch.exp(dls)
    o0 = T(opac[idx])
    e = torch.exp(dlogit)
    o = o0 * e / ((1.0 - o0) + o0 * e)
    pm, vm = T(u0["proj_mat"]).reshape(4, 4).T, T(u0["view_mat"]).reshape(4, 4).T     # [row][column]
    W, H = float(u0["width"]), float(u0["height"])
    tan_x, tan_y = float(np.float32(u0["tan_fovx"])), float(np.float32(u0["tan_fovy"]))
    ph = torch.cat([p, torch.ones((len(idx), 1), dtype=torch.float64)], dim=1)
    hh, t = ph @ pm.T, (ph @ vm.T)[:, :3]
    uv = torch.stack([((hh[:, 0] / hh[:, 3] + 1.0) * W - 1.0) / 2.0, ((hh[:, 1] / hh[:, 3] + 1.0) * H - 1.0) / 2.0], dim=1)
    txy = torch.where(binds, cconst * t[:, 2:3], t[:, :2])
    fx, fy = W / (2.0 * tan_x), H / (2.0 * tan_y)
    zero = torch.zeros(len(idx), dtype=torch.float64)
    J = torch.stack([torch.stack([fx / t[:, 2], zero, -fx * txy[:, 0] / t[:, 2] ** 2], dim=1),
                     torch.stack([zero, fy / t[:, 2], -fy * txy[:, 1] / t[:, 2] ** 2], dim=1)], dim=1)
    A = J @ vm[:3, :3]
    qh = q / q.norm(dim=1, keepdim=True)
    w_, x_, y_, z_ = qh.unbind(dim=1)
    R = torch.stack([torch.stack([1 - 2 * (y_ * y_ + z_ * z_), 2 * (x_ * y_ - z_ * w_), 2 * (x_ * z_ + y_ * w_)], dim=1),
                     torch.stack([2 * (x_ * y_ + z_ * w_), 1 - 2 * (x_ * x_ + z_ * z_), 2 * (y_ * z_ - x_ * w_)], dim=1),
                     torch.stack([2 * (x_ * z_ - y_ * w_), 2 * (y_ * z_ + x_ * w_), 1 - 2 * (x_ * x_ + y_ * y_)], dim=1)], dim=1)
    Sigma = R @ torch.diag_embed(s * s) @ R.transpose(1, 2)
    cov = A @ Sigma @ A.transpose(1, 2)
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
    rel = p - T(u0["camera_position"])[:3]
    d = rel / rel.norm(dim=1, keepdim=True)
    x, y, z = d.unbind(dim=1)
    c0, c1, c2, c3 = pref.SH_C0, pref.SH_C1, pref.SH_C2, pref.SH_C3
    B = torch.stack([torch.full_like(x, c0), -c1 * y, c1 * z, -c1 * x,
                     c2[0] * x * y, c2[1] * y * z, c2[2] * (2 * z * z - x * x - y * y), c2[3] * z * x, c2[4] * (x * x - y * y),
                     c3[0] * (3 * x * x - y * y) * y, c3[1] * x * y * z, c3[2] * (4 * z * z - x * x - y * y) * y,
                     c3[3] * z * (2 * z * z - 3 * x * x - 3 * y * y), c3[4] * x * (4 * z * z - x * x - y * y),
                     c3[5] * (x * x - y * y) * z, c3[6] * x * (x * x - 3 * y * y)], dim=1)
    rgb = 0.5 + torch.einsum("nj,njk->nk", B, shl)
    flows = torch.ones((len(idx), 3), dtype=torch.bool)
    flows[:, 0] = torch.as_tensor(np.asarray(red_flows, bool)[idx])
    rgb = torch.where(flows, rgb, torch.zeros_like(rgb))
    return dict(idx=idx, leaves=dict(means=p, log_scales=dls, quats=q, opacity_logits=dlogit, sh=shl),
                uv=uv, conic=conic, opacity=op, rgb=rgb)


def gradients(f, n, k):
    """The leaves' gradients after a backward through `f` (forward's return), scattered to the six outputs' shapes over n
    Gaussians (culled rows 0), sh_rest of k coefficients."""
    idx, leaves = f["idx"], f["leaves"]

    def full(t, shape):
        out = np.zeros((n,) + shape)
        out[idx] = t.numpy().reshape((len(idx),) + shape)
        return out
    sh = leaves["sh"].grad
    return dict(means=full(leaves["means"].grad, (3,)), log_scales=full(leaves["log_scales"].grad, (3,)),
                quats=full(leaves["quats"].grad, (4,)), opacity_logits=full(leaves["opacity_logits"].grad, ()),
                sh_dc=full(sh[:, 0], (3,)), sh_rest=full(sh[:, 1:1 + k].contiguous(), (k, 3)))
