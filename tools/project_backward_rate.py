#!/usr/bin/env python3
"""What gs_project_backward (k_project_backward, gs_project_backward.hip) costs next to the blend's backward it follows, on the
frame both describe.  Per scene, at one resolution, from one run:

    k_blend_backward, all four outputs         the pass in front of it: d_colour, d_opacity, d_conic, d_uv from grad_rgb and grad_alpha
    k_project_backward, all six outputs        those four sums in; means, log-scales, quaternions, logits, SH DC and 45 rest coefficients out
    k_project_backward, without the SH outputs the same without d_sh_dc and d_sh_rest (the coefficients are still read: they shape d_means)
    torch projection, float32, fwd + bwd       a dense torch restatement of the record function over ALL N Gaussians (the visible
                                               ones and the culled alike), differentiated by autograd: what INTEGRATION.md 3g
                                               left to the caller before this pass existed (--no-torch leaves it out)

A pass is timed between two events on the stream it runs on (the renderer's, idle before: the call returns synchronised, so the
span is the launches, the kernels and nothing else; the torch projection between two events on torch's current stream).  One warm
call per pass -- the first gs_project_backward after a frame also rebuilds the frame's tiles plane, once -- then --repeats ROUNDS,
each round timing every pass once in turn; median and minimum over the rounds.  The sums keep growing over the rounds: a binary64
add costs the same whatever it adds to.  Every figure of one scene is taken on the same frame.

    python tools/project_backward_rate.py [--gaussians 1000000] [--scenes S T] [--width 1920 --height 1080] [--repeats 15] [--no-torch] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--gaussians", type=int, default=1_000_000)
ap.add_argument("--scenes", nargs="+", default=["S", "T"])
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--repeats", type=int, default=15)
ap.add_argument("--no-torch", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()

import torch  # noqa: E402

pkg = entry.load_package()
w, h, n = args.width, args.height, args.gaussians

SH_C0, SH_C1 = 0.28209479177387814, 0.4886025119029199
SH_C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
SH_C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
         -0.5900435899266435)


def timed(call, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    call()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def torch_projection(p, u):
    """uv, conic, opacity, rgb of every Gaussian from the six parameter tensors, float32 on the device: the record function of
    gs_project_backward (include/gs3d_hip.h) without the culls, antialiasing off, the clamps as torch.clamp."""
    pm = torch.tensor(np.asarray(u["proj_mat"][0], np.float32).reshape(4, 4).T.copy(), device="cuda")
    vm = torch.tensor(np.asarray(u["view_mat"][0], np.float32).reshape(4, 4).T.copy(), device="cuda")
    W, H = float(u["width"][0]), float(u["height"][0])
    tan_x, tan_y = float(u["tan_fovx"][0]), float(u["tan_fovy"][0])
    ph = torch.cat([p["means"], torch.ones_like(p["means"][:, :1])], dim=1)
    hh, t = ph @ pm.T, (ph @ vm.T)[:, :3]
    uv = torch.stack([((hh[:, 0] / hh[:, 3] + 1.0) * W - 1.0) / 2.0, ((hh[:, 1] / hh[:, 3] + 1.0) * H - 1.0) / 2.0], dim=1)
    tz = t[:, 2]
    tx = torch.clamp(t[:, 0] / tz, -1.3 * tan_x, 1.3 * tan_x) * tz
    ty = torch.clamp(t[:, 1] / tz, -1.3 * tan_y, 1.3 * tan_y) * tz
    fx, fy = W / (2.0 * tan_x), H / (2.0 * tan_y)
    zero = torch.zeros_like(tz)
    J = torch.stack([torch.stack([fx / tz, zero, -fx * tx / tz ** 2], dim=1), torch.stack([zero, fy / tz, -fy * ty / tz ** 2], dim=1)], dim=1)
    A = J @ vm[:3, :3]
    q = p["quats"] / p["quats"].norm(dim=1, keepdim=True)
    qw, qx, qy, qz = q.unbind(dim=1)
    R = torch.stack([torch.stack([1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)], dim=1),
                     torch.stack([2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)], dim=1),
                     torch.stack([2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)], dim=1)], dim=1)
    M = A @ R
    cov = (M * torch.exp(2.0 * p["log_scales"])[:, None, :]) @ M.transpose(1, 2)
    m00, m11, m01 = cov[:, 0, 0] + 0.3, cov[:, 1, 1] + 0.3, cov[:, 0, 1]
    det = m00 * m11 - m01 * m01
    conic = torch.stack([m11 / det, -m01 / det, m00 / det], dim=1)
    rel = p["means"] - torch.tensor(np.asarray(u["camera_position"][0][:3], np.float32), device="cuda")
    x, y, z = (rel / rel.norm(dim=1, keepdim=True)).unbind(dim=1)
    c2, c3 = SH_C2, SH_C3
    B = torch.stack([torch.full_like(x, SH_C0), -SH_C1 * y, SH_C1 * z, -SH_C1 * x,
                     c2[0] * x * y, c2[1] * y * z, c2[2] * (2 * z * z - x * x - y * y), c2[3] * z * x, c2[4] * (x * x - y * y),
                     c3[0] * (3 * x * x - y * y) * y, c3[1] * x * y * z, c3[2] * (4 * z * z - x * x - y * y) * y,
                     c3[3] * z * (2 * z * z - 3 * x * x - 3 * y * y), c3[4] * x * (4 * z * z - x * x - y * y),
                     c3[5] * (x * x - y * y) * z, c3[6] * x * (x * x - 3 * y * y)], dim=1)
    rgb = 0.5 + B[:, :1] * p["sh_dc"] + torch.einsum("nj,njk->nk", B[:, 1:], p["sh_rest"])
    rgb = torch.cat([torch.clamp(rgb[:, :1], min=0.0), rgb[:, 1:]], dim=1)
    return uv, conic, torch.sigmoid(p["opacity_logits"]), rgb


lines = [f"# python tools/project_backward_rate.py --gaussians {n} --scenes {' '.join(args.scenes)} --width {w} --height {h} "
         f"--repeats {args.repeats}   ({torch.cuda.get_device_name(0)}; {args.repeats} rounds after one warm call, every pass once per round)",
         "%-6s %-44s %10s %10s %18s" % ("scene", "what", "median_ms", "min_ms", "x k_blend_backward")]
for kind in args.scenes:
    rec = pkg.synth.synth_records(n, seed=0, kind=kind)
    scene = pkg.Scene.from_records(rec, device=0)
    del rec
    rend = pkg.Renderer(scene)
    u = pkg.camera_uniforms(pkg.make_camera(), w, h)
    rend.render_host(u, want_rgba=True)
    st = rend.stats()
    stream = torch.cuda.ExternalStream(rend.stream)
    gen = torch.Generator(device="cuda").manual_seed(1)
    grad_rgb = torch.randn((h, w, 3), dtype=torch.float32, device="cuda", generator=gen)
    grad_alpha = torch.randn((h, w), dtype=torch.float32, device="cuda", generator=gen)
    f64 = dict(dtype=torch.float64, device="cuda")
    d = dict(colour=torch.zeros((n, 3), **f64), opacity=torch.zeros((n,), **f64), conic=torch.zeros((n, 3), **f64), uv=torch.zeros((n, 2), **f64))
    rend.blend_backward(grad_rgb, grad_alpha, **d)            # the inputs of the projection: one blend backward's sums
    g_in = {k: v.clone() for k, v in d.items()}
    geo = dict(means=torch.zeros((n, 3), **f64), log_scales=torch.zeros((n, 3), **f64), quats=torch.zeros((n, 4), **f64),
               opacity_logits=torch.zeros((n,), **f64))
    sh = dict(sh_dc=torch.zeros((n, 3), **f64), sh_rest=torch.zeros((n, 15, 3), **f64))
    passes = [("k_blend_backward, all four outputs", lambda: rend.blend_backward(grad_rgb, grad_alpha, **d), stream),
              ("k_project_backward, all six outputs", lambda: rend.project_backward(**g_in, out={**geo, **sh}), stream),
              ("k_project_backward, without the SH outputs", lambda: rend.project_backward(**g_in, out=dict(geo)), stream)]
    if not args.no_torch:
        params = {k: v.requires_grad_() for k, v in scene.to_tensors().items()}
        g32 = {k: v.float() for k, v in g_in.items()}

        def torch_step():
            for v in params.values():
                v.grad = None
            uv, conic, opacity, rgb = torch_projection(params, u)
            ((g32["uv"] * uv).sum() + (g32["conic"] * conic).sum() + (g32["opacity"] * opacity).sum() + (g32["colour"] * rgb).sum()).backward()
        passes.append(("torch projection, float32, fwd + bwd, all N", torch_step, torch.cuda.current_stream()))
    for _, call, _ in passes:
        call()
    torch.cuda.synchronize()
    ms = {what: [] for what, _, _ in passes}
    for _ in range(args.repeats):
        for what, call, s in passes:
            ms[what].append(timed(call, s))
    blend = statistics.median(ms[passes[0][0]])
    for what, _, _ in passes:
        med = statistics.median(ms[what])
        lines.append("%-6s %-44s %10.3f %10.3f %18.2f" % (kind, what, med, min(ms[what]), med / blend))
    lines.append(f"#      {kind}({n}): V = {st.num_visible} visible Gaussians, D = {st.num_instances} tile instances; "
                 f"{int((g_in['opacity'] != 0).sum())} Gaussians carry a gradient from the blend")
    rend.close()
    scene.close()
    del grad_rgb, grad_alpha, d, g_in, geo, sh, passes
    if not args.no_torch:
        del params, g32
    torch.cuda.empty_cache()
text = "\n".join(lines) + "\n"
print(text, end="")
if args.out:
    with open(args.out, "w") as f:
        f.write(text)
