#!/usr/bin/env python3
"""What gs_camera_backward (k_camera_backward and its finishing wave, gs_camera_backward.hip) costs next to gs_project_backward,
whose per-Gaussian chain it shares, on the frame both describe.  Per scene, at one resolution, from one run:

    k_project_backward, all six outputs          the yardstick: the same four sums in, the six parameter gradients out
    k_project_backward, without the SH outputs   the same without d_sh_dc and d_sh_rest: what the camera pass is expected to stay at or below
    k_camera_backward, all three outputs         the four sums in; d_view_mat, d_proj_mat, d_camera_position out (two launches)
    k_camera_backward, camera_position only      the same launches with two outputs NULL: all 27 sums are formed whatever is asked for
    camera_pose_gradient (host)                  the three results brought to the host and gs_camera_uniforms_backward: wall clock

A device pass is timed between two events on the renderer's stream (idle before: the call returns synchronised), as
tools/project_backward_rate.py times its passes; the host step by time.perf_counter.  One warm call per pass, then --repeats
ROUNDS, each round timing every pass once in turn; median and minimum over the rounds.  Every figure of one scene is taken on
the same frame, with the same blend backward's sums as the inputs.

    python tools/camera_backward_rate.py [--gaussians 1000000] [--scenes S T] [--width 1920 --height 1080] [--repeats 15] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--gaussians", type=int, default=1_000_000)
ap.add_argument("--scenes", nargs="+", default=["S", "T"])
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--repeats", type=int, default=15)
ap.add_argument("--out", default=None)
args = ap.parse_args()

import torch  # noqa: E402

pkg = entry.load_package()
w, h, n = args.width, args.height, args.gaussians


def timed(call, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    call()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def wall(call, _):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


lines = [f"# python tools/camera_backward_rate.py --gaussians {n} --scenes {' '.join(args.scenes)} --width {w} --height {h} "
         f"--repeats {args.repeats}   ({torch.cuda.get_device_name(0)}; {args.repeats} rounds after one warm call, every pass once per round)",
         "%-6s %-44s %10s %10s %34s" % ("scene", "what", "median_ms", "min_ms", "x k_project_backward without SH")]
for kind in args.scenes:
    rec = pkg.synth.synth_records(n, seed=0, kind=kind)
    scene = pkg.Scene.from_records(rec, device=0)
    del rec
    rend = pkg.Renderer(scene)
    cam = pkg.make_camera()
    u = pkg.camera_uniforms(cam, w, h)
    rend.render_host(u, want_rgba=True)
    st = rend.stats()
    stream = torch.cuda.ExternalStream(rend.stream)
    gen = torch.Generator(device="cuda").manual_seed(1)
    grad_rgb = torch.randn((h, w, 3), dtype=torch.float32, device="cuda", generator=gen)
    grad_alpha = torch.randn((h, w), dtype=torch.float32, device="cuda", generator=gen)
    g_in = rend.blend_backward(grad_rgb, grad_alpha, colour=True, opacity=True, conic=True, uv=True)
    f64 = dict(dtype=torch.float64, device="cuda")
    geo = dict(means=torch.zeros((n, 3), **f64), log_scales=torch.zeros((n, 3), **f64), quats=torch.zeros((n, 4), **f64),
               opacity_logits=torch.zeros((n,), **f64))
    sh = dict(sh_dc=torch.zeros((n, 3), **f64), sh_rest=torch.zeros((n, 15, 3), **f64))
    outs = dict(view_mat=torch.zeros(16, **f64), proj_mat=torch.zeros(16, **f64), camera_position=torch.zeros(3, **f64))
    passes = [("k_project_backward, all six outputs", lambda: rend.project_backward(**g_in, out={**geo, **sh}), timed),
              ("k_project_backward, without the SH outputs", lambda: rend.project_backward(**g_in, out=dict(geo)), timed),
              ("k_camera_backward, all three outputs", lambda: rend.camera_backward(**g_in, **outs), timed),
              ("k_camera_backward, camera_position only",
               lambda: rend.camera_backward(**g_in, view_mat=None, proj_mat=None, camera_position=outs["camera_position"]), timed),
              ("camera_pose_gradient (host)", lambda: pkg.camera_pose_gradient(cam, w, h, outs), wall)]
    for _, call, _ in passes:
        call()
    torch.cuda.synchronize()
    ms = {what: [] for what, _, _ in passes}
    for _ in range(args.repeats):
        for what, call, clock in passes:
            ms[what].append(clock(call, stream))
    yard = statistics.median(ms[passes[1][0]])
    for what, _, _ in passes:
        med = statistics.median(ms[what])
        lines.append("%-6s %-44s %10.3f %10.3f %34.2f" % (kind, what, med, min(ms[what]), med / yard))
    lines.append(f"#      {kind}({n}): V = {st.num_visible} visible Gaussians, D = {st.num_instances} tile instances; "
                 f"{int((g_in['opacity'] != 0).sum())} Gaussians carry a gradient from the blend")
    rend.close()
    scene.close()
    del grad_rgb, grad_alpha, g_in, geo, sh, outs, passes
    torch.cuda.empty_cache()
text = "\n".join(lines) + "\n"
print(text, end="")
if args.out:
    with open(args.out, "w") as f:
        f.write(text)
