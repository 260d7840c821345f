#!/usr/bin/env python3
"""What gs_blend_backward (k_blend_backward, gs_backward.hip) costs next to its two sibling passes on the frame all three describe.
Per scene, at one resolution, from one run:

    exact blend, ms_render                  the yardstick: gs_get_stats' ms_render of the same frame in exp mode 2
    k_blend_backward, all four outputs      grad_rgb and grad_alpha in, d_colour, d_opacity, d_conic, d_uv out: two walks, nine sums
    k_blend_backward, geometry only         without d_colour: two walks, six sums
    k_blend_backward, d_colour alone        one walk, three sums (the instantiation without the first walk)
    k_features, 3 channels, out only        gs_blend_features: the forward for three channels
    k_lift, 4 channels, out + weight        gs_lift_pixels: one walk, the transpose-reduce of four channels and the weight

A pass is timed between two events on the stream it runs on (the renderer's, idle before: the call returns synchronised, so the
span is the launches, the kernels and nothing else).  One warm call per pass, then --repeats ROUNDS, each round timing every pass
once in turn, so that a drift of the clock or a neighbour on the machine falls on all of them alike; median and minimum over the
rounds.  The sums keep growing over the rounds: a binary64 add costs the same whatever it adds to.  Every figure of one scene is
taken on the same frame.

    python tools/blend_backward_rate.py [--gaussians 1000000] [--scenes S T] [--width 1920 --height 1080] [--repeats 15] [--out FILE]
"""
import argparse
import os
import statistics
import sys

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


def blend_ms(rend, u, mode):
    rend.set_exp_mode(mode)
    ms = []
    for _ in range(args.repeats + 1):
        rend.render_host(u, want_rgba=True)
        ms.append(rend.stats().ms_render)
    return statistics.median(ms[1:])


def timed(call, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    call()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


lines = [f"# python tools/blend_backward_rate.py --gaussians {n} --scenes {' '.join(args.scenes)} --width {w} --height {h} "
         f"--repeats {args.repeats}   ({torch.cuda.get_device_name(0)}; {args.repeats} rounds after one warm call, every pass once per round)",
         "%-6s %-40s %6s %10s %10s %13s" % ("scene", "what", "walks", "median_ms", "min_ms", "x exact blend")]
for kind in args.scenes:
    rec = pkg.synth.synth_records(n, seed=0, kind=kind)
    scene = pkg.Scene.from_records(rec, device=0)
    del rec
    rend = pkg.Renderer(scene)
    u = pkg.camera_uniforms(pkg.make_camera(), w, h)
    exact = blend_ms(rend, u, 2)
    st = rend.stats()
    stream = torch.cuda.ExternalStream(rend.stream)
    gen = torch.Generator(device="cuda").manual_seed(1)
    grad_rgb = torch.randn((h, w, 3), dtype=torch.float32, device="cuda", generator=gen)
    grad_alpha = torch.randn((h, w), dtype=torch.float32, device="cuda", generator=gen)
    values4 = torch.randn((h, w, 4), dtype=torch.float32, device="cuda", generator=gen)
    feats = torch.randn((n, 3), dtype=torch.float32, device="cuda", generator=gen)
    f64 = dict(dtype=torch.float64, device="cuda")
    d = dict(colour=torch.zeros((n, 3), **f64), opacity=torch.zeros((n,), **f64), conic=torch.zeros((n, 3), **f64), uv=torch.zeros((n, 2), **f64))
    lifted, weight = torch.zeros((n, 4), **f64), torch.zeros((n,), **f64)
    fmap = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    passes = [("k_blend_backward, all four outputs", 2, lambda: rend.blend_backward(grad_rgb, grad_alpha, **d)),
              ("k_blend_backward, geometry only", 2, lambda: rend.blend_backward(grad_rgb, grad_alpha, opacity=d["opacity"], conic=d["conic"], uv=d["uv"])),
              ("k_blend_backward, d_colour alone", 1, lambda: rend.blend_backward(grad_rgb, colour=d["colour"])),
              ("k_features, 3 channels, out only", 1, lambda: rend.feature_maps(features=feats, out=fmap)),
              ("k_lift, 4 channels, out + weight", 1, lambda: rend.lift_pixels(values4, out=lifted, weight=weight))]
    for _, _, call in passes:
        call()
    ms = {what: [] for what, _, _ in passes}
    for _ in range(args.repeats):
        for what, _, call in passes:
            ms[what].append(timed(call, stream))
    lines.append("%-6s %-40s %6s %10.3f %10s %13.2f" % (kind, "exact blend (exp mode 2), ms_render", "1", exact, "", 1.0))
    for what, walks, _ in passes:
        med = statistics.median(ms[what])
        lines.append("%-6s %-40s %6d %10.3f %10.3f %13.2f" % (kind, what, walks, med, min(ms[what]), med / exact))
    full = statistics.median(ms[passes[0][0]])
    lines.append(f"#      {kind}({n}): V = {st.num_visible}, D = {st.num_instances} tile instances; {int((weight > 0).sum())} Gaussians were "
                 f"blended at some pixel; all four outputs = {full / statistics.median(ms[passes[3][0]]):.2f} x k_features of 3 channels, "
                 f"{full / statistics.median(ms[passes[4][0]]):.2f} x k_lift of 4 channels")
    rend.close()
    scene.close()
    del grad_rgb, grad_alpha, values4, feats, d, lifted, weight, fmap
    torch.cuda.empty_cache()
text = "\n".join(lines) + "\n"
print(text, end="")
if args.out:
    with open(args.out, "w") as f:
        f.write(text)
