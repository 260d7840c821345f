#!/usr/bin/env python3
"""What gs_lift_pixels (k_lift, gs_lift.hip) costs next to its forward, gs_blend_features, on the frame both describe.  Per
scene, at one resolution, from one run:

    exact blend, ms_render              the yardstick: gs_get_stats' ms_render of the same frame in exp mode 2
    k_lift, C channels, out + weight    C in --channels (0: the weights alone, the channel-less instantiation; G = 16 is one
                                        full group, one launch; 64 is four launches, each walking the lists again)
    k_lift, 3 channels, half masked     the same under a mask that counts the left half of the image
    k_features, C channels, out only    the forward for the same channels, beside it

A pass is timed between two events on the stream it runs on (the renderer's, idle before: the call returns synchronised, so the
span is the launches, the kernels and nothing else); median of --repeats after one warm call per shape.  The sums keep growing
over the repeats: a binary64 add costs the same whatever it adds to.  Every figure of one scene is taken on the same frame.

    python tools/pixel_lift_rate.py [--gaussians 1000000] [--scenes S T] [--width 1920 --height 1080] [--channels 0 1 3 16 64]
                                    [--repeats 15] [--out FILE]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

G = 16  # gs_kernels.h: kLiftGroup, kFeatureGroup

ap = argparse.ArgumentParser()
ap.add_argument("--gaussians", type=int, default=1_000_000)
ap.add_argument("--scenes", nargs="+", default=["S", "T"])
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--channels", type=int, nargs="+", default=[0, 1, 3, G, 64])
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


def pass_ms(call, stream):
    call()
    ms = []
    for _ in range(args.repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        call()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


lines = [f"# python tools/pixel_lift_rate.py --gaussians {n} --scenes {' '.join(args.scenes)} --width {w} --height {h} "
         f"--channels {' '.join(str(c) for c in args.channels)} --repeats {args.repeats}"
         f"   ({torch.cuda.get_device_name(0)}; median of {args.repeats} after one warm call; G = {G} channels per launch)",
         "%-6s %-40s %9s %10s %13s" % ("scene", "what", "launches", "median_ms", "x exact blend")]
for kind in args.scenes:
    rec = pkg.synth.synth_records(n, seed=0, kind=kind)
    scene = pkg.Scene.from_records(rec, device=0)
    del rec
    rend = pkg.Renderer(scene)
    u = pkg.camera_uniforms(pkg.make_camera(), w, h)
    exact = blend_ms(rend, u, 2)
    st = rend.stats()
    stream = torch.cuda.ExternalStream(rend.stream)
    weight = torch.zeros((n,), dtype=torch.float64, device="cuda")
    rows = [("exact blend (exp mode 2), ms_render", 1, exact)]
    gen = torch.Generator(device="cuda").manual_seed(1)
    for c in args.channels:
        if c == 0:
            rows.append(("k_lift, 0 channels, weight only", 1, pass_ms(lambda: rend.lift_pixels(None, weight=weight), stream)))
            continue
        values = torch.randn((h, w, c), dtype=torch.float32, device="cuda", generator=gen)
        out = torch.zeros((n, c), dtype=torch.float64, device="cuda")
        rows.append((f"k_lift, {c} channels, out + weight", -(-c // G),
                     pass_ms(lambda: rend.lift_pixels(values, out=out, weight=weight), stream)))
        if c == 3:
            mask = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
            mask[:, :w // 2] = 1
            rows.append(("k_lift, 3 channels, half masked", 1, pass_ms(lambda: rend.lift_pixels(values, out=out, weight=weight, mask=mask), stream)))
            del mask
        del values, out
        feats = torch.randn((n, c), dtype=torch.float32, device="cuda", generator=gen)
        fmap = torch.zeros((h, w, c), dtype=torch.float32, device="cuda")
        rows.append((f"k_features, {c} channels, out only", -(-c // G), pass_ms(lambda: rend.feature_maps(features=feats, out=fmap), stream)))
        del feats, fmap
        torch.cuda.empty_cache()
    for what, launches, ms in rows:
        lines.append("%-6s %-40s %9d %10.3f %13.2f" % (kind, what, launches, ms, ms / exact))
    lines.append(f"#      {kind}({n}): V = {st.num_visible}, D = {st.num_instances} tile instances; {int((weight > 0).sum())} Gaussians were "
                 f"blended at some pixel")
    rend.close()
    scene.close()
    del weight
    torch.cuda.empty_cache()
text = "\n".join(lines) + "\n"
print(text, end="")
if args.out:
    with open(args.out, "w") as f:
        f.write(text)
