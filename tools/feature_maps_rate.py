#!/usr/bin/env python3
"""What gs_blend_features (k_features, gs_features.hip) costs next to the frame it describes.  Per scene, at one resolution, from
one run:

    exact blend, ms_render              the yardstick: gs_get_stats' ms_render of the same frame in exp mode 2 (blend start to
                                        frame end, stamped by the kernels) -- the same walk with the same exp and three channels
    default blend, ms_render            the same frame in exp mode 3, for scale
    k_features, C channels, all maps    C in --channels (0: alpha and the two depths alone, the channel-less instantiation; G = 16
                                        is one full group, one launch; 64 is four launches, each walking the lists again)
    k_features, 3 channels, out only    without the three [H][W] stores

The pass is timed between two events on the stream it runs on (the renderer's, idle before: the call returns synchronised, so
the span is the launches, the kernels and nothing else); median of --repeats after one warm call per shape.  Every figure of
one scene is taken on the same frame.

    python tools/feature_maps_rate.py [--gaussians 1000000] [--scenes S T] [--width 1920 --height 1080] [--channels 0 3 16 64]
                                      [--repeats 15] [--out FILE]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

G = 16  # gs_kernels.h: kFeatureGroup

ap = argparse.ArgumentParser()
ap.add_argument("--gaussians", type=int, default=1_000_000)
ap.add_argument("--scenes", nargs="+", default=["S", "T"])
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--channels", type=int, nargs="+", default=[0, 3, G, 64])
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


def pass_ms(rend, stream, **tensors):
    rend.feature_maps(**tensors)
    ms = []
    for _ in range(args.repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        rend.feature_maps(**tensors)
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


lines = [f"# python tools/feature_maps_rate.py --gaussians {n} --scenes {' '.join(args.scenes)} --width {w} --height {h} "
         f"--channels {' '.join(str(c) for c in args.channels)} --repeats {args.repeats}"
         f"   ({torch.cuda.get_device_name(0)}; median of {args.repeats} after one warm call; G = {G} channels per launch)",
         "%-6s %-40s %9s %10s %13s" % ("scene", "what", "launches", "median_ms", "x exact blend")]
for kind in args.scenes:
    rec = pkg.synth.synth_records(n, seed=0, kind=kind)
    scene = pkg.Scene.from_records(rec, device=0)
    del rec
    rend = pkg.Renderer(scene)
    u = pkg.camera_uniforms(pkg.make_camera(), w, h)
    default = blend_ms(rend, u, 3)
    exact = blend_ms(rend, u, 2)          # (last: the frame the pass walks below is this mode's -- the lists are the same in every mode)
    st = rend.stats()
    stream = torch.cuda.ExternalStream(rend.stream)
    alpha, depth, median = (torch.zeros((h, w), dtype=torch.float32, device="cuda") for _ in range(3))
    rows = [("default blend (exp mode 3), ms_render", 1, default), ("exact blend (exp mode 2), ms_render", 1, exact)]
    gen = torch.Generator(device="cuda").manual_seed(1)
    for c in args.channels:
        if c == 0:
            rows.append(("k_features, 0 channels, alpha + depths", 1, pass_ms(rend, stream, alpha=alpha, depth=depth, median_depth=median)))
            continue
        feats = torch.randn((n, c), dtype=torch.float32, device="cuda", generator=gen)
        out = torch.zeros((h, w, c), dtype=torch.float32, device="cuda")
        rows.append((f"k_features, {c} channels, all maps", -(-c // G),
                     pass_ms(rend, stream, features=feats, out=out, alpha=alpha, depth=depth, median_depth=median)))
        if c == 3:
            rows.append(("k_features, 3 channels, out only", 1, pass_ms(rend, stream, features=feats, out=out)))
        del feats, out
        torch.cuda.empty_cache()
    for what, launches, ms in rows:
        lines.append("%-6s %-40s %9d %10.3f %13.2f" % (kind, what, launches, ms, ms / exact))
    covered = int((alpha > 0).sum())
    lines.append(f"#      {kind}({n}): V = {st.num_visible}, D = {st.num_instances} tile instances; {covered} of {w * h} pixels have alpha > 0, "
                 f"{int(torch.isfinite(median).sum())} a finite median depth")
    rend.close()
    scene.close()
    del alpha, depth, median
    torch.cuda.empty_cache()
text = "\n".join(lines) + "\n"
print(text, end="")
if args.out:
    with open(args.out, "w") as f:
        f.write(text)
