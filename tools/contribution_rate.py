#!/usr/bin/env python3
"""What gs_accumulate_contributions (k_contrib, gs_contrib.hip) costs next to the frame it describes.  Per scene, at one
resolution, from one run:

    exact blend, ms_render              the yardstick: gs_get_stats' ms_render of the same frame in exp mode 2 (blend start to
                                        frame end, stamped by the kernels) -- the same walk with the same exp, plus the colour
                                        accumulate and the image stores, minus the reduction and the atomics
    default blend, ms_render            the same frame in exp mode 3, for scale
    k_contrib, all outputs              weight + pixels + top_id
    k_contrib, pixels only              no wave reduction of q, no 64-bit atomics
    k_contrib, top_id only              no atomics at all: the walk, the staging and the barriers
    k_contrib, 1 % mask, all outputs    a centred rectangle of 1 % of the frame: the tiles without a counted pixel return at once

The pass is timed between two events on the stream it runs on (the renderer's, idle before: the call returns synchronised, so
the span is the launch, the kernel and nothing else); median of --repeats after one warm call.

How many atomics that was: the pass issues one 64-bit and one 32-bit atomic add per (tile, entry) pair some counted pixel
blends, one lane per address.  The frame's instance count D (gs_get_stats) bounds the pairs from above, so
(all outputs - top_id only) / D bounds what a flushed pair costs -- reduction, two LDS atomics, two global atomics -- from below.

    python tools/contribution_rate.py [--gaussians 1000000] [--scenes S T] [--width 1920 --height 1080] [--repeats 15] [--out FILE]
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


def pass_ms(rend, stream, **tensors):
    rend.contributions(**tensors)
    ms = []
    for _ in range(args.repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        rend.contributions(**tensors)
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


lines = [f"# python tools/contribution_rate.py --gaussians {n} --scenes {' '.join(args.scenes)} --width {w} --height {h} --repeats {args.repeats}"
         f"   ({torch.cuda.get_device_name(0)}; median of {args.repeats} after one warm call)",
         "%-6s %-36s %10s %12s" % ("scene", "what", "median_ms", "x exact blend")]
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
    weight = torch.zeros(n, dtype=torch.int64, device="cuda")
    pixels = torch.zeros(n, dtype=torch.int32, device="cuda")
    top_id = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    mask = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    mh, mw = max(1, round(h * 0.1)), max(1, round(w * 0.1))
    mask[(h - mh) // 2:(h - mh) // 2 + mh, (w - mw) // 2:(w - mw) // 2 + mw] = 1
    rows = [("default blend (exp mode 3), ms_render", default), ("exact blend (exp mode 2), ms_render", exact),
            ("k_contrib, all outputs", pass_ms(rend, stream, weight=weight, pixels=pixels, top_id=top_id)),
            ("k_contrib, pixels only", pass_ms(rend, stream, pixels=pixels)),
            ("k_contrib, top_id only", pass_ms(rend, stream, top_id=top_id)),
            ("k_contrib, 1 % mask, all outputs", pass_ms(rend, stream, weight=weight, pixels=pixels, top_id=top_id, mask=mask))]
    for what, ms in rows:
        lines.append("%-6s %-36s %10.3f %12.2f" % (kind, what, ms, ms / exact))
    # how many atomics that was: one 64-bit and one 32-bit add per (tile, entry) some counted pixel blends
    pixels.zero_()
    rend.contributions(pixels=pixels)
    touched = int((pixels != 0).sum())
    blended = int(pixels.sum(dtype=torch.int64))
    extra = rows[2][1] - rows[4][1]
    lines.append(f"#      {kind}({n}): V = {st.num_visible}, D = {st.num_instances} tile instances >= the flushed (tile, entry) pairs; {touched} Gaussians "
                 f"blended somewhere, {blended} blended (pixel, entry) pairs; all outputs - top_id only = {extra:.3f} ms = "
                 f"{extra * 1e6 / max(1, st.num_instances):.2f} ns per instance")
    rend.close()
    scene.close()
    del weight, pixels, top_id, mask
    torch.cuda.empty_cache()
text = "\n".join(lines) + "\n"
print(text, end="")
if args.out:
    with open(args.out, "w") as f:
        f.write(text)
