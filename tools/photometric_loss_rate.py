#!/usr/bin/env python3
"""What gs_photometric_loss (gs_loss.hip) costs on a rendered frame, beside the torch formulation it replaces and the blend
backward it feeds.  Per resolution, on the frame of scene S against a fixed random target, from one run:

    loss + gradient, lambda 0.2           k_loss_ssim<maps>, k_loss_grad, k_loss_finish: the trainer's call
    forward only, lambda 0.2              k_loss_ssim, k_loss_finish: the evaluation call (grad=None)
    loss + gradient, lambda 0             k_loss_l1, k_loss_finish: no window
    torch float32, forward + backward     the yardstick: loss_utils.ssim's formulation -- five F.conv2d(padding=5, groups=3) with
                                          a 2-D window and autograd -- in float32 on the same device and images
    k_blend_backward, all four outputs    what the gradient goes into, on the same frame

A device pass of the library is timed between two events on the renderer's stream (idle before: the calls return synchronised),
the torch row between two events on torch's current stream; one warm call per pass, then --repeats ROUNDS, each round timing
every pass once in turn; median and minimum over the rounds.

    python tools/photometric_loss_rate.py [--gaussians 1000000] [--sizes 1920x1080 3840x2160] [--repeats 15] [--out FILE]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--gaussians", type=int, default=1_000_000)
ap.add_argument("--sizes", nargs="+", default=["1920x1080", "3840x2160"])
ap.add_argument("--repeats", type=int, default=15)
ap.add_argument("--out", default=None)
args = ap.parse_args()

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

pkg = entry.load_package()
n = args.gaussians


def timed(call, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    call()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def torch_window():
    k = torch.arange(11, dtype=torch.float32, device="cuda")
    g = torch.exp(-((k - 5) ** 2) / 4.5)
    g = (g / g.sum()).unsqueeze(1)
    return (g @ g.t()).expand(3, 1, 11, 11).contiguous()


def torch_step(img, gt, window, lam=0.2):
    """Forward and backward of the trainers' loss in float32; img (1, 3, H, W) requires grad."""
    img.grad = None
    mu1, mu2 = F.conv2d(img, window, padding=5, groups=3), F.conv2d(gt, window, padding=5, groups=3)
    s11 = F.conv2d(img * img, window, padding=5, groups=3) - mu1 * mu1
    s22 = F.conv2d(gt * gt, window, padding=5, groups=3) - mu2 * mu2
    s12 = F.conv2d(img * gt, window, padding=5, groups=3) - mu1 * mu2
    ssim = ((2 * mu1 * mu2 + 1e-4) * (2 * s12 + 9e-4) / ((mu1 * mu1 + mu2 * mu2 + 1e-4) * (s11 + s22 + 9e-4))).mean()
    ((1 - lam) * (img - gt).abs().mean() + lam * (1 - ssim)).backward()


lines = [f"# python tools/photometric_loss_rate.py --gaussians {n} --sizes {' '.join(args.sizes)} --repeats {args.repeats}   "
         f"({torch.cuda.get_device_name(0)}; {args.repeats} rounds after one warm call, every pass once per round)",
         "%-10s %-40s %10s %10s %26s" % ("size", "what", "median_ms", "min_ms", "x loss + gradient, 0.2")]
rec = pkg.synth.synth_records(n, seed=0, kind="S")
scene = pkg.Scene.from_records(rec, device=0)
del rec
rend = pkg.Renderer(scene)
stream = torch.cuda.ExternalStream(rend.stream)
for size in args.sizes:
    w, h = (int(v) for v in size.split("x"))
    u = pkg.camera_uniforms(pkg.make_camera(), w, h)
    rgba = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    rend.render(u, rgba.data_ptr())
    rend.synchronize()
    st = rend.stats()
    gen = torch.Generator(device="cuda").manual_seed(1)
    photo = torch.rand((h, w, 3), dtype=torch.float32, device="cuda", generator=gen)
    grad = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
    terms = torch.empty((4,), dtype=torch.float64, device="cuda")
    f64 = dict(dtype=torch.float64, device="cuda")
    sums = dict(colour=torch.zeros((n, 3), **f64), opacity=torch.zeros((n,), **f64), conic=torch.zeros((n, 3), **f64), uv=torch.zeros((n, 2), **f64))
    img = rgba[..., :3].permute(2, 0, 1).unsqueeze(0).contiguous().requires_grad_()
    gt = photo.permute(2, 0, 1).unsqueeze(0).contiguous()
    window = torch_window()
    here = torch.cuda.current_stream()
    passes = [("loss + gradient, lambda 0.2", lambda: rend.photometric_loss(rgba, photo, 0.2, grad=grad, terms=terms), stream),
              ("forward only, lambda 0.2", lambda: rend.photometric_loss(rgba, photo, 0.2, grad=None, terms=terms), stream),
              ("loss + gradient, lambda 0", lambda: rend.photometric_loss(rgba, photo, 0.0, grad=grad, terms=terms), stream),
              ("torch float32, forward + backward", lambda: torch_step(img, gt, window), here),
              ("k_blend_backward, all four outputs", lambda: rend.blend_backward(grad, None, **sums), stream)]
    for _, call, _ in passes:
        call()
    torch.cuda.synchronize()
    ms = {what: [] for what, _, _ in passes}
    for _ in range(args.repeats):
        for what, call, s in passes:
            ms[what].append(timed(call, s))
    yard = statistics.median(ms[passes[0][0]])
    for what, _, _ in passes:
        med = statistics.median(ms[what])
        lines.append("%-10s %-40s %10.3f %10.3f %26.2f" % (size, what, med, min(ms[what]), med / yard))
    rend.photometric_loss(rgba, photo, 0.2, grad=grad, terms=terms)
    lines.append(f"#      {size}: S({n}), V = {st.num_visible} visible Gaussians; loss, l1, ssim, mse = "
                 + ", ".join(f"{float(v):.6g}" for v in terms.cpu()) + f"; scratch {72 * w * h / 2**20:.0f} MiB of P maps")
    del rgba, photo, grad, terms, sums, img, gt, passes
    torch.cuda.empty_cache()
rend.close()
scene.close()
text = "\n".join(lines) + "\n"
print(text, end="")
if args.out:
    with open(args.out, "w") as f:
        f.write(text)
