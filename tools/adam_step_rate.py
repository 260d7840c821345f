#!/usr/bin/env python3
"""What the optimiser's step costs on the device (gs_scene_adam_step: k_adam_step, gs_optim.hip, and the scene's derived passes
behind it) next to what it replaces, on the same tensors, after a real frame's backward.  Per scene, at one resolution, from one run:

    Scene.adam_step, visible mask      all six groups, zero_grads, under the frame's visible mask (Renderer.visible_mask)
    Scene.adam_step, mask of ones      the same with every Gaussian stepped
    what it replaces, piece by piece   zero-fill of the six float64 gradient tensors; their conversion to float32; torch.optim.Adam.step()
                                       over all N (torch's default implementation, and fused=True where this torch takes it);
                                       Scene.update_from_tensors(0, all six); and the sum of the pieces (with the faster Adam)
    k_blend_backward, all four outputs the common yardstick of tools/project_backward_rate.py

A call is timed between two events on the stream it runs on (torch's current stream for the step and the torch pieces -- the step
returns synchronised, so its span is the launches, the kernels, the flag's copy back and the host's part of the call; the renderer's
stream for the blend's backward).  One warm call each, then --repeats ROUNDS, each round timing every item once in turn; median and
minimum over the rounds.  The step consumes its gradients (zero_grads): before every timed step they are copied back from a saved
copy, outside the span.  Parameters drift over the rounds by a few learning rates, which changes no cost.

The traffic count of the step under a mask of V Gaussians is V x (59 x (8 B gradient in + 8 B out + 4 B in and out for each of
parameter, exp_avg, exp_avg_sq) + 236 B of blob) = V x 2596 B; the bytes per second quoted are that count over the WHOLE call's median,
derived passes included, so they understate the kernel's own.

    python tools/adam_step_rate.py [--gaussians 1000000] [--scenes S T] [--width 1920 --height 1080] [--repeats 15] [--out FILE]
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
LR = dict(means=1.6e-4, log_scales=5e-3, quats=1e-3, opacity_logits=5e-2, sh_dc=2.5e-3, sh_rest=1.25e-4)
BYTES_PER_GAUSSIAN = 59 * (8 + 8 + 4 * 6) + 236


def timed(call, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    call()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


lines = [f"# python tools/adam_step_rate.py --gaussians {n} --scenes {' '.join(args.scenes)} --width {w} --height {h} "
         f"--repeats {args.repeats}   ({torch.cuda.get_device_name(0)}; {args.repeats} rounds after one warm call, every item once per round)",
         "%-6s %-58s %10s %10s %18s" % ("scene", "what", "median_ms", "min_ms", "x k_blend_backward")]
for kind in args.scenes:
    rec = pkg.synth.synth_records(n, seed=0, kind=kind)
    scene = pkg.Scene.from_records(rec, device=0)
    del rec
    params = scene.to_tensors()                                   # the trainer's six float32 tensors, as the scene holds them
    rend = pkg.Renderer(scene)
    u = pkg.camera_uniforms(pkg.make_camera(), w, h)
    rend.render_host(u, want_rgba=True)
    st = rend.stats()
    gen = torch.Generator(device="cuda").manual_seed(1)
    grad_rgb = torch.randn((h, w, 3), dtype=torch.float32, device="cuda", generator=gen)
    f64 = dict(dtype=torch.float64, device="cuda")
    d = dict(colour=torch.zeros((n, 3), **f64), opacity=torch.zeros((n,), **f64), conic=torch.zeros((n, 3), **f64), uv=torch.zeros((n, 2), **f64))
    rend.blend_backward(grad_rgb, None, **d)
    grads = {k: torch.zeros_like(v, dtype=torch.float64) for k, v in params.items()}
    rend.project_backward(out=grads, **d)
    saved = {k: v.clone() for k, v in grads.items()}
    visible = rend.visible_mask()
    ones = torch.ones_like(visible)
    v_count = int(visible.sum().item())
    with_gradient = int((saved["opacity_logits"] != 0).sum().item())
    rend.synchronize()
    opt = pkg.Adam(scene, params, lr=LR)
    cur = torch.cuda.current_stream()
    rstream = torch.cuda.ExternalStream(rend.stream)

    def refill():
        for k, v in saved.items():
            grads[k].copy_(v)
        torch.cuda.synchronize()

    def step(mask):
        def call():
            opt.step(grads, mask=mask)
        return call

    # what the step replaces: torch's optimiser on float32 copies of the same parameters, fed the same gradients
    tparams = {k: v.clone().requires_grad_() for k, v in params.items()}
    groups = [dict(params=[tparams[k]], lr=LR[k]) for k in tparams]
    adams = {"default": torch.optim.Adam(groups, eps=1e-15)}
    try:
        fused = torch.optim.Adam([dict(params=[p.detach().clone().requires_grad_()], lr=LR[k]) for k, p in tparams.items()], eps=1e-15, fused=True)
        for g, k in zip(fused.param_groups, tparams):
            g["params"][0].grad = saved[k].float()
        fused.step()
        adams["fused=True"] = fused
    except Exception as e:  # this torch does not take fused=True on this device: said in the table
        lines.append(f"#      torch.optim.Adam(fused=True) is not available here: {type(e).__name__}: {str(e).splitlines()[0][:120]}")
    g32 = {}

    def zero_fill():
        for g in grads.values():
            g.zero_()

    def convert():
        for k, g in grads.items():
            g32[k] = g.float()

    def adam(o):
        def call():
            for g, k in zip(o.param_groups, tparams):
                g["params"][0].grad = g32[k]
            o.step()
        return call

    def ingest():
        scene.update_from_tensors(0, **params)

    items = [("Scene.adam_step, six groups, zero_grads, visible mask", step(visible), cur, refill),
             ("Scene.adam_step, six groups, zero_grads, mask of ones", step(ones), cur, refill),
             ("replaced: zero-fill of six float64 gradient tensors", zero_fill, cur, None),
             ("replaced: float64 -> float32 of the six gradients", convert, cur, refill)]
    items += [(f"replaced: torch.optim.Adam.step(), {name}, all N", adam(o), cur, None) for name, o in adams.items()]
    items += [("replaced: Scene.update_from_tensors(0, all six)", ingest, cur, None),
              ("k_blend_backward, all four outputs", lambda: rend.blend_backward(grad_rgb, None, **d), rstream, None)]
    for _, call, _, before in items:
        if before:
            before()
        call()
    torch.cuda.synchronize()
    ms = {what: [] for what, _, _, _ in items}
    for _ in range(args.repeats):
        for what, call, s, before in items:
            if before:
                before()
            ms[what].append(timed(call, s))
    med = {what: statistics.median(v) for what, v in ms.items()}
    blend = med[items[-1][0]]
    for what, _, _, _ in items:
        lines.append("%-6s %-58s %10.3f %10.3f %18.2f" % (kind, what, med[what], min(ms[what]), med[what] / blend))
    best_adam = min(med[w_] for w_ in med if "torch.optim.Adam" in w_)
    total = sum(med[w_] for w_ in med if w_.startswith("replaced") and "torch.optim.Adam" not in w_) + best_adam
    lines.append("%-6s %-58s %10.3f %10s %18.2f" % (kind, "replaced: the sum of the pieces (the faster Adam)", total, "", total / blend))
    sparse, dense = med[items[0][0]], med[items[1][0]]
    lines.append(f"#      {kind}({n}): V = {st.num_visible} visible Gaussians ({v_count} in the mask), {with_gradient} carry a gradient; "
                 f"the traffic count V x {BYTES_PER_GAUSSIAN} B = {v_count * BYTES_PER_GAUSSIAN / 1e9:.3f} GB in {sparse:.3f} ms = "
                 f"{v_count * BYTES_PER_GAUSSIAN / sparse / 1e9:.2f} TB/s over the whole call; mask of ones: {n * BYTES_PER_GAUSSIAN / 1e9:.3f} GB, "
                 f"{n * BYTES_PER_GAUSSIAN / dense / 1e9:.2f} TB/s")
    rend.close()
    scene.close()
    del grad_rgb, d, grads, saved, params, tparams, adams, g32, opt, items
    torch.cuda.empty_cache()
text = "\n".join(lines) + "\n"
print(text, end="")
if args.out:
    with open(args.out, "w") as f:
        f.write(text)
