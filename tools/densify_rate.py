#!/usr/bin/env python3
"""What adaptive density control costs on the device (gs_accumulate_densify_stats, gs_densify_plan, gs_densify_apply:
gs_densify.hip) next to what it replaces, on the same tensors, after a real frame's backward.  Per scene, at one resolution, from
one run:

    Renderer.densify_stats             the statistic of the frame (one lane per Gaussian)
    gs_densify_plan                    the decision and its two prefix sums, counts back on the host
    gs_densify_apply                   the compaction of six parameter and twelve moment arrays into preallocated outputs
    pkg.densify                        plan, torch.randn, the allocation of the outputs, apply, the per-outcome counts
    replaced: the trainers' sequence   formulation (b) of tests/densify_reference.py in float32 torch ON THE DEVICE, moments included:
                                       boolean masks, cat of clones, cat of split children (build_rotation, bmm, log(exp / 1.6)), removal
                                       of the split parents, the prune over the extended set
    k_blend_backward, all four outputs the common yardstick of tools/project_backward_rate.py

The rule is tuned from the scene's own quantiles so that roughly 5 % of the Gaussians clone, 5 % split and 5 % are pruned; the
counts that came out are recorded.  A call is timed between two events on the stream it runs on (torch's current stream; the
renderer's for the statistic and the blend's backward); the calls return synchronised, so a span is the launches, the kernels,
the copies back and the host's part.  One warm call each, then --repeats ROUNDS, each round timing every item once in turn; median
and minimum over the rounds.

The traffic count of the apply per OUTPUT row: every given array read once and written once, 59 x 3 floats x (4 B + 4 B) = 1416 B,
plus per PARENT the four offsets it reads (16 B); the bytes per second quoted are that count over the whole call's median.

    python tools/densify_rate.py [--gaussians 1000000] [--scenes S T] [--width 1920 --height 1080] [--repeats 15] [--out FILE]
"""
import argparse
import ctypes as C
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
b, L = pkg.binding, pkg.binding.lib()
w, h, n = args.width, args.height, args.gaussians
NAMES = b.PARAMETER_NAMES
BYTES_PER_ROW, BYTES_PER_PARENT = 59 * 3 * 8, 16


def timed(call, stream):
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    call()
    z.record(stream)
    z.synchronize()
    return a.elapsed_time(z)


def build_rotation(r):
    q = r / torch.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2] + r[:, 3] * r[:, 3])[:, None]
    R = torch.zeros((q.size(0), 3, 3), device=r.device)
    s, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = 1 - 2 * (y * y + z * z), 2 * (x * y - s * z), 2 * (x * z + s * y)
    R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = 2 * (x * y + s * z), 1 - 2 * (x * x + z * z), 2 * (y * z - s * x)
    R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = 2 * (x * z - s * y), 2 * (y * z + s * x), 1 - 2 * (x * x + y * y)
    return R


def trainer_sequence(params, state, stats, rule):
    """Formulation (b) on the device: returns the new parameters and moments (the trainers' order)."""
    t = dict(params)
    mom = {what: dict(state[what]) for what in state}
    avg = (stats["grad_sum"] / stats["count"]).float()
    avg[avg.isnan()] = 0.0
    radii = stats["max_radius"]

    def extend(rows, changed):
        for k in t:
            for what in mom:
                mom[what][k] = torch.cat([mom[what][k], torch.zeros_like(mom[what][k][rows])])
            t[k] = torch.cat([t[k], changed.get(k, t[k][rows])])

    grow = avg >= rule["grad_threshold"]
    clone = grow & (torch.exp(t["log_scales"]).max(dim=1).values <= rule["dense_extent"])
    count = int(clone.sum())
    extend(clone, {})
    radii = torch.cat([radii, torch.zeros(count, device="cuda")])
    grow = torch.cat([grow, torch.zeros(count, dtype=torch.bool, device="cuda")])
    split = grow & (torch.exp(t["log_scales"]).max(dim=1).values > rule["dense_extent"])
    stds = torch.exp(t["log_scales"][split]).repeat(2, 1)
    samples = torch.normal(mean=torch.zeros_like(stds), std=stds)
    rots = build_rotation(t["quats"][split]).repeat(2, 1, 1)
    means = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + t["means"][split].repeat(2, 1)
    log_scales = torch.log(torch.exp(t["log_scales"][split].repeat(2, 1)) / 1.6)
    twice = torch.nonzero(split).reshape(-1).repeat(2)
    extend(twice, dict(means=means, log_scales=log_scales))
    radii = torch.cat([radii, torch.zeros(len(twice), device="cuda")])
    keep = ~torch.cat([split, torch.zeros(len(twice), dtype=torch.bool, device="cuda")])
    keep &= ~(torch.sigmoid(t["opacity_logits"].reshape(-1)) < rule["min_opacity"])
    if rule["max_screen_radius"] > 0:
        keep &= ~(radii > rule["max_screen_radius"])
    if rule["max_world_scale"] > 0:
        keep &= ~(torch.exp(t["log_scales"]).max(dim=1).values > rule["max_world_scale"])
    return {k: v[keep] for k, v in t.items()}, {what: {k: v[keep] for k, v in mom[what].items()} for what in mom}


lines = [f"# python tools/densify_rate.py --gaussians {n} --scenes {' '.join(args.scenes)} --width {w} --height {h} "
         f"--repeats {args.repeats}   ({torch.cuda.get_device_name(0)}; {args.repeats} rounds after one warm call, every item once per round)",
         "%-6s %-58s %10s %10s %18s" % ("scene", "what", "median_ms", "min_ms", "x k_blend_backward")]
for kind in args.scenes:
    rec = pkg.synth.synth_records(n, seed=0, kind=kind)
    scene = pkg.Scene.from_records(rec, device=0)
    del rec
    params = scene.to_tensors()
    rend = pkg.Renderer(scene)
    u = pkg.camera_uniforms(pkg.make_camera(), w, h)
    rend.render_host(u, want_rgba=True)
    gen = torch.Generator(device="cuda").manual_seed(1)
    grad_rgb = torch.randn((h, w, 3), dtype=torch.float32, device="cuda", generator=gen)
    f64 = dict(dtype=torch.float64, device="cuda")
    d = dict(colour=torch.zeros((n, 3), **f64), opacity=torch.zeros((n,), **f64), conic=torch.zeros((n, 3), **f64), uv=torch.zeros((n, 2), **f64))
    rend.blend_backward(grad_rgb, None, **d)
    stats = pkg.densify_stats_zeros(scene)
    rend.densify_stats(d["uv"], stats)
    state = dict(exp_avg={k: torch.randn_like(v) for k, v in params.items()}, exp_avg_sq={k: torch.rand_like(v) for k, v in params.items()})
    # the rule from the scene's own quantiles: 10 % grow, half of them small; the faintest 5 % go
    seen = stats["count"] != 0
    avg = (stats["grad_sum"] / stats["count"])[seen]
    scale = torch.exp(params["log_scales"]).max(dim=1).values
    threshold = float(torch.quantile(avg[torch.randperm(len(avg), device="cuda")[:1_000_000]], max(0.0, 1.0 - 0.10 * n / max(1, int(seen.sum())))))
    growing = torch.zeros(n, dtype=torch.bool, device="cuda")
    growing[seen] = avg >= threshold
    rule = dict(grad_threshold=threshold, dense_extent=float(scale[growing].median()),
                min_opacity=float(torch.quantile(torch.sigmoid(params["opacity_logits"].reshape(-1))[:1_000_000], 0.05)),
                max_screen_radius=0.0, max_world_scale=0.0)
    rend.synchronize()
    cur = torch.cuda.current_stream()
    rstream = torch.cuda.ExternalStream(rend.stream)

    new_params, new_state, info = pkg.densify(scene, params, rule, stats, state)
    n_out, n_noise = info["n_out"], info["n_noise"]
    noise = torch.randn((n_noise, 2, 3), device="cuda")
    scratch = torch.empty(2 * (n + 1), dtype=torch.int32, device="cuda")
    inp, out = b.DensifyInput(), b.DensifyOutput()
    for g, name in enumerate(NAMES):
        setattr(inp.params, name, params[name].data_ptr())
        setattr(out.params, name, new_params[name].data_ptr())
        out.exp_avg[g], out.exp_avg_sq[g] = state["exp_avg"][name].data_ptr(), state["exp_avg_sq"][name].data_ptr()
        out.out_exp_avg[g], out.out_exp_avg_sq[g] = new_state["exp_avg"][name].data_ptr(), new_state["exp_avg_sq"][name].data_ptr()
    inp.params.sh_rest_coeffs = out.params.sh_rest_coeffs = int(params["sh_rest"].shape[1])
    inp.grad_sum, inp.count, inp.max_radius = (stats[k].data_ptr() for k in ("grad_sum", "count", "max_radius"))
    inp.scratch, inp.rule = scratch.data_ptr(), b._densify_rule(rule)
    out.noise, out.n_noise, out.n_out = noise.data_ptr(), n_noise, n_out
    counts = (C.c_uint64(0), C.c_uint64(0))
    handle = C.c_void_p(cur.cuda_stream or None)
    torch.cuda.synchronize()

    def plan():
        b._check(L.gs_densify_plan(C.byref(inp), C.c_uint64(n), 0, handle, C.byref(counts[0]), C.byref(counts[1])))

    def apply():
        b._check(L.gs_densify_apply(C.byref(inp), C.c_uint64(n), C.byref(out), 0, handle))

    kept = {}

    def whole():
        kept["new"] = pkg.densify(scene, params, rule, stats, state)

    def replaced():
        kept["old"] = trainer_sequence(params, state, stats, rule)

    spare = pkg.densify_stats_zeros(scene)            # (the timed statistic accumulates here: the rule's statistics stay as they are)
    items = [("Renderer.densify_stats", lambda: rend.densify_stats(d["uv"], spare), rstream),
             ("gs_densify_plan", plan, cur), ("gs_densify_apply, 6 parameter + 12 moment arrays", apply, cur),
             ("pkg.densify: plan, randn, allocation, apply, counts", whole, cur),
             ("replaced: the trainers' sequence in float32 torch", replaced, cur),
             ("k_blend_backward, all four outputs", lambda: rend.blend_backward(grad_rgb, None, **d), rstream)]
    for _, call, _ in items:
        call()
    torch.cuda.synchronize()
    assert (counts[0].value, counts[1].value) == (n_out, n_noise) and len(kept["old"][0]["means"]) == n_out
    ms = {what: [] for what, _, _ in items}
    for _ in range(args.repeats):
        for what, call, s in items:
            ms[what].append(timed(call, s))
    med = {what: statistics.median(v) for what, v in ms.items()}
    blend = med[items[-1][0]]
    for what, _, _ in items:
        lines.append("%-6s %-58s %10.3f %10.3f %18.2f" % (kind, what, med[what], min(ms[what]), med[what] / blend))
    traffic = n_out * BYTES_PER_ROW + n * BYTES_PER_PARENT
    lines.append(f"#      {kind}({n}): {int(seen.sum())} seen by the frame; parents removed {info['parents_removed']}, single {info['parents_single']}, "
                 f"cloned {info['parents_cloned']}, split {info['parents_split']}; n_out = {n_out}; the apply's traffic count n_out x {BYTES_PER_ROW} B "
                 f"+ n x {BYTES_PER_PARENT} B = {traffic / 1e9:.3f} GB in {med[items[2][0]]:.3f} ms = {traffic / med[items[2][0]] / 1e9:.2f} TB/s over the whole call")
    rend.close()
    scene.close()
    del grad_rgb, d, params, state, stats, new_params, new_state, kept, noise, scratch
    torch.cuda.empty_cache()
text = "\n".join(lines) + "\n"
print(text, end="")
if args.out:
    with open(args.out, "w") as f:
        f.write(text)
