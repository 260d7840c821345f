#!/usr/bin/env python3
"""What moving a scene on the device costs (Scene.transform, gs_scene_transform):

    transform (whole scene)   wall time of the call: k_scene_transform + cov3D (+ the spatial copy from 4 M on), returns synchronised
    transform (1 % range)     the same for n / 100 Gaussians in the middle of the scene
    update (1 % range)        Scene.update_from_tensors of the same range, all members: the call a rigid motion would otherwise take

Each is warmed once, then the median of --repeats is taken, all in one process.  The kernels are timed with events on the
stream, on a scene without a spatial copy.  The call always runs k_cov3d behind k_scene_transform, so the events bracket both;
an update of the scales alone (k_ingest_arrays over 3 floats + k_cov3d) is timed beside it to show k_cov3d's share.
The yardstick is k_ingest_arrays, timed as tools/device_ingest_rate.py times it (an update of positions + SH: 51 floats in,
51 out per Gaussian), in the same process.

    python tools/scene_transform_rate.py [--gaussians 1000000 6000000] [--repeats 10] [--out profiles/rNN_scene_transform.txt]

THE KERNEL ALONE.  gs_scene_transform returns synchronised and always runs k_cov3d behind the kernel, so no pair of events of
the caller's can bracket k_scene_transform by itself.  --kernel-loop N is the driver for a profiler instead: on one S(N) scene
without a spatial copy it alternates --repeats whole-scene transforms with as many whole-scene updates of positions + SH
(k_ingest_arrays, the yardstick) and prints nothing else; the per-kernel durations and counters come from

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o ka -- python tools/scene_transform_rate.py --kernel-loop 6000000
    rocprofv3 --kernel-trace --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE --output-format csv -d OUT -o lds -- python tools/... (a run of its own)
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--gaussians", type=int, nargs="+", default=[1_000_000, 6_000_000])
ap.add_argument("--repeats", type=int, default=10)
ap.add_argument("--out", default=None)
ap.add_argument("--kernel-loop", type=int, default=0, metavar="N", help="only alternate transforms and position + SH updates of an S(N) scene (for a profiler)")
args = ap.parse_args()

import torch  # noqa: E402

pkg = entry.load_package()
MOVE = dict(rotation=(0.61, -0.33, 0.52, 0.49), translation=(0.7, -1.3, 0.45), scale=1.01)
if args.kernel_loop:
    os.environ["GS_SPATIAL_MIN"] = str(1 << 40)
    n = args.kernel_loop
    rec = pkg.synth.synth_records(n, seed=0, kind="S")
    dev = dict(means=rec[:, 0:3], log_scales=rec[:, 55:58], quats=rec[:, 58:62], opacity_logits=rec[:, 54], sh_dc=rec[:, 6:9],
               sh_rest=rec[:, 9:54].reshape(n, 3, 15).transpose(0, 2, 1))
    dev = {k: torch.from_numpy(v.copy()).cuda().contiguous() for k, v in dev.items()}
    scene = pkg.Scene.from_tensors(**dev)
    for i in range(args.repeats + 1):
        scene.transform(rotation=(0.61, -0.33 if i % 2 else 0.33, 0.52, 0.49), translation=(0.1, 0.2, 0.3), scale=1.01 if i % 2 else 1 / 1.01)
        scene.update_from_tensors(0, means=dev["means"], sh_dc=dev["sh_dc"], sh_rest=dev["sh_rest"])
    print(f"kernel loop: {args.repeats + 1} transforms and updates of S({n})")
    sys.exit(0)
BACK = dict(rotation=(0.61, 0.33, -0.52, -0.49), translation=(0.0, 0.0, 0.0), scale=1 / 1.01)  # keeps the scales in range over many repeats


def wall_ms(fn):
    fn()  # warm
    ms = []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ms), min(ms), max(ms)


def event_ms(fn):
    fn()
    ms = []
    for _ in range(args.repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


lines = [f"# python tools/scene_transform_rate.py --gaussians {' '.join(map(str, args.gaussians))} --repeats {args.repeats}   "
         f"({torch.cuda.get_device_name(0)}; S(n) scenes; median [min .. max] of {args.repeats} after one warm call)",
         "%-10s %-26s %12s %22s %14s" % ("gaussians", "path", "median_ms", "[min .. max]", "Gaussians/s")]
for n in args.gaussians:
    rec = pkg.synth.synth_records(n, seed=0, kind="S")
    host = dict(means=rec[:, 0:3], log_scales=rec[:, 55:58], quats=rec[:, 58:62], opacity_logits=rec[:, 54], sh_dc=rec[:, 6:9],
                sh_rest=rec[:, 9:54].reshape(n, 3, 15).transpose(0, 2, 1))
    dev = {k: torch.from_numpy(v.copy()).cuda().contiguous() for k, v in host.items()}
    torch.cuda.synchronize()
    scene = pkg.Scene.from_tensors(**dev)
    state = [0]

    def move(first=0, count=None, s=scene):
        state[0] ^= 1
        s.transform(first=first, count=count, **(MOVE if state[0] else BACK))

    m, first = max(1, n // 100), n // 2
    part = {k: v[first:first + m] for k, v in dev.items()}
    rows = [("transform (whole scene)", wall_ms(move), n), ("transform (1 % range)", wall_ms(lambda: move(first, m)), m),
            ("update (1 % range)", wall_ms(lambda: scene.update_from_tensors(first, **part)), m)]
    del scene
    for name, (med, lo, hi), count in rows:
        lines.append("%-10d %-26s %12.3f %22s %14.4g" % (n, name, med, f"[{lo:.3f} .. {hi:.3f}]", count / (med * 1e-3)))
    # the kernels alone: a scene without a spatial copy, events on the stream
    old = os.environ.get("GS_SPATIAL_MIN")
    os.environ["GS_SPATIAL_MIN"] = str(1 << 40)
    flat = pkg.Scene.from_tensors(**dev)
    if old is None:
        del os.environ["GS_SPATIAL_MIN"]
    else:
        os.environ["GS_SPATIAL_MIN"] = old
    plain = {k: dev[k] for k in ("means", "sh_dc", "sh_rest")}
    k_ing = event_ms(lambda: flat.update_from_tensors(0, **plain))
    k_cov = event_ms(lambda: flat.update_from_tensors(0, log_scales=dev["log_scales"]))
    k_tra = event_ms(lambda: move(s=flat))
    lines.append(f"#   k_ingest_arrays (means + sh_dc + sh_rest: 51 floats in, 51 out = {n * 408 / 1e6:.0f} MB), events on the stream: "
                 f"{k_ing[0]:.3f} ms [{k_ing[1]:.3f} .. {k_ing[2]:.3f}] = {n * 408 / (k_ing[0] * 1e-3) / 1e9:.0f} GB/s of algorithmic bytes")
    lines.append(f"#   scales alone (k_ingest_arrays over 3 floats + k_cov3d: 10 floats in, 6 out): {k_cov[0]:.3f} ms [{k_cov[1]:.3f} .. {k_cov[2]:.3f}]")
    lines.append(f"#   k_scene_transform (55 floats in, 55 out = {n * 440 / 1e6:.0f} MB) + k_cov3d, events on the stream: {k_tra[0]:.3f} ms "
                 f"[{k_tra[1]:.3f} .. {k_tra[2]:.3f}]: the transform alone moves at least {n * 440 / (k_tra[0] * 1e-3) / 1e9:.0f} GB/s of algorithmic bytes "
                 f"(cov3D's time left in; per-kernel times: rocprofv3 --kernel-trace --stats)")
    del flat, dev, part, plain
    torch.cuda.empty_cache()
text = "\n".join(lines) + "\n"
print(text, end="")
if args.out:
    with open(args.out, "w") as f:
        f.write(text)
