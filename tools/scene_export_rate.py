#!/usr/bin/env python3
"""How fast a scene leaves the device (gs_scene_to_device_arrays, gs_scene_save_ply), next to the ingest's rate from the same
run:

    k_scene_export, all six members     59 floats read and 59 written per Gaussian (472 B), 3 scales + 1 opacity inverted
    k_scene_export, copies only         means + quats + sh_dc + sh_rest: 55 floats each way (440 B), no arithmetic
    k_scene_export, inversions only     log_scales + opacity_logits: 4 floats each way (32 B), all of the arithmetic
    k_ingest_arrays, means + SH         51 floats each way (408 B): the ingest's own measure (tools/device_ingest_rate.py)
    k_scene_export, means + SH          the same members the other way
    download_records / save_ply         wall time of the streamed paths (kernel -> device buffer -> pinned memory -> host / file)

The kernels are timed with events on the stream (median of --repeats after one warm call), on a scene without a spatial copy
so that the kernel is all the stream runs; the streamed paths by the wall clock (they return synchronised).  "all six" close
to "copies only" means the inversions hide behind the memory traffic; the sum of "copies only" and "inversions only" means
they do not.

    python tools/scene_export_rate.py [--gaussians 1000000 6000000] [--repeats 10] [--out profiles/rNN_scene_export.txt]
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--gaussians", type=int, nargs="+", default=[1_000_000, 6_000_000])
ap.add_argument("--repeats", type=int, default=10)
ap.add_argument("--out", default=None)
args = ap.parse_args()

import torch  # noqa: E402

pkg = entry.load_package()
os.environ["GS_SPATIAL_MIN"] = str(1 << 40)  # no copy in spatial order: an update then runs k_ingest_arrays and nothing else


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
    return statistics.median(ms)


def wall_ms(fn, repeats):
    fn()
    ms = []
    for _ in range(repeats):
        t = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ms)


lines = [f"# python tools/scene_export_rate.py --gaussians {' '.join(map(str, args.gaussians))} --repeats {args.repeats}   "
         f"({torch.cuda.get_device_name(0)}; S(n) scenes; median of {args.repeats} after one warm call)",
         "%-10s %-40s %10s %14s %10s" % ("gaussians", "what", "median_ms", "Gaussians/s", "GB/s")]
for n in args.gaussians:
    rec = pkg.synth.synth_records(n, seed=0, kind="S")
    host = dict(means=rec[:, 0:3], log_scales=rec[:, 55:58], quats=rec[:, 58:62], opacity_logits=rec[:, 54], sh_dc=rec[:, 6:9],
                sh_rest=rec[:, 9:54].reshape(n, 3, 15).transpose(0, 2, 1))
    dev = {k: torch.from_numpy(v.copy()).cuda().contiguous() for k, v in host.items()}
    del rec, host
    scene = pkg.Scene.from_tensors(**dev)
    out = {k: torch.empty_like(v) for k, v in dev.items()}
    torch.cuda.synchronize()
    subset = lambda *names: {k: out[k] for k in names}  # noqa: E731
    rows = []

    def kernel(what, bytes_per, fn):
        ms = event_ms(fn)
        rows.append((what, ms, bytes_per))

    kernel("k_scene_export, all six members", 472, lambda: scene.to_tensors(out=out))
    kernel("k_scene_export, copies only", 440, lambda: scene.to_tensors(out=subset("means", "quats", "sh_dc", "sh_rest")))
    kernel("k_scene_export, inversions only", 32, lambda: scene.to_tensors(out=subset("log_scales", "opacity_logits")))
    plain = {k: dev[k] for k in ("means", "sh_dc", "sh_rest")}
    kernel("k_ingest_arrays, means + SH", 408, lambda: scene.update_from_tensors(0, **plain))
    kernel("k_scene_export, means + SH", 408, lambda: scene.to_tensors(out=subset("means", "sh_dc", "sh_rest")))
    few = max(2, args.repeats // 3)
    rows.append(("download_records (wall)", wall_ms(lambda: scene.download_records(), few), 248))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "scene.ply")
        rows.append(("save_ply (wall, file bytes)", wall_ms(lambda: scene.save_ply(path), few), 248))
    for what, ms, bytes_per in rows:
        lines.append("%-10d %-40s %10.3f %14.4g %10.1f" % (n, what, ms, n / (ms * 1e-3), n * bytes_per / (ms * 1e-3) / 1e9))
    del scene, dev, out, plain
    torch.cuda.empty_cache()
text = "\n".join(lines) + "\n"
print(text, end="")
if args.out:
    with open(args.out, "w") as f:
        f.write(text)
