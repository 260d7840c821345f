#!/usr/bin/env python3
"""How long the ways into a scene take for a model that already lies in HBM (a trainer's six tensors), against the host
path for the same numbers:

    from_records            Scene.from_records of the (n, 62) host records: CPU activation, 236 B / Gaussian over PCIe
    from_tensors            Scene.from_tensors of the six device tensors: k_ingest_arrays + the same load-time passes
    update (whole scene)    Scene.update_from_tensors(0, all members): ingest + cov3D + alpha cuts (+ the spatial copy from 4 M on)
    update (1 % range)      the same for n / 100 Gaussians in the middle of the scene

Each is warmed once, then the median of --repeats wall times is taken (every call returns synchronised), all in one process.
k_ingest_arrays itself is timed with events on the stream, as an update of positions + SH -- the members nothing is derived
from, on a scene without a spatial copy, so that the kernel is all the stream runs: 51 of a Gaussian's 59 floats, read once
and written once.

    python tools/device_ingest_rate.py [--gaussians 1000000 6000000] [--repeats 10] [--out profiles/rNN_device_ingest.txt]
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
args = ap.parse_args()

import torch  # noqa: E402

pkg = entry.load_package()


def wall_ms(fn):
    fn()  # warm
    ms = []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ms)


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


lines = [f"# python tools/device_ingest_rate.py --gaussians {' '.join(map(str, args.gaussians))} --repeats {args.repeats}   "
         f"({torch.cuda.get_device_name(0)}; S(n) scenes; median of {args.repeats} after one warm call; wall time of calls that return synchronised)",
         "%-10s %-22s %12s %14s" % ("gaussians", "path", "median_ms", "Gaussians/s")]
ok = True
for n in args.gaussians:
    rec = pkg.synth.synth_records(n, seed=0, kind="S")
    host = dict(means=rec[:, 0:3], log_scales=rec[:, 55:58], quats=rec[:, 58:62], opacity_logits=rec[:, 54], sh_dc=rec[:, 6:9],
                sh_rest=rec[:, 9:54].reshape(n, 3, 15).transpose(0, 2, 1))
    dev = {k: torch.from_numpy(v.copy()).cuda().contiguous() for k, v in host.items()}
    torch.cuda.synchronize()
    keep = []

    def from_records():
        keep[:] = [pkg.Scene.from_records(rec)]

    def from_tensors():
        keep[:] = [pkg.Scene.from_tensors(**dev)]

    t_rec = wall_ms(from_records)
    t_ten = wall_ms(from_tensors)
    scene = keep[0]
    t_all = wall_ms(lambda: scene.update_from_tensors(0, **dev))
    m, first = max(1, n // 100), n // 2
    part = {k: v[first:first + m] for k, v in dev.items()}
    t_part = wall_ms(lambda: scene.update_from_tensors(first, **part))
    keep.clear()
    del scene
    for name, ms, count in (("from_records", t_rec, n), ("from_tensors", t_ten, n), ("update (whole scene)", t_all, n), ("update (1 % range)", t_part, m)):
        lines.append("%-10d %-22s %12.3f %14.4g" % (n, name, ms, count / (ms * 1e-3)))
    lines.append(f"#   from_tensors / from_records = {t_ten / t_rec:.4f}")
    ok = ok and t_ten <= t_rec
    # the kernel alone
    old = os.environ.get("GS_SPATIAL_MIN")
    os.environ["GS_SPATIAL_MIN"] = str(1 << 40)
    flat = pkg.Scene.from_tensors(**dev)
    if old is None:
        del os.environ["GS_SPATIAL_MIN"]
    else:
        os.environ["GS_SPATIAL_MIN"] = old
    plain = {k: dev[k] for k in ("means", "sh_dc", "sh_rest")}
    t_k = event_ms(lambda: flat.update_from_tensors(0, **plain))
    lines.append(f"#   k_ingest_arrays (means + sh_dc + sh_rest: 51 floats in, 51 out per Gaussian = {n * 408 / 1e6:.0f} MB), events on the stream: "
                 f"{t_k:.3f} ms = {n * 408 / (t_k * 1e-3) / 1e9:.0f} GB/s of algorithmic bytes")
    del flat, dev, part, plain
    torch.cuda.empty_cache()
lines.append("# condition -- from_tensors not slower than from_records on the same data: " + ("holds" if ok else "FAILS"))
text = "\n".join(lines) + "\n"
print(text, end="")
if args.out:
    with open(args.out, "w") as f:
        f.write(text)
sys.exit(0 if ok else 1)
