#!/usr/bin/env python3
"""What the first step of a trainer costs on the device: the mean squared distance to the k nearest neighbours of every point of a
cloud (gs_knn_dist2: gs_knn.hip), next to what it replaces on the same device.  Per cloud, from one run:

    gs_knn_dist2, mean_dist2 only        the C call on preallocated outputs and scratch: seventeen launches and the synchronisation
    pkg.knn_dist2                        the same with the wrapper's finite check and its allocations
    pkg.init_from_points                 the six tensors of the model
    replaced: chunked cdist + topk       float32 torch on the same device: squared distances of a chunk of queries against all
                                         points by broadcasting (x - y)^2 summed, the row's own index masked out, topk(k, smallest),
                                         the mean -- the same quantity within tests/knn_reference.py's rounding bound, which the
                                         run checks on a sample.  --torch-limit bounds the cloud it is run on (it is quadratic);
                                         above it, it is timed on that many QUERIES against all points and scaled, and says so.

A call is timed between two events on torch's current stream (the calls return synchronised, so a span is the launches, the
kernels and the host's part).  One warm call each, then --repeats rounds, each timing every item once in turn; median and minimum.
The share of box pairs visited is box_visits.sum() / boxes^2.  The kernels one by one are not timed here (the C entry is one
call): a rocprofv3 kernel trace of this script gives them.

    python tools/knn_init_rate.py [--points 1000000] [--scenes S T] [--k 3] [--repeats 9] [--torch-limit 65536] [--out FILE]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--points", type=int, nargs="+", default=[1_000_000])
ap.add_argument("--scenes", nargs="+", default=["S", "T"])
ap.add_argument("--k", type=int, default=3)
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--torch-limit", type=int, default=65_536)
ap.add_argument("--torch-repeats", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import knn_reference as kr  # noqa: E402

pkg = entry.load_package()
b, L = pkg.binding, pkg.binding.lib()
k = args.k


def timed(call):
    s = torch.cuda.current_stream()
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(s)
    call()
    z.record(s)
    z.synchronize()
    return a.elapsed_time(z)


def torch_knn(points, queries, chunk):
    """mean over the k smallest squared distances of queries [0, queries) against all points, the row's own index excluded."""
    out = torch.empty(queries, dtype=torch.float32, device="cuda")
    for c0 in range(0, queries, chunk):
        q = points[c0:min(c0 + chunk, queries)]
        d2 = torch.zeros((len(q), len(points)), dtype=torch.float32, device="cuda")
        for a in range(3):
            d = q[:, a, None] - points[None, :, a]
            d2 += d * d
        d2[torch.arange(len(q), device="cuda"), torch.arange(c0, c0 + len(q), device="cuda")] = float("inf")
        out[c0:c0 + len(q)] = torch.topk(d2, k, dim=1, largest=False).values.sum(dim=1) / k
    return out


lines = [f"# python tools/knn_init_rate.py --points {' '.join(map(str, args.points))} --scenes {' '.join(args.scenes)} --k {k} --repeats {args.repeats} "
         f"--torch-limit {args.torch_limit}   ({torch.cuda.get_device_name(0)}; GS_KNN_BOX = {b.KNN_BOX}; one warm call, then rounds, every item once per round)",
         "%-6s %9s %-50s %11s %11s" % ("scene", "points", "what", "median_ms", "min_ms")]
for n in args.points:
    for kind in args.scenes:
        xyz_host = np.ascontiguousarray(pkg.synth.synth_records(n, seed=0, kind=kind)[:, :3], np.float32)
        xyz = torch.as_tensor(xyz_host).cuda()
        L.gs_knn_scratch_bytes.restype, L.gs_knn_scratch_bytes.argtypes = C.c_uint64, [C.c_uint64]
        need = int(L.gs_knn_scratch_bytes(C.c_uint64(n)))
        scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
        mean = torch.empty(n, dtype=torch.float32, device="cuda")
        handle = C.c_void_p(torch.cuda.current_stream().cuda_stream or None)
        kept = {}

        def entry_only():
            b._check(L.gs_knn_dist2(C.c_void_p(xyz.data_ptr()), C.c_uint64(n), C.c_int(k), C.c_void_p(mean.data_ptr()), None, None,
                                    C.c_void_p(scratch.data_ptr()), C.c_uint64(need), 0, handle))

        def wrapper():
            kept["w"] = pkg.knn_dist2(xyz, k=k)

        def model():
            kept["m"] = pkg.init_from_points(xyz, k=k)

        queries = min(n, args.torch_limit)
        # a chunk's distance matrix stays near 1 GiB
        chunk = max(1, min(queries, (1 << 28) // n))

        def replaced():
            kept["t"] = torch_knn(xyz, queries, chunk)

        items = [("gs_knn_dist2, mean_dist2 only", entry_only, args.repeats), ("pkg.knn_dist2", wrapper, args.repeats),
                 ("pkg.init_from_points", model, args.repeats),
                 (f"replaced: chunked cdist + topk, {queries} queries", replaced, args.torch_repeats)]
        for _, call, _ in items:
            call()
        torch.cuda.synchronize()
        ms = {what: [] for what, _, _ in items}
        for r in range(args.repeats):
            for what, call, reps in items:
                if r < reps:
                    ms[what].append(timed(call))
        med = {what: statistics.median(v) for what, v in ms.items()}
        for what, _, _ in items:
            lines.append("%-6s %9d %-50s %11.3f %11.3f" % (kind, n, what, med[what], min(ms[what])))
        visits = pkg.knn_dist2(xyz, k=k, mean=False, visits=True)["box_visits"]
        boxes = len(visits)
        # the two agree within the counted roundings (both sides carry them: twice the bound), on the queries torch answered
        got, old = kept["w"]["mean_dist2"][:queries].double(), kept["t"].double()
        agree = bool(((got - old).abs() <= 2.0 * kr.rounding_bound(k) * got).all())
        # ... and a sample of the kernels' values are the restatement's bits
        rows = np.random.default_rng(1).choice(n, 256, replace=False)
        want, _ = kr.knn_rows(xyz_host, rows, k)
        exact = bool(np.array_equal(kept["w"]["mean_dist2"].cpu().numpy()[rows].view(np.uint32), want.view(np.uint32)))
        scaled = med[items[3][0]] * n / queries
        lines.append(f"#      {kind}({n}): box pairs visited {int(visits.sum())} of {boxes}^2 = {float(visits.sum()) / boxes ** 2:.5f} "
                     f"(mean {float(visits.float().mean()):.1f}, max {int(visits.max())} boxes per query box); scratch {need / 1e6:.1f} MB; "
                     f"torch formulation {'as timed' if queries == n else f'scaled from {queries} queries to {n}'}: {scaled:.1f} ms = "
                     f"{scaled / med[items[0][0]]:.1f} x gs_knn_dist2; agrees with torch within the rounding bound: {agree}; 256 sampled rows "
                     f"equal the restatement's bits: {exact}")
        del xyz, scratch, mean, kept, visits
        torch.cuda.empty_cache()
lines.append("# not measured here: the kernels one by one (see the kernel trace), GS_KNN_BOX = 128 and 512, k other than the one given")
text = "\n".join(lines) + "\n"
print(text, end="")
if args.out:
    with open(args.out, "w") as f:
        f.write(text)
