"""Blend-kernel work statistics from the instrumented build (libgs3d_hip_stats.so, -DGS_BLEND_STATS: `make -C
3dgs.cpp_amd/csrc stats`), per workload, as JSON -- the figures bench.py's `roofline.flops_view` is computed from.

    GS3D_HIP_LIB=3dgs.cpp_amd/libgs3d_hip_stats.so python tools/blend_stats.py [--out gpurun_out/blend_work.json] B C T E

walked_pairs        (pixel, entry) pairs the REFERENCE's loop walks: every pixel, its tile's list up to and including the
                    entry it breaks at (render.comp:60-85) -- a property of the workload, not of this implementation;
                    SURVEY 8d prices the blend at 22 flop each
contributing_pairs  of those, the ones with alpha >= 1/255 that are accumulated
wave_pairs          (entry, 8x8-pixel wave) pairs this implementation evaluates after its exact quadrant culling
lanes_in_exp        lanes that reach exp() in them

The counters live in the compiler's form of the pair loop, which the guarded default (exp mode 3) does not run, so the frames are
rendered in exp mode 2.  That counts the same work: every counter is a function of the keep and break decisions alone, and modes 2
and 3 take the same decisions (the alpha cut is decided on `power`, the break is the reference's or resolved
exactly).  A quadrant that mode 3 abandons and walks a second time is that mode's cost, not the workload's, and is not counted.
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

WORKLOADS = {"A": (10_000, 256, 256, "A"), "B": (1_000_000, 1920, 1080, "S"), "C": (6_000_000, 1920, 1080, "S"),
             "T": (6_000_000, 1920, 1080, "T"), "E": (6_000_000, 3840, 2160, "S")}


def workload_key(n, w, h, kind):
    return f"{kind}({n})@{w}x{h}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("names", nargs="*", default=["B"])
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    pkg = entry.load_package()
    L = pkg.binding.lib()
    if not hasattr(L, "gs_debug_blend_stats"):
        raise SystemExit("needs the instrumented build: GS3D_HIP_LIB=3dgs.cpp_amd/libgs3d_hip_stats.so")
    result = {}
    for name in args.names:
        n, w, h, kind = WORKLOADS[name]
        rec = pkg.synth.synth_records(n, seed=0, kind=kind)
        scene = pkg.Scene.from_records(rec)
        del rec
        rend = pkg.Renderer(scene)
        rend.set_exp_mode(2)  # (the counted loop: see above)
        u = pkg.camera_uniforms(pkg.make_camera(), w, h)
        out = (ctypes.c_ulonglong * 12)()
        for _ in range(3):  # the first frames may be re-run at a larger sort level: keep the last, clean one
            rend.render_host(u, want_rgba=True)
            L.gs_debug_blend_stats(out, 1)
        st = rend.stats()
        v = [int(x) for x in out]
        # walked_pairs is defined over the REFERENCE's lists.  On a frame whose lists are culled (gs_set_tile_cull) the instrumented
        # loop walks the shorter lists and would count fewer of them: that figure, and contributing_pairs beside it, come from one
        # more frame with the cull off; everything else is this implementation's work on the lists it walks.
        listed = None
        if hasattr(L, "gs_set_tile_cull") and rend.tile_cull()[1]:
            listed = rend.listed_instances()
            rend.set_tile_cull(False)
            rend.render_host(u, want_rgba=True)
            L.gs_debug_blend_stats(out, 1)
            v_ref = [int(x) for x in out]
            assert v_ref[8] == v[8], "the cull changed the contributing pairs"
            v[7] = v_ref[7]
        result[workload_key(n, w, h, kind)] = {
            "gaussians": int(st.num_gaussians), "visible": int(st.num_visible), "instances": int(st.num_instances),
            "walked_pairs": v[7], "contributing_pairs": v[8], "wave_pairs": v[2], "wave_pairs_reaching_exp": v[4],
            "lanes_alive_in_wave_pairs": v[3], "lanes_in_exp": v[5], "wave_chunks": v[0], "entries_staged": v[6],
            "flop_per_walked_pair": 22}
        if listed is not None:
            result[workload_key(n, w, h, kind)]["instances_listed"] = int(listed)
        print(name, json.dumps(result[workload_key(n, w, h, kind)]), flush=True)
        rend.close()
        scene.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
