"""The one-pass level 1 (gs_set_level1_fused; gs_kernels.h: L1Fused): k_preprocess files the level-1 candidate records itself, one
device atomic per (workgroup, bin it touches), and k_l1_hist / k_l1_scan / k_l1_scatter_any_order are not launched.  It may change
nothing: on the same frame the two paths must agree with NO tolerance -- the taps array for array (tiles, depth, aabb, sorted_tile,
sorted_gid, ranges), the exp-mode-2 image and the default (mode 3) image bit for bit, V / D / E1 / the fullest bin -- and with the
oracle.  Within a bin the candidates arrive in an order that differs from run to run; level 2 orders them by (depth bits, id).

No reference counterpart (the reference sorts every instance globally): the oracle's lists are the yardstick for both paths.
Every test runs under both depth-order settings of the suite (conftest.py): on the global path the one-pass level 1 never engages,
which is then what the test checks."""
import numpy as np
import pytest

import limit_scenes as ls
from helpers import compare_stages, oracle_frame

pytestmark = pytest.mark.gpu

TAPS = ("tiles", "depth", "aabb", "sorted_tile", "sorted_gid")


class _HipBuffers:
    """Device allocations through the HIP runtime the library itself uses (as tests/test_gpu_parity.py)."""

    def __init__(self):
        import ctypes
        self.C = ctypes
        self.hip = ctypes.CDLL("libamdhip64.so")
        self.ptrs = []

    def alloc(self, nbytes):
        p = self.C.c_void_p()
        assert self.hip.hipMalloc(self.C.byref(p), self.C.c_size_t(nbytes)) == 0
        self.ptrs.append(p)
        return p.value

    def download(self, ptr, shape, dtype):
        out = np.zeros(shape, dtype)
        assert self.hip.hipMemcpy(out.ctypes.data_as(self.C.c_void_p), self.C.c_void_p(ptr), self.C.c_size_t(out.nbytes), 2) == 0
        return out

    def close(self):
        for p in self.ptrs:
            self.hip.hipFree(p)


def snapshot(rend, u, images=True):
    """One frame: the exp-mode-2 image, whether it took the one-pass level 1, its counts, its taps, and the default blend's image."""
    rend.set_exp_mode(2)
    img, _ = rend.render_host(u)
    fused = rend.level1_fused()
    st = rend.stats()
    out = {"image": img, "fused": fused, "retries": st.retries,
           "counts": (st.num_visible, st.num_instances, st.num_bin_entries, st.max_bin_entries)}
    for k in TAPS:
        out[k] = rend.stage(k).copy()
    out["ranges"] = rend.stage("ranges", u).copy()
    if images:
        rend.set_exp_mode(3)
        out["image3"], _ = rend.render_host(u)
        assert rend.level1_fused() == fused
        rend.set_exp_mode(2)
    return out


def assert_same_frame(a, b):
    assert a["counts"] == b["counts"]
    vis = a["tiles"] != 0
    np.testing.assert_array_equal(a["tiles"], b["tiles"])
    for k in ("depth", "aabb"):  # (a culled Gaussian's depth and box are whatever an earlier frame left: compare_stages masks them too)
        np.testing.assert_array_equal(a[k].reshape(len(vis), -1)[vis].view(np.uint8), b[k].reshape(len(vis), -1)[vis].view(np.uint8))
    for k in ("sorted_tile", "sorted_gid", "ranges"):
        np.testing.assert_array_equal(a[k], b[k])
    for k in ("image", "image3"):
        if k in a and k in b:
            np.testing.assert_array_equal(a[k].view(np.uint32), b[k].view(np.uint32))


def both_paths(pkg, oracle, rec, w, h, sort_path, camera=None, on=1):
    """The frame on the three kernels (switch 0), then with the switch at `on`, on one renderer; both against each other and
    the second against the oracle.  Returns (scene, renderer, uniforms, the two snapshots)."""
    verts, u_ref, ref = oracle_frame(oracle, rec, w, h, camera)
    scene = pkg.Scene.from_records(rec, device=0)
    rend = pkg.Renderer(scene)
    u = pkg.camera_uniforms(camera if camera is not None else pkg.make_camera(), w, h)
    assert u.tobytes() == u_ref.tobytes()
    rend.set_level1_fused(0)
    three = snapshot(rend, u)
    assert not three["fused"]
    rend.set_level1_fused(on)
    one = snapshot(rend, u)
    assert one["fused"] == (sort_path != "1"), "the one-pass level 1 engages on the bin-local path, and only there"
    assert_same_frame(three, one)
    compare_stages(pkg, rend, u, ref)  # (the last frame: the one-pass path's)
    np.testing.assert_array_equal(one["image"].view(np.uint32), ref["image"].view(np.uint32))
    again = snapshot(rend, u, images=False)  # the same buffers once more: the frame's last kernel zeroed the cursors
    assert_same_frame(one, again)
    return scene, rend, u, three, one


def wide_splats(rec, first, count, log_scale):
    """`count` splats of scale exp(log_scale) next to each other in front of the default camera: neighbours in the order the
    kernels read the scene in (lanes of one wave), each covering the screen or most of it."""
    rec[first:first + count, 0:3] = np.array([0.0, 0.0, -4.0], np.float32) + np.linspace(0, 0.01, count)[:, None].astype(np.float32)
    rec[first:first + count, 55:58] = log_scale


def bins_touched(aabb, ids, shift):
    """bins in the tile boxes of Gaussians `ids` (the aabb tap: x0 y0 x1 y1 in tiles, upper bounds exclusive)"""
    b = aabb.reshape(-1, 4)[ids].astype(np.int64)
    return (((b[:, 2] - 1) >> shift) + 1 - (b[:, 0] >> shift)) * (((b[:, 3] - 1) >> shift) + 1 - (b[:, 1] >> shift))


# (name, Gaussians, kind, width, height, GS_BIN_SHIFT or None, spatial copy, what the scene gets)
CASES = [
    ("one_bin", 2000, "A", 64, 64, None, True, None),                     # 4 x 4 tiles: a single bin, every workgroup reserves in it
    ("screen_filler_and_big_boxes", 30000, "A", 640, 360, None, True, "big"),
    ("bins_of_4x4_tiles", 30011, "A", 640, 360, 2, True, "big"),          # 10 x 6 bins; a ragged last wave (30011 = 64 * 468 + 59)
    ("culled_workgroup", 20000, "A", 320, 200, None, True, "culled"),     # a workgroup with no visible lane among full ones
    ("over_64_bins_per_workgroup", 20000, "T", 1024, 1024, 2, False, "big"),  # 16 x 16 bins, scene-id order: a workgroup touches most of them
    ("padded_grid_of_32", 6000, "A", 1104, 80, 2, True, "big"),           # 18 x 2 bins: the 32-wide grid (the kernels' 1024-bin tables)
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_paths_agree(pkg, oracle, gpu, monkeypatch, _sort_path, case):
    name, n, kind, w, h, shift, spatial, extra = case
    monkeypatch.setenv("GS_SPATIAL_MIN", "0" if spatial else "1000000000")
    if shift is not None:
        monkeypatch.setenv("GS_BIN_SHIFT", str(shift))
    rec = pkg.synth.synth_records(n, seed=n, kind=kind)
    if extra == "big":
        wide_splats(rec, 0, 1, 1.5)     # one splat that fills the screen: it touches every bin
        wide_splats(rec, 64, 9, 1.0)    # several lanes of one wave with boxes of more than kL1BigBox = 12 bins
    if extra == "culled":
        rec[4000:5000, 0] += 1000.0     # 1000 neighbours far outside the frustum: whole workgroups of culled lanes
    # spatial copy: by rule (-1); scene-id order: the rule refuses (no spatial copy), the switch forces it
    scene, rend, u, three, one = both_paths(pkg, oracle, rec, w, h, _sort_path, on=-1 if spatial else 1)
    if extra == "big":
        s_ = shift or 3
        all_bins = (((w + 15) // 16 - 1 >> s_) + 1) * (((h + 15) // 16 - 1 >> s_) + 1)
        assert bins_touched(one["aabb"], [0], s_)[0] == all_bins, "the screen-filling splat does not touch every bin"
        assert (bins_touched(one["aabb"], np.arange(64, 73), s_) > 12).all(), "the wave's wide splats stay within kL1BigBox bins"
    print(f"{name}: V D E1 maxbin {one['counts']} one-pass {one['fused']}")


def test_no_visible_gaussian(pkg, oracle, gpu, monkeypatch, _sort_path):
    monkeypatch.setenv("GS_SPATIAL_MIN", "0")
    rec = pkg.synth.synth_records(3000, seed=2, kind="A")
    rec[:, 2] = np.abs(rec[:, 2])  # every Gaussian behind the camera
    scene, rend, u, three, one = both_paths(pkg, oracle, rec, 200, 120, _sort_path, on=-1)
    assert one["counts"] == (0, 0, 0, 0)
    assert not one["image"][..., :3].any()


def test_fall_backs(pkg, oracle, gpu, monkeypatch, _sort_path):
    """By rule the path needs the scene's spatial copy and a scene below the dense-list threshold; the getter says what ran."""
    rec = pkg.synth.synth_records(8000, seed=8, kind="A")
    w, h = 320, 200
    verts, u_ref, ref = oracle_frame(oracle, rec, w, h)
    u = pkg.camera_uniforms(pkg.make_camera(), w, h)
    for env, mode, want in [({"GS_SPATIAL_MIN": "1000000000"}, -1, False),                         # no spatial copy
                            ({"GS_SPATIAL_MIN": "0"}, -1, True),
                            ({"GS_SPATIAL_MIN": "0", "GS_L1_DENSE_MIN": "8000"}, -1, False),       # a scene AT dense_min
                            ({"GS_SPATIAL_MIN": "0", "GS_L1_DENSE_MIN": "8000"}, 1, False),        # ... which the switch does not override
                            ({"GS_SPATIAL_MIN": "0", "GS_L1_DENSE_MIN": "8001"}, -1, True),
                            ({"GS_SPATIAL_MIN": "0", "GS_L1_FUSED": "0"}, None, False)]:           # the environment's switch
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            scene = pkg.Scene.from_records(rec, device=0)
            rend = pkg.Renderer(scene)
        if mode is not None:
            rend.set_level1_fused(mode)
        img, _ = rend.render_host(u)
        assert rend.level1_fused() == (want and _sort_path != "1"), (env, mode)
        compare_stages(pkg, rend, u, ref)
        np.testing.assert_array_equal(img.view(np.uint32), ref["image"].view(np.uint32))
        rend.close()
        scene.close()


def _fullest_bin(pkg, rec, u):
    """(fullest bin, E1) of the frame, from a renderer that runs the three kernels."""
    scene = pkg.Scene.from_records(rec, device=0)
    rend = pkg.Renderer(scene)
    rend.set_level1_fused(0)
    rend.render_host(u)
    st = rend.stats()
    rend.close()
    scene.close()
    return st.max_bin_entries, st.num_bin_entries


def test_region_edge(pkg, oracle, gpu, monkeypatch, _sort_path):
    """Bin b owns cap = candidate capacity / bins records.  A fullest bin of exactly cap stays on the one-pass path; with cap one
    short the frame overflows, is re-run once on the three kernels, which then stay for the hold (32 frames) -- after which the
    rule decides again: cap is below 5/4 of the fullest bin, the candidate buffer grows (within 4 x its first size) and the path
    re-engages.  Every frame equal to the oracle's."""
    monkeypatch.setenv("GS_SPATIAL_MIN", "0")
    rec = pkg.synth.synth_records(8000, seed=21, kind="A")  # (a fullest bin below 4096: no re-run for the depth-order level's sake)
    w, h, bins = 640, 360, 5 * 3
    verts, u_ref, ref = oracle_frame(oracle, rec, w, h)
    u = pkg.camera_uniforms(pkg.make_camera(), w, h)
    fullest, e1 = _fullest_bin(pkg, rec, u)
    assert fullest * bins >= max(e1, 256) and fullest < 4096
    for cand, overflows in [(fullest * bins, False), (fullest * bins + bins - 1, False), (fullest * bins - 1, True)]:
        monkeypatch.setenv("GS_INITIAL_CAND_CAPACITY", str(cand))
        scene = pkg.Scene.from_records(rec, device=0)
        rend = pkg.Renderer(scene)
        img, _ = rend.render_host(u)
        st = rend.stats()
        compare_stages(pkg, rend, u, ref)
        np.testing.assert_array_equal(img.view(np.uint32), ref["image"].view(np.uint32))
        assert (st.num_bin_entries, st.max_bin_entries) == (e1, fullest)
        if _sort_path == "1":
            assert not rend.level1_fused() and st.retries == 0
            continue
        if not overflows:
            assert rend.level1_fused() and st.retries == 0, cand
            continue
        assert not rend.level1_fused() and st.retries == 1, "one re-run, on the three kernels"
        for k in range(31):  # the hold: 32 frames retire on the three kernels (the re-run was the first)
            img, _ = rend.render_host(u)
            assert not rend.level1_fused(), k
        img, _ = rend.render_host(u)  # the rule again: cap < 5/4 of the fullest bin -> the buffer grows by what the rule needs
        assert rend.level1_fused()
        st = rend.stats()
        assert st.retries == 1
        compare_stages(pkg, rend, u, ref)
        np.testing.assert_array_equal(img.view(np.uint32), ref["image"].view(np.uint32))


def _exact_frame(pkg, rend, u, ref):
    """One frame, equal to the oracle's: (whether it took the one-pass level 1, its stats)."""
    img, _ = rend.render_host(u)
    fused = rend.level1_fused()
    st = rend.stats()
    compare_stages(pkg, rend, u, ref)
    np.testing.assert_array_equal(img.view(np.uint32), ref["image"].view(np.uint32))
    return fused, st


@pytest.mark.parametrize("extra", [False, True], ids=["E1_is_8V", "E1_is_8V_plus_1"])
def test_wide_splat_exit(pkg, oracle, gpu, monkeypatch, _sort_path, extra):
    """L1FusedPolicy's wide-splat exit, E1 > 8 V (limit_scenes.wide_ratio: every visible Gaussian in 4 x 2 bins, and one of them in
    3 x 3).  By rule the first frame of either scene is a one-pass frame -- no frame has retired, the frame tells -- and what it
    counted decides the second: at E1 = 8 V the path stays, at 8 V + 1 the three kernels run.  The switch overrides the ratio, and
    the rule, asked again, leaves again.  E1 and V feed the rule, so both are asserted, whichever form of level 1 counted them."""
    sc = ls.wide_ratio(extra)
    for k, v in sc.env.items():
        monkeypatch.setenv(k, v)
    verts, u_ref, ref = oracle_frame(oracle, sc.records, sc.width, sc.height)
    got = ls.measure(sc, ref)
    for key, want in sc.expect.items():
        assert got[key] == want, f"{sc.name} missed its edge ({sc.pins}): {key} is {got[key]}, not {want}"
    e1, v = sc.expect["bin_entries"][2], sc.expect["visible"]
    assert (e1 > ls.WIDE_RATIO * v) == extra and e1 - ls.WIDE_RATIO * v == (1 if extra else 0)
    scene = pkg.Scene.from_records(sc.records, device=0)
    rend = pkg.Renderer(scene)
    u = pkg.camera_uniforms(pkg.make_camera(), sc.width, sc.height)
    assert u.tobytes() == u_ref.tobytes()
    auto = _sort_path != "1"   # (on the global path the one-pass level 1 never engages)
    try:
        for mode, want in [(None, auto), (None, auto and not extra), (1, auto), (1, auto), (-1, auto and not extra)]:
            if mode is not None:
                rend.set_level1_fused(mode)
            fused, st = _exact_frame(pkg, rend, u, ref)
            assert fused == want, f"{sc.name}: mode {mode}, one-pass {fused}"
            assert (st.num_bin_entries, st.num_visible, st.max_bin_entries, st.retries) == (e1, v, sc.expect["fullest_bin"][2], 0)
    finally:
        rend.close()
        scene.close()


def _counts(pkg, rec, u):
    """(fullest bin, E1, D) of the frame, from a renderer that runs the three kernels."""
    scene = pkg.Scene.from_records(rec, device=0)
    rend = pkg.Renderer(scene)
    rend.set_level1_fused(0)
    rend.render_host(u)
    st = rend.stats()
    assert st.retries == 0
    rend.close()
    scene.close()
    return st.max_bin_entries, st.num_bin_entries, st.num_instances


@pytest.mark.parametrize("edge", ["lists_hold_E1", "lists_hold_D_minus_1"])
def test_list_buffer_overflow_on_a_one_pass_frame(pkg, oracle, gpu, monkeypatch, _sort_path, edge):
    """A frame of one bin (64 x 64 px) whose splats cover several tiles each: D well above E1.  The per-tile lists start at the
    least (E1: GS_INITIAL_CAPACITY caps the candidate buffer too, so the bin's region is then full to its last record) and the most
    (D - 1) with which level 2 overflows them while the bin's region holds: exactly one re-run, no hold -- the re-run and the next
    frame are one-pass frames -- and every frame equal to the oracle's."""
    monkeypatch.setenv("GS_SPATIAL_MIN", "0")
    rec = pkg.synth.synth_records(2000, seed=2000, kind="A")
    w = h = 64
    verts, u_ref, ref = oracle_frame(oracle, rec, w, h)
    u = pkg.camera_uniforms(pkg.make_camera(), w, h)
    fullest, e1, d = _counts(pkg, rec, u)
    assert fullest == e1 >= 256 and d >= 2 * e1, f"one bin, D well above E1: fullest bin {fullest}, E1 {e1}, D {d}"
    lists = e1 if edge == "lists_hold_E1" else d - 1
    assert ls.region_cap(ls.candidate_capacity(len(rec), {"GS_INITIAL_CAPACITY": str(lists)}), ls.screen_bins(w, h, 3)) >= fullest
    monkeypatch.setenv("GS_INITIAL_CAPACITY", str(lists))
    scene = pkg.Scene.from_records(rec, device=0)
    rend = pkg.Renderer(scene)
    try:
        for frame in range(2):
            fused, st = _exact_frame(pkg, rend, u, ref)
            assert (st.max_bin_entries, st.num_bin_entries, st.num_instances) == (fullest, e1, d)
            if _sort_path == "1":   # the global path's lists overflow too; the one-pass level 1 never engages there
                assert not fused and st.retries >= 1
                continue
            assert st.retries == 1, f"frame {frame}: {st.retries} re-runs"
            assert fused, f"frame {frame}: the three kernels ran"
    finally:
        rend.close()
        scene.close()


def test_three_frames_in_flight_two_poses(pkg, oracle, gpu, monkeypatch, _sort_path):
    """The camera alternates between two poses whose fullest bins differ by more than the rule's 5/4 margin, with a candidate
    buffer whose regions hold the one and not the other: frames overflow, are re-run, the path is held and re-engages while three
    frames are in flight.  Every frame equals the same pose rendered alone on the three kernels."""
    monkeypatch.setenv("GS_SPATIAL_MIN", "0")
    rec = pkg.synth.synth_records(3500, seed=33, kind="A")
    w, h, bins = 640, 360, 5 * 3
    # the default pose, and one from 8 units further back: the whole scene inside the centre bin
    poses = [pkg.camera_uniforms(pkg.make_camera(), w, h), pkg.camera_uniforms(pkg.make_camera(position=(0.0, 0.0, 8.0)), w, h)]
    full = [_fullest_bin(pkg, rec, p)[0] for p in poses]
    cap = (5 * full[0] + 3) // 4
    assert cap < full[1] < 4096, f"the poses' fullest bins {full} do not differ by more than 5/4 (or the wide one needs another depth-order level)"
    # the serial references: each pose alone, three kernels
    scene = pkg.Scene.from_records(rec, device=0)
    plain = pkg.Renderer(scene)
    plain.set_level1_fused(0)
    serial = [plain.render_host(p)[0] for p in poses]
    for p, s_img in zip(poses, serial):
        ref = oracle.stages(oracle.activate_records(rec), p.view(oracle.UNIFORMS_DT))["image"]
        np.testing.assert_array_equal(s_img.view(np.uint32), ref.view(np.uint32))
    monkeypatch.setenv("GS_INITIAL_CAND_CAPACITY", str(cap * bins))
    rend = pkg.Renderer(scene)
    rend.set_frames_in_flight(3)
    dev = _HipBuffers()
    count = 12
    outs = [dev.alloc(w * h * 16) for _ in range(count)]
    took = []
    for k in range(count):
        rend.render(poses[k % 2], outs[k], 0)
        took.append(rend.level1_fused())
    rend.synchronize()
    for k in range(count):
        np.testing.assert_array_equal(dev.download(outs[k], (h, w, 4), np.float32).view(np.uint32), serial[k % 2].view(np.uint32), err_msg=f"frame {k}")
    dev.close()
    st = rend.stats()
    if _sort_path == "1":
        assert not any(took) and st.retries == 0
    else:
        assert took[0], "no frame has retired yet: the rule engages"
        assert st.retries >= 1, "the wide pose ran over its bin regions at least once"
        assert False in took, "... after which the path is held"
    print(f"fullest bins {full}, cap {cap}, one-pass per enqueue {took}, retries {st.retries}")


def test_both_switch_positions_under_graph_replay(pkg, oracle, gpu, monkeypatch, _sort_path):
    monkeypatch.setenv("GS_SPATIAL_MIN", "0")
    rec = pkg.synth.synth_records(12000, seed=5, kind="A")
    w, h = 400, 240
    verts, u_ref, ref = oracle_frame(oracle, rec, w, h)
    u = pkg.camera_uniforms(pkg.make_camera(), w, h)
    scene = pkg.Scene.from_records(rec, device=0)
    rend = pkg.Renderer(scene)
    rend.set_graph_mode(True)
    for mode in (0, 1, 0, -1):
        rend.set_level1_fused(mode)
        for _ in range(3):  # capture, then replays
            img, _ = rend.render_host(u)
            assert rend.level1_fused() == (mode != 0 and _sort_path != "1")
            np.testing.assert_array_equal(img.view(np.uint32), ref["image"].view(np.uint32))
        compare_stages(pkg, rend, u, ref)
