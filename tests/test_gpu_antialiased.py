"""The antialiased mode (gs_set_antialiased) on the device.

The mode scales each splat's opacity by comp = sqrt(det(cov2D) / det(cov2D + 0.3 I)) in k_preprocess and takes the scaled
opacity's alpha cut per frame; nothing else of the frame changes.  Hence the exact contract checked here: the frame of scene S
with the mode on equals, bit for bit, the ordinary frame of the scene S' whose opacities are the scaled ones (read back from the
record tap) -- and that ordinary frame is the reference's own (the oracle on S').  The lists do not depend on the mode, the
factor agrees with float64 within a derived bound, the per-frame alpha cut is the load-time one for every binary32 opacity, and
switching the mode (queued frames, graph replay, GS_ANTIALIASED) gives each frame its own setting's bits."""
import os

import numpy as np
import pytest

import aa_reference as aa
import np_reference as npr
from helpers import assert_guarded_close, assert_images_identical, compare_stages

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RECORD_TAPS = ("radius", "conic_opacity", "uv_rg", "b", "alpha_cut")


def _sub_pixel_and_needles(pkg, n=20000, seed=41):
    """Mostly sub-pixel splats, a third of them needles (long axis 0.2 .. 1 world units, sub-pixel across)."""
    rec = pkg.synth.synth_records(n, seed=seed, kind="A")
    rng = np.random.default_rng(seed)
    rec[:, 55:58] = rng.uniform(-8.0, -4.5, (n, 3))
    k = n // 3
    rec[:k, 55] = rng.uniform(-1.5, 0.0, k)
    rec[:k, 58:62] = rng.normal(size=(k, 4))
    rec[:, 54] = rng.uniform(-2.0, 4.0, n)
    return rec


def _slab_scene(pkg):
    import hashlib
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_slabs", os.path.join(GOLDEN, "make_golden_slabs.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    g = np.load(os.path.join(GOLDEN, "scene_slabs24k.npz"))
    rec = mod.slab_scene_records(pkg)
    assert hashlib.sha256(rec.tobytes()).hexdigest() == str(g["records_sha256"])
    w, h = int(g["uniforms"]["width"][0]), int(g["uniforms"]["height"][0])
    u = pkg.camera_uniforms(g["camera"].view(pkg.binding.CAMERA_DT), w, h)
    assert u.tobytes() == g["uniforms"].tobytes()
    return rec, u


def _taps(rend, u):
    """Every stage tap of the last frame; the per-Gaussian record fields of the visible Gaussians only (the others are whatever
    the buffer held)."""
    tiles = rend.stage("tiles")
    vis = tiles != 0
    out = dict(tiles=tiles, depth=rend.stage("depth")[vis], aabb=rend.stage("aabb").reshape(-1, 4)[vis])
    for name in RECORD_TAPS:
        t = rend.stage(name)
        out[name] = (t.reshape(len(tiles), -1)[vis] if t.size != len(tiles) else t[vis]).view(np.uint32)
    for name in ("sorted_tile", "sorted_gid"):
        out[name] = rend.stage(name)
    out["ranges"] = rend.stage("ranges", u)
    if rend.stats().sort_path == 1:
        out["depth_order"] = rend.stage("depth_order")
    st = rend.stats()
    out["V"], out["D"] = np.array([st.num_visible]), np.array([st.num_instances])
    return out


def _assert_taps_equal(a, b, label, only=None):
    assert set(a) == set(b)
    for k in a if only is None else only:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{label}: tap {k}")


def _render_aa(pkg, verts, u, exp_mode):
    """S rendered with the mode on; returns (scene, renderer, rgba, bgra, taps, S' vertices)."""
    scene = pkg.Scene.from_vertices(verts, device=0)
    rend = pkg.Renderer(scene)
    rend.set_exp_mode(exp_mode)
    rend.set_antialiased(True)
    assert rend.antialiased
    img, bgra = rend.render_host(u, want_rgba=True, want_bgra=True)
    taps = _taps(rend, u)
    vis = taps["tiles"] != 0
    op = rend.stage("conic_opacity").reshape(-1, 4)[:, 3]
    prime = verts.copy()
    prime["scale_opacity"][vis, 3] = op[vis]  # vertex column 7: the opacity
    return scene, rend, img, bgra, taps, prime


def _scenes(pkg, oracle, which, monkeypatch):
    if which == "subpixel_needles":
        rec = _sub_pixel_and_needles(pkg)
        return oracle.activate_records(rec), pkg.camera_uniforms(pkg.make_camera(), 960, 540)
    if which == "slabs24k":
        rec, u = _slab_scene(pkg)
        return oracle.activate_records(rec), u
    monkeypatch.setenv("GS_L1_DENSE_MIN", "0")
    monkeypatch.setenv("GS_SPATIAL_MIN", "0")
    rec = _sub_pixel_and_needles(pkg, n=6000, seed=43)
    return oracle.activate_records(rec), pkg.camera_uniforms(pkg.make_camera(), 640, 360)


@pytest.mark.parametrize("exp_mode", [2, 3])
@pytest.mark.parametrize("which", ["subpixel_needles", "slabs24k", "dense_lists_morton"])
def test_antialiased_frame_is_the_plain_frame_of_the_compensated_scene(pkg, oracle, gpu, monkeypatch, which, exp_mode):
    """S with the mode on == S' (opacities replaced by the frame's opacity') with it off: RGBA, BGRA and every stage tap, alpha cut
    included, bit for bit.  S' is then pinned to the reference: in exp mode 2 its image is the oracle's on S' bit for bit and
    every stage tap matches the oracle's buffers; in mode 3 the guarded blend is within rounding noise of that image."""
    verts, u = _scenes(pkg, oracle, which, monkeypatch)
    scene, rend, img, bgra, taps, prime = _render_aa(pkg, verts, u, exp_mode)
    vis = taps["tiles"] != 0
    assert vis.sum() > 1000
    comp = prime["scale_opacity"][vis, 3].astype(np.float64) / verts["scale_opacity"][vis, 3]
    assert (comp < 1).mean() > 0.99, "the scene must exercise the factor"

    s2 = pkg.Scene.from_vertices(prime, device=0)
    r2 = pkg.Renderer(s2)
    r2.set_exp_mode(exp_mode)
    assert not r2.antialiased
    img2, bgra2 = r2.render_host(u, want_rgba=True, want_bgra=True)
    np.testing.assert_array_equal(img.view(np.uint32), img2.view(np.uint32))
    np.testing.assert_array_equal(bgra, bgra2)
    _assert_taps_equal(taps, _taps(r2, u), f"{which}, exp mode {exp_mode}")

    ref = oracle.stages(prime, u.view(oracle.UNIFORMS_DT))
    if exp_mode == 2:
        assert_images_identical(img, ref["image"], label=f"{which}: antialiased frame vs the oracle on S'")
        compare_stages(pkg, rend, u, ref)
        np.testing.assert_array_equal(taps["alpha_cut"], oracle.alpha_cut(prime["scale_opacity"][:, 3])[vis].view(np.uint32))
    else:
        assert_guarded_close(rend, u, ref["image"], label=f"{which}: antialiased, guarded blend vs the oracle on S'")
    for o in (rend, r2, scene, s2):
        o.close()


def test_lists_are_the_same_with_the_mode_on_and_off(pkg, oracle, gpu):
    """Opacity enters neither the cull, the radius, the box nor the depth order: lists, ranges, tiles, boxes, radii, conics and the
    counts V and D are those of the mode off; the opacity changes (smaller) and so does the alpha cut (more negative opacity:
    a cut at least as close to 0)."""
    verts = oracle.activate_records(_sub_pixel_and_needles(pkg))
    u = pkg.camera_uniforms(pkg.make_camera(), 960, 540)
    scene = pkg.Scene.from_vertices(verts, device=0)
    rend = pkg.Renderer(scene)
    rend.render_host(u)
    off = _taps(rend, u)
    co_off = rend.stage("conic_opacity").reshape(-1, 4)[off["tiles"] != 0]
    rend.set_antialiased(True)
    rend.render_host(u)
    on = _taps(rend, u)
    co_on = rend.stage("conic_opacity").reshape(-1, 4)[on["tiles"] != 0]
    _assert_taps_equal(off, on, "mode on vs off", only=[k for k in off if k not in ("conic_opacity", "alpha_cut")])
    np.testing.assert_array_equal(co_on[:, :3].view(np.uint32), co_off[:, :3].view(np.uint32))
    assert (co_on[:, 3] <= co_off[:, 3]).all() and (co_on[:, 3] < co_off[:, 3]).mean() > 0.99
    cut_on, cut_off = on["alpha_cut"].view(np.float32), off["alpha_cut"].view(np.float32)
    assert (cut_on >= cut_off).all()
    scene.close()


def test_factor_against_float64(pkg, oracle, gpu):
    """comp_gpu = opacity' / opacity (binary32 opacity' = fl(opacity comp): relative error <= 2^-24 from that rounding) against
    float64 comp from np_reference's 2D covariance, within aa_reference.comp_tolerance -- a first-order bound of det(cov2D)'s
    cancellation under float64_check's error model, not a tuned constant.  The same check rejects a dilation of 0.31, a missing
    square root and det(cov2D) taken from the dilated matrix; and comp < 1 wherever det(cov2D) > 0."""
    rec = _sub_pixel_and_needles(pkg, n=20000, seed=47)
    w, h = 960, 540
    u = pkg.camera_uniforms(pkg.make_camera(), w, h)
    scene = pkg.Scene.from_records(rec, device=0)
    rend = pkg.Renderer(scene)
    rend.render_host(u)
    plain = rend.stage("conic_opacity").reshape(-1, 4)[:, 3].copy()
    rend.set_antialiased(True)
    rend.render_host(u)
    vis = rend.stage("tiles") != 0
    scaled = rend.stage("conic_opacity").reshape(-1, 4)[:, 3]
    comp_gpu = scaled[vis].astype(np.float64) / plain[vis]

    cam = npr.camera((0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0), float(np.float32(45.0)), float(np.float32(0.1)),
                     float(np.float32(1000.0)), w, h)
    sc = npr.activate(rec)
    pre = npr.preprocess(sc, cam)
    sub = {k: (v[vis] if isinstance(v, np.ndarray) and v.shape[:1] == (len(rec),) else v) for k, v in pre.items()}
    want = aa.comp64(sub)
    bad = aa.comp_violations(comp_gpu, sub, want)
    assert not bad.any(), (f"{bad.sum()} of {len(bad)} factors outside the bound; worst |d comp^2| / bound = "
                           f"{float((np.abs(comp_gpu ** 2 - want ** 2) / aa.comp_tolerance(sub)).max()):.3g}")
    print(f"comp vs float64: worst |d comp^2| / bound = {float((np.abs(comp_gpu ** 2 - want ** 2) / aa.comp_tolerance(sub)).max()):.3g}")
    pre31 = npr.preprocess(sc, cam, dict(dilation=0.31))
    sub31 = {k: (v[vis] if isinstance(v, np.ndarray) and v.shape[:1] == (len(rec),) else v) for k, v in pre31.items()}
    for label, mutated in (("dilation 0.31", aa.comp64(sub31, rules=dict(dilation=0.31))), ("no sqrt", aa.comp64(sub, sqrt=False)),
                           ("det_raw from the dilated matrix", aa.comp64(sub, raw_from_dilated=True))):
        assert aa.comp_violations(comp_gpu, sub, mutated).mean() > 0.5, label
    a, b, c = sub["cov2d"].T
    raw = (a - 0.3) * (c - 0.3) - b * b
    assert (comp_gpu[raw > 0] < 1).all()
    scene.close()


def test_per_frame_alpha_cut_is_the_load_time_cut_for_every_opacity(pkg, gpu):
    """The mode's per-frame cut (a seeded search) returns the bits of the load-time bisection for EVERY binary32 opacity: all
    2^32 patterns, NaNs, infinities, negatives and subnormals included."""
    bad, first = pkg.debug_alpha_cut_scan(0, 1 << 32)
    assert bad == 0, f"{bad} opacities differ, the first with pattern {first:#010x}"


def test_sparse_sub_pixel_splats_are_dimmer(pkg, oracle, gpu):
    """Isolated sub-pixel splats on the black background: every pixel is colour x min(0.99, o exp(power)) of one splat, so with
    opacity' <= opacity every pixel of the antialiased frame is <= the plain frame's, and most lit ones strictly lower.  (The
    frame's alpha channel is 1 everywhere, render.comp:98: coverage cannot be read from it.)"""
    w, h, step = 640, 352, 16
    xs, ys = np.meshgrid(np.arange(8, w, step), np.arange(8, h, step))
    n = xs.size
    cam = pkg.make_camera()
    u = pkg.camera_uniforms(cam, w, h)
    # place splat k at pixel (xs, ys) on the plane z = -4 (p_view.z = 4), through the pinhole
    tan_x = np.tan(np.radians(45.0) / 2)
    tan_y = tan_x * h / w
    z = 4.0
    px = ((2 * (xs.ravel() + 0.5) / w) - 1) * tan_x * z
    py = -((2 * (ys.ravel() + 0.5) / h) - 1) * tan_y * z
    rec = np.zeros((n, 62), np.float32)
    rec[:, 0], rec[:, 1], rec[:, 2] = px, py, -z
    rec[:, 6:9] = 1.5                           # SH DC: a positive colour in every channel, no view dependence
    rec[:, 54] = 2.0                            # opacity 0.88
    rec[:, 55:58] = np.log(0.0015)              # ~0.6 px across
    rec[:, 58] = 1.0
    scene = pkg.Scene.from_records(rec, device=0)
    rend = pkg.Renderer(scene)
    plain, _ = rend.render_host(u)
    assert rend.stats().num_visible == n
    rend.set_antialiased(True)
    dim, _ = rend.render_host(u)
    assert (dim[..., 3] == 1).all() and (plain[..., 3] == 1).all()
    lit = plain[..., :3] > 0
    assert lit.sum() >= 9 * n
    assert (dim[..., :3] <= plain[..., :3]).all()
    assert (dim[..., :3][lit] < plain[..., :3][lit]).mean() > 0.9
    assert dim[..., :3].sum() < 0.8 * plain[..., :3].sum()
    scene.close()


class _HipBuffers:
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


def test_switching_the_mode(pkg, oracle, gpu, monkeypatch):
    """Three frames in flight, the mode alternating per frame, each frame into its own buffer: every frame is the serial frame of
    its own setting.  Graph replay captures both variants (the toggle re-uses neither's graph for the other).  GS_ANTIALIASED=1 at
    creation is set_antialiased(1), and switching off again gives the default bits."""
    rec = _sub_pixel_and_needles(pkg, n=12000, seed=53)
    w, h = 640, 360
    poses = [pkg.camera_uniforms(pkg.make_camera(position=(0.02 * k, 0.0, 0.03 * k), rotation=pkg.dist.pose_quaternion(k, 1.0)), w, h)
             for k in range(6)]
    scene = pkg.Scene.from_records(rec, device=0)
    rend = pkg.Renderer(scene)
    assert not rend.antialiased
    serial = {}
    for aa_on in (False, True):
        rend.set_antialiased(aa_on)
        for k, u in enumerate(poses):
            serial[aa_on, k] = rend.render_host(u)[0]
    for k in range(len(poses)):
        assert not np.array_equal(serial[False, k], serial[True, k])
    dev = _HipBuffers()
    for graph in (False, True):
        rend.set_graph_mode(graph)
        rend.set_frames_in_flight(3)
        outs = [dev.alloc(w * h * 16) for _ in poses]
        for rep in range(2):
            for k, (u, o) in enumerate(zip(poses, outs)):
                rend.set_antialiased(k % 2 == 1)
                rend.render(u, o, 0)
            rend.synchronize()
            for k, o in enumerate(outs):
                np.testing.assert_array_equal(dev.download(o, (h, w, 4), np.float32), serial[k % 2 == 1, k],
                                              err_msg=f"graph {graph}, pass {rep}, frame {k}")
    rend.set_graph_mode(False)
    rend.set_frames_in_flight(1)
    rend.set_antialiased(False)
    assert not rend.antialiased
    again, _ = rend.render_host(poses[0])
    np.testing.assert_array_equal(again.view(np.uint32), serial[False, 0].view(np.uint32))
    monkeypatch.setenv("GS_ANTIALIASED", "1")
    r2 = pkg.Renderer(scene)
    assert r2.antialiased
    img, _ = r2.render_host(poses[1])
    np.testing.assert_array_equal(img.view(np.uint32), serial[True, 1].view(np.uint32))
    dev.close()
    scene.close()
