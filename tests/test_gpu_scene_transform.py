"""gs_scene_transform on the device (k_scene_transform, gs_scene.hip): a scene moved in place by x -> s R x + t.

DATA.  The downloaded result against the float64 transform (tests/transform_reference.py) of the downloaded original, with the
tolerances the kernel's documented operation order gives, eps = 2^-24 (half an ulp, relative; R, q and M_l reach the kernel rounded
once to binary32, which is one of the roundings counted):
    positions    s * ((R_k0 x + R_k1 y) + R_k2 z) + t_k: three rounded entries of R, three products, two sums, the product with s
                 and the sum with t, each <= eps of a partial result <= s |p|_1 + |t_k|:            8 eps (s |p|_1 + |t_k|)
    scales       one product:                                                                       4 eps relative
    quaternions  four rounded components of q, four products and three sums per component (each partial result <= 1), then the
                 norm (two relative eps) and the product with its reciprocal:                        8 eps absolute, sign as computed;
                 the norm of the result within 4 eps of 1
    SH band l    2l+1 rounded entries of M, 2l+1 products, 2l sums, |M_ij| <= 1:                     16 eps |c_l|_1 per channel
Opacity, the DC term, every Gaussian outside the range and the blob's padding keep their bits.
DERIVED DATA is consistent bit for bit: cov3D and the frame are the oracle's of the downloaded vertices.
INVARIANCE: the moved scene through the moved camera shows the original frame within the caps that
tests/test_transform_invariance_yardstick.py pins on the reference alone.
"""
import functools

import numpy as np
import pytest

import transform_reference as tr
from helpers import assert_images_identical
from test_gpu_device_arrays import raw_blob  # the scene's blob as it lies in HBM, through hipMemcpy

pytestmark = pytest.mark.gpu

W, H = tr.W, tr.H
EPS = 2.0 ** -24
T1 = (tr.ROTATION, tr.TRANSLATION, 1.7)
T2 = ((-0.2, 0.9, 0.1, -0.35), (-2.0, 0.25, 1.1), 0.4)


@functools.lru_cache(maxsize=None)
def records(n, seed=3):
    import __graft_entry__ as entry
    r = entry.load_package().synth.synth_records(n, seed=seed, kind="A")
    r.setflags(write=False)
    return r


def once(_sort_path):
    if _sort_path == "1":
        pytest.skip("independent of the depth-order path: runs once")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def as_oracle(oracle, verts, half_sh=False):
    v = np.ascontiguousarray(verts, np.float32).copy()
    if half_sh:  # what a quantised scene renders from: every coefficient rounded to binary16, ties to even
        v[:, 12:60] = v[:, 12:60].astype(np.float16).astype(np.float32)
    return v.view(oracle.VERTEX_DT).reshape(-1)


def check_data(got, orig, transform, first, count, factor=1.0, translations=None, label=""):
    """got / orig: (n, 60) downloaded vertices after / before; transform = (rotation, translation, scale) of the whole move.
    translations: per component, the magnitudes |t_k| that were rounded on the way, in the result's units (default: the transform's own)."""
    q, t, s = tr.params32(*transform)
    want = tr.transform_vertices(orig, *transform, first=first, count=count)
    sel = slice(first, first + count)
    outside = np.ones(len(orig), bool)
    outside[sel] = False
    assert np.array_equal(bits(got[outside]), bits(orig[outside])), f"{label}: a Gaussian outside the range changed"
    assert np.array_equal(bits(got[sel, 7]), bits(orig[sel, 7])), f"{label}: opacity changed"
    assert np.array_equal(bits(got[sel, 12:15]), bits(orig[sel, 12:15])), f"{label}: the SH DC term changed"
    assert np.array_equal(bits(got[sel, 3]), bits(orig[sel, 3]))
    g, w, o = got[sel].astype(np.float64), want[sel], orig[sel].astype(np.float64)
    t_mag = np.abs(t) if translations is None else np.asarray(translations, np.float64).reshape(3)
    tol_pos = factor * 8 * EPS * (s * np.abs(o[:, 0:3]).sum(axis=1, keepdims=True) + t_mag)
    worst = dict(pos=float((np.abs(g[:, 0:3] - w[:, 0:3]) / tol_pos).max()),
                 scale=float((np.abs(g[:, 4:7] / w[:, 4:7] - 1) / (factor * 4 * EPS)).max()),
                 rot=float((np.abs(g[:, 8:12] - w[:, 8:12]) / (factor * 8 * EPS)).max()),
                 norm=float((np.abs(np.linalg.norm(g[:, 8:12], axis=1) - 1) / (4 * EPS)).max()))
    sh_g, sh_w, sh_o = (a[:, 12:60].reshape(-1, 16, 3) for a in (g, w, o))
    for l, js in tr.BANDS.items():
        tol = factor * 16 * EPS * np.abs(sh_o[:, js, :]).sum(axis=1, keepdims=True)
        worst[f"sh{l}"] = float((np.abs(sh_g[:, js, :] - sh_w[:, js, :]) / (tol + 1e-300)).max())  # (a band of zeros stays zero)
    print(f"{label}: error / tolerance " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, f"{label}: beyond the tolerance (error / tolerance): {bad}"


def check_blob_outside(before, after, n, first, count, label=""):
    """The raw blob: padding of the 11 planes, the opacity plane and everything of Gaussians outside the range, bit for bit."""
    st = (n + 15) & ~15
    keep = np.ones(len(before), bool)
    for p in range(11):
        if p != 10:
            keep[p * st + first:p * st + first + count] = False
    keep[11 * st + 48 * first:11 * st + 48 * (first + count)] = False
    assert keep[10 * st:11 * st].all() and all(keep[p * st + n:(p + 1) * st].all() for p in range(11))
    assert np.array_equal(bits(before)[keep], bits(after)[keep]), f"{label}: the blob changed outside the range"


def check_derived(pkg, oracle, scene, rend=None, half_sh=False, label=""):
    """cov3D and the frame of the scene as it stands = the oracle's of its downloaded vertices, bit for bit."""
    verts = scene.download_vertices()
    np.testing.assert_array_equal(bits(scene.download_cov3d()), bits(oracle.cov3d(as_oracle(oracle, verts))), err_msg=f"{label}: cov3D")
    own = rend is None
    rend = rend or pkg.Renderer(scene)
    u = pkg.camera_uniforms(pkg.make_camera(), W, H)
    img, _ = rend.render_host(u)
    ref = oracle.stages(as_oracle(oracle, verts, half_sh), u)
    assert_images_identical(img, ref["image"], label)
    if own:
        rend.close()
    return img


# ---- data ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 15, 16, 17, 255, 256, 257, 1000])
def test_a_whole_scene_is_moved_as_float64_moves_it(pkg, oracle, gpu, _sort_path, n):
    """The planes' padding edge (16) and the workgroup's (256), from both sides; 1000: four workgroups, the last one partial."""
    once(_sort_path)
    scene = pkg.Scene.from_records(records(n))
    orig, blob = scene.download_vertices(), raw_blob(scene)
    scene.transform(*T1)
    got = scene.download_vertices()
    check_data(got, orig, T1, 0, n, label=f"n={n}")
    assert np.abs(got[:, 15:60] - orig[:, 15:60]).max() > 1e-3  # the bands did move
    check_blob_outside(blob, raw_blob(scene), n, 0, n, f"n={n}")
    check_derived(pkg, oracle, scene, label=f"n={n}")


N_RANGE = 600
RANGES = [(0, 1), (599, 1), (255, 2), (3, 250), (0, 600)]


@pytest.mark.parametrize("first,count", RANGES)
def test_a_range_is_moved_and_nothing_else(pkg, oracle, gpu, _sort_path, first, count):
    scene = pkg.Scene.from_records(records(N_RANGE))
    rend = pkg.Renderer(scene)
    check_derived(pkg, oracle, scene, rend, label="before")
    orig, blob = scene.download_vertices(), raw_blob(scene)
    rend.synchronize()
    scene.transform(*T2, first=first, count=count)
    label = f"[{first}, {first + count})"
    check_data(scene.download_vertices(), orig, T2, first, count, label=label)
    check_blob_outside(blob, raw_blob(scene), N_RANGE, first, count, label)
    check_derived(pkg, oracle, scene, rend, label=label)  # cov3D was redone over the range only: the rest must still be right


def test_count_none_reaches_the_end_and_an_identity_renormalises(pkg, oracle, gpu, _sort_path):
    once(_sort_path)
    scene = pkg.Scene.from_records(records(N_RANGE))
    orig = scene.download_vertices()
    scene.transform(first=590)  # the identity, [590, 600)
    got = scene.download_vertices()
    assert np.array_equal(bits(got[:590]), bits(orig[:590]))
    g, o = got[590:].astype(np.float64), orig[590:].astype(np.float64)
    assert np.array_equal(bits(got[590:, 0:8]), bits(orig[590:, 0:8]))       # 1 * x + 0, exactly
    assert np.array_equal(bits(got[590:, 12:60]), bits(orig[590:, 12:60]))   # identity matrices, exactly
    assert np.abs(g[:, 8:12] - o[:, 8:12]).max() <= 8 * EPS and np.abs(np.linalg.norm(g[:, 8:12], axis=1) - 1).max() <= 4 * EPS
    check_derived(pkg, oracle, scene, label="identity")


def test_out_of_range_calls_and_empty_ranges_leave_the_blob_alone(pkg, gpu, _sort_path):
    once(_sort_path)
    scene = pkg.Scene.from_records(records(N_RANGE))
    before = raw_blob(scene)
    scene.transform(*T1, first=0, count=0)
    scene.transform(*T1, first=N_RANGE, count=0)  # no Gaussians, at the very end
    scene.transform(*T1, first=N_RANGE)           # count None: to the end
    for first, count in ((N_RANGE, 1), (N_RANGE - 1, 2), (2 ** 64 - 1, 2), (1, N_RANGE), (N_RANGE + 1, 0)):
        with pytest.raises(pkg.binding.GsError, match="out of bounds") as e:
            scene.transform(*T1, first=first, count=count)
        assert e.value.code == -1
    with pytest.raises(pkg.binding.GsError, match="scale"):
        scene.transform(scale=-2.0)
    np.testing.assert_array_equal(bits(raw_blob(scene)), bits(before))


# ---- derived data ----------------------------------------------------------------------------------------------------------------
def test_a_quantised_scene_is_requantised(pkg, oracle, gpu, _sort_path):
    scene = pkg.Scene.from_records(records(N_RANGE))
    scene.quantize_sh()
    rend = pkg.Renderer(scene)
    stale = check_derived(pkg, oracle, scene, rend, half_sh=True, label="quantised, before")
    rend.synchronize()
    scene.transform(*T2, first=3, count=250)
    assert scene.sh_bits == 16
    img = check_derived(pkg, oracle, scene, rend, half_sh=True, label="quantised, a range")
    assert not np.array_equal(img, stale)
    rend.synchronize()
    scene.transform(*T1)
    check_derived(pkg, oracle, scene, rend, half_sh=True, label="quantised, whole")


def test_a_scene_with_a_copy_in_spatial_order(pkg, oracle, gpu, _sort_path, monkeypatch):
    """GS_SPATIAL_MIN=1 forces the second copy and `perm`: the move must reach the copy the frames read (cov3D lives in ITS order),
    whole planes, while the order itself stays that of the positions the scene was built with."""
    monkeypatch.setenv("GS_SPATIAL_MIN", "1")
    scene = pkg.Scene.from_records(records(N_RANGE))
    rend = pkg.Renderer(scene)
    check_derived(pkg, oracle, scene, rend, label="spatial copy, before")
    orig = scene.download_vertices()
    rend.synchronize()
    scene.transform(*T2, first=3, count=250)
    check_data(scene.download_vertices(), orig, T2, 3, 250, label="spatial copy")
    check_derived(pkg, oracle, scene, rend, label="spatial copy, a range")
    rend.synchronize()
    scene.transform(*T1)
    check_derived(pkg, oracle, scene, rend, label="spatial copy, whole")


# ---- invariance ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", tr.SCALES)
@pytest.mark.parametrize("n", [1200, 5000])
def test_the_moved_scene_through_the_moved_camera_shows_the_same_frame(pkg, gpu, _sort_path, n, scale):
    """The yardstick's inputs; its caps: mean |d| <= 2e-4, at most 2 % of the pixels beyond 1e-3 (the reference alone stays within
    half of each: tests/test_transform_invariance_yardstick.py)."""
    scene = pkg.Scene.from_records(records(n))
    rend = pkg.Renderer(scene)
    cam = pkg.make_camera(position=tr.CAMERA["position"], rotation=tr.unit(tr.CAMERA["rotation"]))
    before, _ = rend.render_host(pkg.camera_uniforms(cam, W, H))
    visible = rend.stats().num_visible
    scene.transform(tr.ROTATION, tr.TRANSLATION, scale)  # (render_host has synchronised the renderer)
    cam2 = pkg.transform_camera(cam, tr.ROTATION, tr.TRANSLATION, scale)
    after, _ = rend.render_host(pkg.camera_uniforms(cam2, W, H))
    mean, beyond, worst = tr.frame_difference(after, before)
    print(f"n={n} s={scale}: visible {visible} / {rend.stats().num_visible}, mean |d| {mean:.3g}, beyond 1e-3: {beyond * 100:.2f} %, max |d| {worst:.3g}")
    assert visible > n // 2 and before[..., :3].max() > 0.1
    assert mean <= tr.CAP_MEAN and beyond <= tr.CAP_FRACTION
    unmoved, _ = rend.render_host(pkg.camera_uniforms(cam, W, H))
    assert tr.frame_difference(unmoved, before)[0] > 10 * tr.CAP_MEAN  # the scene did move


# ---- round trip and composition ----------------------------------------------------------------------------------------------------
def rounded_translations(first, second):
    """Per component k of the result of `first` then `second`: what the two translations contribute to the magnitudes that
    are rounded on the way -- the first step's, carried through the second (s2 sum_j |R2_kj| |t1_j|), plus |t2_k|."""
    _, t1, _ = tr.params32(*first)
    q2, t2, s2 = tr.params32(*second)
    return s2 * np.abs(tr.rotation_matrix(q2)) @ np.abs(t1) + np.abs(t2)


def test_a_move_and_its_inverse_give_the_scene_back(pkg, gpu, _sort_path):
    """Three times the data tolerances, the identity being the transform compared with; |t_k| in them is what both steps'
    translations put into component k (rounded_translations): a Gaussian near the origin passes through |t1| on the way."""
    once(_sort_path)
    n = 1000
    scene = pkg.Scene.from_records(records(n))
    orig = scene.download_vertices()
    inv = tr.inverse(*T1)
    scene.transform(*T1)
    scene.transform(*inv)
    t_mag = rounded_translations(T1, inv)
    check_data(scene.download_vertices(), orig, ((1, 0, 0, 0), (0, 0, 0), 1.0), 0, n, factor=3.0, translations=t_mag, label="T then its inverse")


def test_two_moves_equal_the_composed_move(pkg, gpu, _sort_path):
    """Three times the data tolerances around the float64 move by the composed transform (as binary32 carries it); |t_k| in
    them is what both steps' translations put into component k (rounded_translations)."""
    once(_sort_path)
    n = 1000
    two, one = pkg.Scene.from_records(records(n)), pkg.Scene.from_records(records(n))
    orig = two.download_vertices()
    two.transform(*T1, first=100, count=800)
    two.transform(*T2, first=100, count=800)
    both = tr.compose(T2, T1)
    one.transform(*both, first=100, count=800)
    t_mag = rounded_translations(T1, T2)
    check_data(two.download_vertices(), orig, both, 100, 800, factor=3.0, translations=t_mag, label="T1 then T2")
    check_data(one.download_vertices(), orig, both, 100, 800, label="the composed move")


# ---- frames ----------------------------------------------------------------------------------------------------------------------
N_FRAME = 1200
_FRAMES = {}


def fresh_frame(pkg, key, make_vertices):
    """The frame (default camera) of a fresh scene made from vertices, computed once per key and shared."""
    if key not in _FRAMES:
        scene = pkg.Scene.from_vertices(make_vertices())
        rend = pkg.Renderer(scene)
        img, _ = rend.render_host(pkg.camera_uniforms(pkg.make_camera(), W, H))
        img.setflags(write=False)
        _FRAMES[key] = img
        rend.close()
        scene.close()
    return _FRAMES[key]


@pytest.mark.parametrize("mode", ["plain", "graph", "two_in_flight"])
def test_the_same_renderer_shows_the_moved_scene(pkg, gpu, _sort_path, mode):
    import torch
    move = ((0.98, 0.05, -0.15, 0.1), (0.1, -0.05, 0.2), 1.1)  # gentle: the scene stays in view
    scene = pkg.Scene.from_records(records(N_FRAME))
    rend = pkg.Renderer(scene)
    u = pkg.camera_uniforms(pkg.make_camera(), W, H)
    if mode == "graph":
        rend.set_graph_mode(True)
    frames = 2 if mode == "two_in_flight" else 1
    if frames == 2:
        rend.set_frames_in_flight(2)
    out = [torch.zeros(H, W, 4, device="cuda") for _ in range(frames)]
    torch.cuda.synchronize()  # (the renderer's streams do not wait for torch's)

    def render():
        for _ in range(2):  # (graph mode: the second round replays what the first captured)
            for o in out:
                rend.render(u, o.data_ptr())
        rend.synchronize()
        return [o.cpu().numpy() for o in out]

    old = fresh_frame(pkg, ("old", _sort_path), lambda: pkg.activate_records(records(N_FRAME)))
    for img in render():
        assert np.array_equal(bits(img), bits(old))
    scene.transform(*move, first=200, count=900)  # (render() has synchronised the renderer)
    moved = scene.download_vertices()
    want = fresh_frame(pkg, ("moved", _sort_path), lambda: moved)
    for img in render():
        assert np.array_equal(bits(img), bits(want)), f"{mode}: the frame after the move is not the frame of a fresh scene of the same vertices"
    assert tr.frame_difference(want, old)[0] > 10 * tr.CAP_MEAN and want[..., :3].max() > 0.1


def test_the_move_runs_on_the_callers_stream(pkg, gpu, _sort_path):
    """Tensors filled and handed to the scene on a torch stream, then the move on the same stream without a synchronisation in
    between: the result is the serial one."""
    once(_sort_path)
    import torch
    n, first, count = 1000, 100, 700
    new = records(n, seed=11)[:count]
    host = dict(means=new[:, 0:3], log_scales=new[:, 55:58], quats=new[:, 58:62], opacity_logits=new[:, 54], sh_dc=new[:, 6:9],
                sh_rest=new[:, 9:54].reshape(count, 3, 15).transpose(0, 2, 1))
    host = {k: np.array(v, np.float32, order="C") for k, v in host.items()}
    serial = pkg.Scene.from_records(records(n))
    serial.update_from_tensors(first, **{k: torch.from_numpy(v).cuda() for k, v in host.items()})
    torch.cuda.synchronize()
    serial.transform(*T1, first=50, count=900)
    want = raw_blob(serial)
    stream = torch.cuda.Stream()
    by_current, explicit, raw = (pkg.Scene.from_records(records(n)) for _ in range(3))
    with torch.cuda.stream(stream):
        d = {k: torch.from_numpy(v).pin_memory().to("cuda", non_blocking=True) for k, v in host.items()}
        by_current.update_from_tensors(first, **d)        # stream=None: torch's current stream, i.e. `stream`
        by_current.transform(*T1, first=50, count=900)
    explicit.update_from_tensors(first, **d, stream=stream)
    explicit.transform(*T1, first=50, count=900, stream=stream)
    raw.update_from_tensors(first, **d, stream=stream.cuda_stream)
    raw.transform(*T1, first=50, count=900, stream=stream.cuda_stream)
    for s in (by_current, explicit, raw):
        np.testing.assert_array_equal(bits(raw_blob(s)), bits(want))
        np.testing.assert_array_equal(bits(s.download_cov3d()), bits(serial.download_cov3d()))
