"""A scene built and refreshed from a trainer's device arrays (gs_scene_from_device_arrays, gs_scene_update_from_device_arrays)
must be BIT FOR BIT the scene the host path builds from the same numbers: Scene.from_records of the (n, 62) records the six
arrays are cut from.  "Equal" below is bitwise wherever the host value is not a NaN, and a NaN where it is (the default NaNs
of x86 and gfx950 differ in sign).  Compared: the downloaded vertices, cov3D, the raw blob, the alpha cuts a frame carries and
the frame itself (exp mode 2, the suite's default: frames of equal scenes are bit-identical).
"""
import ctypes
import functools

import numpy as np
import pytest

from helpers import assert_guarded_close, oracle_frame

pytestmark = pytest.mark.gpu

W, H = 128, 96
MEMBERS = ("means", "log_scales", "quats", "opacity_logits", "sh_dc", "sh_rest")
COLUMNS = dict(means=slice(0, 3), sh_dc=slice(6, 9), sh_rest=slice(9, 54), opacity_logits=slice(54, 55), log_scales=slice(55, 58),
               quats=slice(58, 62))


def cut(r):
    """The six arrays of (n, 62) PLY-domain records, as a trainer holds them (host side, C-contiguous)."""
    r = np.ascontiguousarray(r, np.float32)
    n = len(r)
    a = dict(means=r[:, 0:3], sh_dc=r[:, 6:9], sh_rest=r[:, 9:54].reshape(n, 3, 15).transpose(0, 2, 1), opacity_logits=r[:, 54],
             log_scales=r[:, 55:58], quats=r[:, 58:62])
    return {k: np.array(v, np.float32, order="C") for k, v in a.items()}  # (copies: writable, dense)


def to_device(arrays, offset=False):
    """torch tensors on the GPU; offset: each a slice, one float in, of a larger allocation -- 4-byte aligned and no more."""
    import torch
    out = {}
    for k, v in arrays.items():
        t = torch.from_numpy(v)
        if offset:
            big = torch.empty(v.size + 1, dtype=torch.float32, device="cuda")
            big[1:].copy_(t.reshape(-1))
            d = big[1:].view(v.shape)
            assert d.data_ptr() % 16 == 4 and d.is_contiguous()
        else:
            d = t.cuda()
        out[k] = d
    return out


def merge(base, new, first, members=MEMBERS):
    """base with the `members` of Gaussians [first, first + len(new)) taken from `new`."""
    m = base.copy()
    for k in members:
        m[first:first + len(new), COLUMNS[k]] = new[:, COLUMNS[k]]
    return m


def same(dev, host, label):
    dev, host = np.ascontiguousarray(dev, np.float32), np.ascontiguousarray(host, np.float32)
    assert dev.shape == host.shape, (label, dev.shape, host.shape)
    nan = np.isnan(host)
    assert np.isnan(dev[nan]).all(), f"{label}: a NaN of the host path is a number here"
    bad = np.argwhere((dev.view(np.uint32) != host.view(np.uint32)) & ~nan)
    assert len(bad) == 0, f"{label}: {len(bad)} value(s) differ in their bits, first at {tuple(bad[0])}: {dev[tuple(bad[0])]!r} != {host[tuple(bad[0])]!r}"


def raw_blob(scene):
    hip = ctypes.CDLL("libamdhip64.so")
    ptr, floats = scene.blob()
    host = np.empty(floats, np.float32)
    assert hip.hipMemcpy(host.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(ptr), ctypes.c_size_t(floats * 4), ctypes.c_int(2)) == 0
    return host


def state(pkg, scene, frame=True, rend=None):
    """Everything of a scene that can be read back: vertices, cov3D, the raw blob; with a frame, its pixels and the alpha cuts of
    the visible Gaussians (GS_STAGE_ALPHA_CUT)."""
    s = dict(vertices=scene.download_vertices(), cov3d=scene.download_cov3d(), blob=raw_blob(scene))
    if frame:
        own = rend is None
        rend = rend or pkg.Renderer(scene)
        u = pkg.camera_uniforms(pkg.make_camera(), W, H)
        s["image"], _ = rend.render_host(u)
        vis = rend.stage("tiles") != 0
        s["visible"] = vis
        s["alpha_cut"] = np.where(vis, rend.stage("alpha_cut"), 0).astype(np.float32)
        if own:
            rend.close()
    return s


def same_state(got, want, label):
    for k in ("vertices", "cov3d", "blob", "alpha_cut"):
        if k in want:
            same(got[k], want[k], f"{label}: {k}")
    if "image" in want:
        np.testing.assert_array_equal(got["visible"], want["visible"])
        assert np.array_equal(got["image"].view(np.uint32), want["image"].view(np.uint32)), f"{label}: the frames differ"


@functools.lru_cache(maxsize=None)
def records(n, seed=3):
    import __graft_entry__ as entry
    r = entry.load_package().synth.synth_records(n, seed=seed, kind="A")
    r.setflags(write=False)
    return r


_REFERENCE = {}


def reference(pkg, key, make_records, quantized=False):
    """The state of Scene.from_records(make_records()), computed once per key and shared."""
    if key not in _REFERENCE:
        scene = pkg.Scene.from_records(make_records())
        if quantized:
            scene.quantize_sh()
        _REFERENCE[key] = state(pkg, scene)
        scene.close()
    return _REFERENCE[key]


def once(_sort_path):
    if _sort_path == "1":
        pytest.skip("independent of the depth-order path: runs once")


# ---- build -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 15, 16, 17, 255, 256, 257, 1000])
def test_a_scene_from_tensors_equals_the_scene_from_records(pkg, gpu, _sort_path, n):
    """The planes' padding edge (16) and the workgroup's (256), from both sides."""
    once(_sort_path)
    want = reference(pkg, ("build", n), lambda: records(n))
    scene = pkg.Scene.from_tensors(**to_device(cut(records(n))))
    assert scene.num_vertices == n
    same_state(state(pkg, scene), want, f"n={n}")


@pytest.mark.parametrize("k", [0, 3, 8, 15])
def test_sh_degrees_below_three_leave_the_higher_bands_zero(pkg, gpu, _sort_path, k):
    once(_sort_path)
    n = 257
    a = cut(records(n))
    a["sh_rest"] = np.ascontiguousarray(a["sh_rest"][:, :k, :])
    zeroed = records(n).copy()
    for c in range(3):  # planar in the record: 15 R, 15 G, 15 B
        zeroed[:, 9 + 15 * c + k:9 + 15 * (c + 1)] = 0
    want = reference(pkg, ("degree", k), lambda: zeroed)
    d = to_device(a)
    for sh_rest in ([d["sh_rest"]] if k else [d["sh_rest"], None]):  # (n, 0, 3) and None both mean degree 0
        scene = pkg.Scene.from_tensors(**dict(d, sh_rest=sh_rest))
        same_state(state(pkg, scene), want, f"sh_rest_coeffs={k}")


def test_arrays_that_are_only_four_byte_aligned(pkg, gpu, _sort_path):
    once(_sort_path)
    n = 257
    scene = pkg.Scene.from_tensors(**to_device(cut(records(n)), offset=True))
    same_state(state(pkg, scene), reference(pkg, ("build", n), lambda: records(n)), "offset slices")


def test_the_ingest_runs_on_the_callers_stream(pkg, gpu, _sort_path):
    """The arrays are filled on a non-default stream and handed over without a synchronisation: the ingest must queue behind."""
    once(_sort_path)
    import torch
    n = 1000
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d = {k: torch.from_numpy(v).pin_memory().to("cuda", non_blocking=True) for k, v in cut(records(n)).items()}
        by_current = pkg.Scene.from_tensors(**d)  # stream=None: torch's current stream, i.e. `stream`
    explicit = pkg.Scene.from_tensors(**d, stream=stream)
    raw = pkg.Scene.from_tensors(**d, stream=stream.cuda_stream)
    for s in (by_current, explicit, raw):
        same_state(state(pkg, s), reference(pkg, ("build", n), lambda: records(n)), "non-default stream")


# ---- activation at the edges of its domain ----------------------------------------------------------------------------------
def _bits(b):
    return np.array([b], np.uint32).view(np.float32)[0]


def edge_records():
    under = np.float32(float.fromhex("-0x1.9fe368p6"))  # glibc's underflow bound
    vals = [0.0, -0.0, np.inf, -np.inf, np.nan, 1e38, -1e38, 1e-45, -1e-45, _bits(0x42B17217), _bits(0x42B17218),
            under, np.nextafter(under, np.float32(0)), np.nextafter(under, np.float32(-np.inf)), -87.4, -100.0, 16.7, -16.7]
    vals = np.array(vals + [-v for v in vals], np.float32)  # the sigmoid evaluates exp(-logit): both signs of everything
    n = 300
    r = records(n).copy()
    for i in range(n):
        r[i, 54] = vals[i % len(vals)]
        for k in range(3):
            r[i, 55 + k] = vals[(i // len(vals) + 5 * k + i) % len(vals)]
    quats = np.array([[0, 0, 0, 0], [1e-45, 0, 0, 0], [1e-40, -1e-41, 3e-39, 1e-45], [1e-20, 1e-20, 1e-20, 1e-20], [1e20, 0, 0, 0],
                      [1e20, -1e20, 1e20, 1e20], [3e38, 3e38, 3e38, 3e38], [np.nan, 1, 0, 0], [1, 0, np.nan, 0], [np.inf, 1, 1, 1],
                      [-0.0, 0, 0, 2], [1, 2, 3, 4]], np.float32)
    r[40:40 + len(quats), 58:62] = quats
    return r


def test_activation_equals_the_hosts_on_edge_values(pkg, gpu, _sort_path):
    """exp over/underflow on either side of libm's bounds, subnormal results, the sigmoid's saturation, quaternions whose norm
    underflows, overflows or is NaN: the device's exp, division and square root against gs_activate_records."""
    once(_sort_path)
    r = edge_records()
    with np.errstate(all="ignore"):
        want = pkg.activate_records(r)
    scene = pkg.Scene.from_tensors(**to_device(cut(r)))
    got = scene.download_vertices()
    same(got, want, "edge values")
    # the cases are what they claim to be
    assert np.isinf(want[:, 4:7]).any() and (want[:, 4:7] == 0).any() and np.isnan(want[:, 4:8]).any() and np.isnan(want[:, 8:12]).any()
    tiny = np.float32(np.finfo(np.float32).tiny)
    assert ((want[:, 4:8] > 0) & (want[:, 4:8] < tiny)).any() and (want[:, 7] == 1).any()


def test_the_ingests_exp_equals_libm_on_every_nonnegative_binary32(pkg, oracle, gpu, _sort_path):
    """[+0, +inf]: 2 139 095 041 values through the device function itself (the negative half: test_gpu_expf.py, through the
    function this one wraps)."""
    once(_sort_path)
    first, count = 0x00000000, 0x7F800000 + 1
    dev = pkg.binding.debug_activation_expf_scan(first, count)
    host = oracle.libm_expf_block_sums(first, count)
    bad = np.nonzero(dev != host)[0]
    assert len(bad) == 0, f"{len(bad)} of {len(dev)} blocks of 2^20 values differ from libm's expf, first block {bad[0]} (bits {first + (int(bad[0]) << 20):#x} ..)"


# ---- update ------------------------------------------------------------------------------------------------------------------
N_UPDATE = 600
RANGES = [(0, 1), (599, 1), (255, 2), (3, 250), (0, 600)]
SUBSETS = {"all": MEMBERS, "means+opacity": ("means", "opacity_logits")}


def _fresh(count):
    return records(N_UPDATE, seed=11)[:count]


def _update(scene, first, new, members, **kw):
    d = to_device({k: v for k, v in cut(new).items() if k in members})
    scene.update_from_tensors(first, **d, **kw)


@pytest.mark.parametrize("subset", list(SUBSETS))
@pytest.mark.parametrize("first,count", RANGES)
def test_an_updated_scene_equals_the_scene_of_the_merged_records(pkg, gpu, _sort_path, first, count, subset):
    members = SUBSETS[subset]
    merged = merge(records(N_UPDATE), _fresh(count), first, members)
    want = reference(pkg, ("update", first, count, subset, _sort_path), lambda: merged)
    scene = pkg.Scene.from_records(records(N_UPDATE))
    rend = pkg.Renderer(scene)
    before = state(pkg, scene, rend=rend)
    assert not np.array_equal(before["blob"].view(np.uint32), want["blob"].view(np.uint32))
    rend.synchronize()
    _update(scene, first, _fresh(count), members)
    same_state(state(pkg, scene, rend=rend), want, f"[{first}, {first + count}) {subset}")


def test_update_argument_checks_and_no_ops(pkg, gpu, _sort_path):
    once(_sort_path)
    scene = pkg.Scene.from_records(records(N_UPDATE))
    before = raw_blob(scene)
    scene.update_from_tensors(0)                                           # no member
    _update(scene, N_UPDATE, _fresh(0), MEMBERS)                           # no rows, at the very end
    np.testing.assert_array_equal(raw_blob(scene).view(np.uint32), before.view(np.uint32))
    for first, count in ((N_UPDATE, 1), (N_UPDATE - 1, 2), (2 ** 64 - 1, 2), (1, N_UPDATE)):
        with pytest.raises(pkg.binding.GsError, match="out of bounds") as e:
            _update(scene, first, _fresh(count), MEMBERS)
        assert e.value.code == -1
    np.testing.assert_array_equal(raw_blob(scene).view(np.uint32), before.view(np.uint32))


def test_update_of_a_scene_with_a_copy_in_spatial_order(pkg, gpu, _sort_path, monkeypatch):
    """GS_SPATIAL_MIN=1 forces the second copy and `perm`: the update must reach the copy the frames read (cov3D lives in ITS
    order) while the order itself stays that of the positions the scene was built with."""
    monkeypatch.setenv("GS_SPATIAL_MIN", "1")
    first, count = 3, 250
    want = reference(pkg, ("update", first, count, "all", _sort_path), lambda: merge(records(N_UPDATE), _fresh(count), first))
    scene = pkg.Scene.from_records(records(N_UPDATE))
    rend = pkg.Renderer(scene)
    state(pkg, scene, rend=rend)
    rend.synchronize()
    _update(scene, first, _fresh(count), MEMBERS)
    same_state(state(pkg, scene, rend=rend), want, "spatial copy")


def test_update_of_a_quantised_scene_requantises(pkg, gpu, _sort_path):
    first, count = 3, 250
    want = reference(pkg, ("quantised", _sort_path), lambda: merge(records(N_UPDATE), _fresh(count), first), quantized=True)
    scene = pkg.Scene.from_records(records(N_UPDATE))
    scene.quantize_sh()
    rend = pkg.Renderer(scene)
    stale = state(pkg, scene, rend=rend)["image"]
    rend.synchronize()
    _update(scene, first, _fresh(count), MEMBERS)
    assert scene.sh_bits == 16
    got = state(pkg, scene, rend=rend)
    same_state(got, want, "quantised")
    assert not np.array_equal(got["image"], stale)


def test_an_update_that_removes_the_only_opacity_above_one_restores_the_guarded_blend(pkg, oracle, gpu, _sort_path):
    """A scene holding an opacity > 1 is blended with mode 2's arithmetic whatever the mode asked for; the flag is taken again
    by every update of the opacities."""
    n, at = 1200, 77
    r = records(n)
    verts = pkg.activate_records(r)
    verts[at, 7] = 2.0
    scene = pkg.Scene.from_vertices(verts)
    rend = pkg.Renderer(scene)
    u = pkg.camera_uniforms(pkg.make_camera(), W, H)
    rend.set_exp_mode(3)
    as3, _ = rend.render_host(u)
    rend.set_exp_mode(2)
    as2, _ = rend.render_host(u)
    assert np.array_equal(as3.view(np.uint32), as2.view(np.uint32))  # mode 3 ran as mode 2
    rend.synchronize()
    _update(scene, at, r[at:at + 1], MEMBERS)
    same(scene.download_vertices(), pkg.activate_records(r), "after the update")
    _, _, ref = oracle_frame(oracle, r, W, H)
    worst, redo, resolved = assert_guarded_close(rend, u, ref["image"], "guarded blend after the update")  # leaves mode 2
    exact, _ = rend.render_host(u)
    rend.set_exp_mode(3)
    guarded, _ = rend.render_host(u)
    st = rend.stats()
    print(f"mode 3 after the update: max|d| {worst:.3g}, blend_redo {st.blend_redo}, blend_resolved {st.blend_resolved}")
    assert (st.blend_redo, st.blend_resolved) == (redo, resolved)
    assert not np.array_equal(guarded.view(np.uint32), exact.view(np.uint32))  # v_exp_f32 is back: not libm's bits


# ---- frames ------------------------------------------------------------------------------------------------------------------
N_FRAME = 1200


def _moved(count=300):
    """Moved and re-coloured: new positions and SH, the rest kept."""
    return records(N_FRAME, seed=29)[:count], ("means", "sh_dc", "sh_rest")


def test_the_frame_of_the_arrays_scene_is_the_frame_of_the_records_scene(pkg, gpu, _sort_path):
    want = reference(pkg, ("frame", _sort_path), lambda: records(N_FRAME))
    scene = pkg.Scene.from_tensors(**to_device(cut(records(N_FRAME))))
    same_state(state(pkg, scene), want, "frame")
    assert want["visible"].sum() > N_FRAME // 2 and want["image"][..., :3].max() > 0.1


@pytest.mark.parametrize("mode", ["plain", "graph", "two_in_flight"])
def test_the_same_renderer_shows_the_updated_scene(pkg, gpu, _sort_path, mode):
    import torch
    first = 400
    new, members = _moved()
    want = reference(pkg, ("moved", _sort_path), lambda: merge(records(N_FRAME), new, first, members))
    scene = pkg.Scene.from_tensors(**to_device(cut(records(N_FRAME))))
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

    old = reference(pkg, ("frame", _sort_path), lambda: records(N_FRAME))["image"]
    for img in render():
        assert np.array_equal(img.view(np.uint32), old.view(np.uint32))
    _update(scene, first, new, members)  # (render() has synchronised the renderer)
    for img in render():
        assert np.array_equal(img.view(np.uint32), want["image"].view(np.uint32)), f"{mode}: the frame after the update is not the merged scene's"
    assert not np.array_equal(old, want["image"])
    same(scene.download_vertices(), want["vertices"], mode)
