"""The export on the device (gs_scene_to_device_arrays, gs_scene_download_records, gs_scene_save_ply) must be BIT FOR BIT the
host's gs_deactivate_vertices of what the scene holds -- which tests/test_scene_export_api.py holds to the numpy restatement
of the rule -- and a scene that goes out and comes back must be the scene it was: positions, scales, opacities and SH in their
bits, rotations within the bound a second normalisation allows (export_reference.ROTATION_BOUND; derived in
test_scene_export_api.py).  "Equal" is bitwise wherever the host value is not a NaN, and a NaN where it is.
"""
import functools
import os

import numpy as np
import pytest

import export_reference as ref
from test_gpu_device_arrays import cut, raw_blob, to_device

pytestmark = pytest.mark.gpu

BLOCK = 256  # Gaussians per workgroup of k_scene_export
W, H = 128, 96
MEMBERS = dict(means=(3,), log_scales=(3,), quats=(4,), opacity_logits=(), sh_dc=(3,), sh_rest=(15, 3))
GUARD = -7.25


@functools.lru_cache(maxsize=None)
def records(n, seed=3):
    import __graft_entry__ as entry
    r = entry.load_package().synth.synth_records(n, seed=seed, kind="A")
    r.setflags(write=False)
    return r


def once(_sort_path):
    if _sort_path == "1":
        pytest.skip("independent of the depth-order path: runs once")


def members_of(rec, k=15):
    """The six arrays of (n, 62) records as to_tensors lays them out, sh_rest cut to k coefficients."""
    a = cut(rec)
    a["sh_rest"] = np.ascontiguousarray(a["sh_rest"][:, :k, :])
    return a


def host_records(pkg, scene, first=0, count=None):
    count = scene.num_vertices - first if count is None else count
    return pkg.deactivate_vertices(scene.download_vertex_range(first, count))


def same_tensors(got, want_rec, label, k=15):
    want = members_of(want_rec, k)
    assert set(got) == set(want), label
    for name, w in want.items():
        g = got[name].cpu().numpy()
        assert g.shape == w.shape, (label, name, g.shape, w.shape)
        ref.same_bits(g, w, f"{label}: {name}")


# ---- the device against the host ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK + 7])
def test_the_device_export_equals_the_hosts(pkg, gpu, _sort_path, n):
    once(_sort_path)
    scene = pkg.Scene.from_records(records(n))
    before = raw_blob(scene)
    want = host_records(pkg, scene)
    ref.same_bits(scene.download_records(), want, f"n={n}: download_records")
    same_tensors(scene.to_tensors(), want, f"n={n}: to_tensors")
    assert np.array_equal(raw_blob(scene).view(np.uint32), before.view(np.uint32)), "the export changed the scene"


@pytest.mark.parametrize("first,count", [(3, 250), (200, 3 * BLOCK + 7 - 200 - 5), (BLOCK, BLOCK + 9), (3 * BLOCK + 6, 1), (40, 0)])
def test_ranges_that_start_inside_the_scene_and_end_inside_a_block(pkg, gpu, _sort_path, first, count):
    once(_sort_path)
    scene = pkg.Scene.from_records(records(3 * BLOCK + 7))
    want = host_records(pkg, scene, first, count)
    ref.same_bits(scene.download_records(first, count), want, "download_records")
    for degree, k in pkg.binding.SH_REST_COEFFS.items():
        same_tensors(scene.to_tensors(first, count, sh_degree=degree), want, f"[{first}, {first + count}) degree {degree}", k)


def guarded(shape):
    """(a destination one float into a larger allocation -- 4-byte aligned and no more --, the allocation)."""
    import torch
    numel = int(np.prod(shape))
    big = torch.full((numel + 64,), GUARD, dtype=torch.float32, device="cuda")
    d = big[1:1 + numel].view(shape)
    assert d.data_ptr() % 16 == 4 and d.is_contiguous()
    return d, big


def guards_intact(big, numel):
    host = big.cpu().numpy()
    return host[0] == GUARD and (host[1 + numel:] == GUARD).all()


@pytest.mark.parametrize("first,count", [(0, 3 * BLOCK + 7), (5, BLOCK + 2)])
def test_each_member_alone_into_an_offset_slice_leaves_its_guards(pkg, gpu, _sort_path, first, count):
    once(_sort_path)
    scene = pkg.Scene.from_records(records(3 * BLOCK + 7))
    before = raw_blob(scene)
    want_rec = host_records(pkg, scene, first, count)
    cases = [(name, trailing, 15) for name, trailing in MEMBERS.items()] + [("sh_rest", (8, 3), 8), ("sh_rest", (3, 3), 3)]
    for name, trailing, k in cases:
        d, big = guarded((count,) + trailing)
        out = scene.to_tensors(first, count, out={name: d})
        assert set(out) == {name}
        ref.same_bits(d.cpu().numpy(), members_of(want_rec, k)[name], f"{name} alone")
        assert guards_intact(big, d.numel()), f"{name} alone: a float outside the destination changed"
    # all six at once, every one offset
    dests = {name: guarded((count,) + trailing) for name, trailing in MEMBERS.items()}
    scene.to_tensors(first, count, out={name: d for name, (d, _) in dests.items()})
    for name, (d, big) in dests.items():
        ref.same_bits(d.cpu().numpy(), members_of(want_rec)[name], f"{name} among six")
        assert guards_intact(big, d.numel()), f"{name} among six: a float outside the destination changed"
    assert np.array_equal(raw_blob(scene).view(np.uint32), before.view(np.uint32)), "the export changed the scene"


def test_out_of_range_exports_are_refused(pkg, gpu, _sort_path):
    once(_sort_path)
    n = 300
    scene = pkg.Scene.from_records(records(n))
    for first, count in ((n, 1), (n - 1, 2), (2 ** 64 - 1, 2), (1, n)):
        with pytest.raises(pkg.binding.GsError, match="out of bounds") as e:
            scene.download_records(first, count)
        assert e.value.code == -1
        with pytest.raises(pkg.binding.GsError, match="out of bounds"):
            scene.to_tensors(first, count, out={})
    assert scene.download_records(n, 0).shape == (0, 62)


# ---- pattern sweep -----------------------------------------------------------------------------------------------------------
def test_the_device_inverse_equals_the_hosts_on_a_sweep_of_bit_patterns(pkg, gpu, _sort_path):
    """2^20 binary32 patterns j * 4099 mod 2^32 -- every exponent, both signs, NaNs, subnormals -- in the three scale planes and
    the opacity plane of a scene of 2^18 Gaussians."""
    once(_sort_path)
    n = 1 << 18
    patterns = ((np.arange(1 << 20, dtype=np.uint64) * 4099) & 0xFFFFFFFF).astype(np.uint32).view(np.float32).reshape(n, 4)
    v = np.zeros((n, 60), np.float32)
    v[:, 0:3] = np.random.default_rng(31).standard_normal((n, 3)).astype(np.float32)
    v[:, 3] = 1.0
    v[:, 8] = 1.0
    v[:, 4:8] = patterns
    scene = pkg.Scene.from_vertices(v)
    stored = scene.download_vertices()
    assert np.array_equal(stored.view(np.uint32), v.view(np.uint32)), "from_vertices does not store the patterns verbatim"
    want = pkg.deactivate_vertices(v)
    got = scene.to_tensors(sh_degree=0)
    ref.same_bits(got["log_scales"].cpu().numpy(), want[:, 55:58], "log_scales over the sweep")
    ref.same_bits(got["opacity_logits"].cpu().numpy(), want[:, 54], "opacity_logits over the sweep")
    assert np.isnan(want[:, 54:58]).any() and np.isfinite(want[:, 54:58]).any() and np.isinf(want[:, 55:58]).any()


# ---- round trips -------------------------------------------------------------------------------------------------------------
N_TRIP = 1200
NOT_ROTATION = [k for k in range(60) if not 8 <= k < 12]


def same_gaussians(pkg, got_vertices, want_vertices, label, images=True):
    """The rules of a round trip: every float but the rotation in its bits (scales that are no images of exp: the nearest
    image, which is what the host's rule gives), the rotation within the bound."""
    keep = NOT_ROTATION if images else [k for k in NOT_ROTATION if not 4 <= k < 7]
    ref.same_bits(got_vertices[:, keep], want_vertices[:, keep], label)
    ref.rotations_within_bound(got_vertices[:, 8:12], want_vertices[:, 8:12], f"{label}: rotations")
    if not images:
        s = want_vertices[:, 4:7].reshape(-1)
        x = ref.log_scales(pkg, s)
        ref.same_bits(got_vertices[:, 4:7].reshape(-1), ref._activated(pkg, 55, 4, x), f"{label}: scales are the rule's images")
        err = lambda c: np.abs(ref._activated(pkg, 55, 4, c).astype(np.float64) - s.astype(np.float64))  # noqa: E731
        assert (err(x) <= err(ref.neighbour(x, 1))).all() and (err(x) <= err(ref.neighbour(x, -1))).all(), f"{label}: not the nearest image"


def round_trip(pkg, scene, label, images=True):
    back = pkg.Scene.from_tensors(**scene.to_tensors())
    assert back.num_vertices == scene.num_vertices
    same_gaussians(pkg, back.download_vertices(), scene.download_vertices(), label, images)
    a, b = raw_blob(back), raw_blob(scene)
    st = (scene.num_vertices + 15) & ~15
    rot = np.zeros(len(a), bool)
    rot[6 * st:10 * st] = True
    if not images:
        rot[3 * st:6 * st] = True  # (the scale planes: checked above)
    ref.same_bits(a[~rot], b[~rot], f"{label}: the blob outside the rotation planes")
    return back


def test_a_scene_exported_and_rebuilt_is_the_same_scene(pkg, gpu, _sort_path):
    once(_sort_path)
    scene = pkg.Scene.from_records(records(N_TRIP))
    round_trip(pkg, scene, "from_records")
    scene.transform(rotation=(0.9, 0.1, -0.3, 0.2), translation=(0.5, -1.0, 2.0), scale=1.7)
    round_trip(pkg, scene, "after a transform", images=False)


def test_a_scene_with_a_copy_in_spatial_order_exports_in_id_order(pkg, gpu, _sort_path, monkeypatch):
    once(_sort_path)
    plain = pkg.Scene.from_records(records(N_TRIP)).download_records()
    monkeypatch.setenv("GS_SPATIAL_MIN", "0")
    scene = pkg.Scene.from_records(records(N_TRIP))
    ref.same_bits(scene.download_records(), plain, "download_records of a scene with a spatial copy")
    round_trip(pkg, scene, "spatial copy")


def test_a_quantised_scene_exports_its_fp32_block(pkg, gpu, _sort_path):
    once(_sort_path)
    plain = pkg.Scene.from_records(records(N_TRIP)).download_records()
    scene = pkg.Scene.from_records(records(N_TRIP))
    scene.quantize_sh()
    assert scene.sh_bits == 16
    ref.same_bits(scene.download_records(), plain, "download_records of a quantised scene")
    round_trip(pkg, scene, "quantised")


# ---- save_ply ----------------------------------------------------------------------------------------------------------------
def test_save_ply_writes_what_write_ply_writes_and_loads_as_the_same_scene(pkg, gpu, _sort_path, tmp_path, monkeypatch):
    """Chunks of 500 records: n = 1200 spans three, the last one partial."""
    scene = pkg.Scene.from_records(records(N_TRIP))
    rec = scene.download_records()
    monkeypatch.setenv("GS_EXPORT_CHUNK", "500")
    ref.same_bits(scene.download_records(), rec, "download_records in three chunks")
    ref.same_bits(scene.download_records(7, 1001), rec[7:1008], "a range in three chunks")
    saved, written = tmp_path / "saved.ply", tmp_path / "written.ply"
    scene.save_ply(saved)
    pkg.write_ply(written, rec)
    with open(saved, "rb") as f, open(written, "rb") as g:
        assert f.read() == g.read(), "save_ply and write_ply(download_records()) differ in their bytes"
    loaded, rebuilt = pkg.Scene.load_ply(saved), pkg.Scene.from_records(rec)
    u = pkg.camera_uniforms(pkg.make_camera(), W, H)
    frames = []
    for s in (loaded, rebuilt):
        rend = pkg.Renderer(s)
        rend.set_exp_mode(2)
        frames.append(rend.render_host(u)[0])
        rend.close()
    for name, a, b in (("vertices", loaded.download_vertices(), rebuilt.download_vertices()),
                       ("cov3d", loaded.download_cov3d(), rebuilt.download_cov3d()), ("blob", raw_blob(loaded), raw_blob(rebuilt))):
        ref.same_bits(a, b, f"the loaded scene's {name}")
    assert np.array_equal(frames[0].view(np.uint32), frames[1].view(np.uint32)) and frames[0][..., :3].max() > 0.1
    same_gaussians(pkg, loaded.download_vertices(), scene.download_vertices(), "saved and reloaded")
    with pytest.raises(pkg.binding.GsError) as e:
        scene.save_ply(tmp_path / "no_such_directory" / "out.ply")
    assert e.value.code == -2 and not os.path.exists(tmp_path / "no_such_directory")


# ---- composition -------------------------------------------------------------------------------------------------------------
def test_two_exports_concatenated_build_the_scene_of_both(pkg, gpu, _sort_path):
    once(_sort_path)
    import torch
    a, b = pkg.Scene.from_records(records(700)), pkg.Scene.from_records(records(500, seed=11))
    ta, tb = a.to_tensors(), b.to_tensors()
    both = pkg.Scene.from_tensors(**{k: torch.cat([ta[k], tb[k]]).contiguous() for k in ta})
    assert both.num_vertices == 1200
    want = np.concatenate([a.download_vertices(), b.download_vertices()])
    same_gaussians(pkg, both.download_vertices(), want, "Gaussian i of the concatenation")
