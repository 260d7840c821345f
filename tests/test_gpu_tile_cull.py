"""The alpha-cut tile cull (gs_set_tile_cull; csrc/gs_tile_cull.h): on the frames of the one-pass level 1 that k_bin_fast orders, the
lists the blend walks are made from the tiles the alpha-cut ellipse's bounding rectangle touches.  It may change nothing a consumer
sees: the exp-mode-2 image bit for bit (on, off and the checker's), the reference list taps (11 .. 15) and every statistic equal with
the cull on and off, before and after a list-buffer overflow; contributions, feature maps and the lift exactly equal.  And what it
does change is pinned: every tile's culled list (taps 16 / 17) is an order-preserving subsequence of its reference list, and every
(tile, entry) left out has no pixel that passes render.comp:68/:78 in the shader's own binary32 (tile_cull_reference.py).

Every test runs under both depth-order settings of the suite (conftest.py): on the global path no frame is culled, which is then
what the getter says and the test checks."""
import numpy as np
import pytest
import torch  # at collection, before the package loads its library: both must bind the same HIP runtime

import tile_cull_reference as tc
from helpers import GUARD_TOL, assert_guarded_close, compare_stages, oracle_frame

pytestmark = pytest.mark.gpu

W, H = 320, 240
STATS = ("num_visible", "num_instances", "num_bin_entries", "max_bin_entries", "sort_level", "retries", "bin_tiles", "instance_capacity")
# (name, Gaussians, kind, width, height, GS_BIN_SHIFT or None)
SCENES = [
    ("S", 20000, "S", W, H, None),
    ("T", 20000, "T", W, H, None),
    ("bins_of_4x4_tiles", 20000, "S", W, H, 2),
    # one bin of 8 x 8 tiles holding more candidates than the largest in-LDS order (16384): the renderer re-runs with bins of 4 x 4
    ("fullest_bin_forces_4x4", 40000, "A", 128, 128, None),
    # one bin of 4 x 4 tiles that cannot be refined and holds more than 16384 candidates: the slab level orders it, from the
    # records' reference halves -- a one-pass frame that is NOT culled
    ("slab_level_is_not_culled", 40000, "A", 64, 64, 2),
]


def _setup(pkg, oracle, monkeypatch, case):
    name, n, kind, w, h, shift = case
    monkeypatch.setenv("GS_SPATIAL_MIN", "0")
    if shift is not None:
        monkeypatch.setenv("GS_BIN_SHIFT", str(shift))
    rec = pkg.synth.synth_records(n, seed=0, kind=kind)
    verts, u_ref, ref = oracle_frame(oracle, rec, w, h)
    scene = pkg.Scene.from_records(rec, device=0)
    rend = pkg.Renderer(scene)
    rend.set_level1_fused(1)  # small scenes take the one-pass level 1
    u = pkg.camera_uniforms(pkg.make_camera(), w, h)
    assert u.tobytes() == u_ref.tobytes()
    return rec, ref, scene, rend, u


def _frame(rend, u, on):
    rend.set_tile_cull(on)
    rend.set_exp_mode(2)
    img, _ = rend.render_host(u)
    st = rend.stats()
    return img, {k: getattr(st, k) for k in STATS}, rend.tile_cull()


def _tile_keys(lists, ranges, n):
    """tile * n + id of every entry of lists laid end to end in tile order (ranges: [T, 2])."""
    lens = (ranges[:, 1] - ranges[:, 0]).astype(np.int64)
    assert int(lens.sum()) == len(lists)
    return np.repeat(np.arange(len(ranges), dtype=np.int64), lens) * n + lists.astype(np.int64)


def _check_culled_lists(oracle, rend, u, ref, n, w):
    """Taps 16 / 17 against the reference's lists: order-preserving subsequences, and every dropped (tile, entry) unused."""
    ranges = ref["boundaries"].reshape(-1, 2).astype(np.int64)
    ref_keys = _tile_keys(ref["sorted_payload"], ranges, n)
    c_ranges = rend.stage("ranges_culled", u).reshape(-1, 2).astype(np.int64)
    c_lists = rend.stage("lists_culled")
    listed = rend.listed_instances()
    assert len(c_lists) == listed == int((c_ranges[:, 1] - c_ranges[:, 0]).sum())
    got_keys = _tile_keys(c_lists, c_ranges, n)
    kept = np.isin(ref_keys, got_keys)  # (an id occurs once in a tile's list: the keys are unique)
    np.testing.assert_array_equal(got_keys, ref_keys[kept])
    dropped = ref_keys[~kept]
    gid, tile = dropped % n, dropped // n
    tx = (w + 15) // 16
    attr = ref["attr"]
    cut = oracle.alpha_cut(attr["conic_opacity"][:, 3])
    checked = tc.assert_dropped_pairs_unused(attr["conic_opacity"][:, :3], attr["uv"], cut, gid, tile % tx, tile // tx)
    assert checked == len(ref_keys) - listed
    return listed, len(ref_keys)


def _check_raw_taps(rend, u, ref, n):
    """Taps 14 / 15: each tile's slice of the raw lists is the reference's list of that tile, and the slices do not overlap."""
    raw = rend.stage("lists_raw")
    rr = rend.stage("ranges_raw", u).reshape(-1, 2).astype(np.int64)
    ranges = ref["boundaries"].reshape(-1, 2).astype(np.int64)
    lens = rr[:, 1] - rr[:, 0]
    np.testing.assert_array_equal(lens, ranges[:, 1] - ranges[:, 0])
    assert int(lens.sum()) == len(raw) == len(ref["sorted_payload"])
    order = np.argsort(rr[:, 0], kind="stable")
    nz = order[lens[order] > 0]
    assert (rr[nz[1:], 0] >= rr[nz[:-1], 1]).all() and (len(nz) == 0 or rr[nz[-1], 1] <= len(raw))
    idx = np.concatenate([np.arange(a, b) for a, b in rr]) if len(raw) else np.zeros(0, np.int64)
    np.testing.assert_array_equal(raw[idx], ref["sorted_payload"])


@pytest.mark.parametrize("case", SCENES, ids=[c[0] for c in SCENES])
def test_cull_changes_no_output(pkg, oracle, gpu, monkeypatch, _sort_path, case):
    name, n, kind, w, h, shift = case
    rec, ref, scene, rend, u = _setup(pkg, oracle, monkeypatch, case)
    try:
        img_on, st_on, (switch, culled) = _frame(rend, u, True)
        assert switch
        fused, sort_level = rend.level1_fused(), st_on["sort_level"]
        assert fused == (_sort_path != "1")
        assert culled == (fused and sort_level < 4), "culled exactly on the one-pass frames that k_bin_fast orders"
        if name == "fullest_bin_forces_4x4" and _sort_path != "1":
            assert st_on["bin_tiles"] == 4 and st_on["retries"] >= 1 and culled
        if shift == 2 and _sort_path != "1":
            assert st_on["bin_tiles"] == 4
        if name == "slab_level_is_not_culled" and _sort_path != "1":
            assert fused and sort_level == 4 and not culled
        np.testing.assert_array_equal(img_on.view(np.uint32), ref["image"].view(np.uint32))
        # the reference taps, twice (the second answer comes from the taps' kept buffers), and the raw pair
        compare_stages(pkg, rend, u, ref)
        compare_stages(pkg, rend, u, ref)
        _check_raw_taps(rend, u, ref, n)
        listed, d = _check_culled_lists(oracle, rend, u, ref, n, w)
        assert d == st_on["num_instances"]
        if culled:
            assert listed < d, "the cull dropped nothing"
        else:
            assert listed == d
        print(f"{name}: sort path {_sort_path} culled {culled} level {sort_level} bins of {st_on['bin_tiles']} tiles: D {d} listed {listed} "
              f"({listed / max(d, 1):.3f})")
        # the guarded blend, cull on
        worst_on, _, _ = assert_guarded_close(rend, u, ref["image"], f"{name} cull on")
        rend.set_exp_mode(3)
        img3_on, _ = rend.render_host(u)

        img_off, st_off, (switch, culled_off) = _frame(rend, u, False)
        assert not switch and not culled_off
        assert st_off == st_on
        np.testing.assert_array_equal(img_off.view(np.uint32), img_on.view(np.uint32))
        compare_stages(pkg, rend, u, ref)
        _check_raw_taps(rend, u, ref, n)
        np.testing.assert_array_equal(rend.stage("lists_culled"), ref["sorted_payload"])
        np.testing.assert_array_equal(rend.stage("ranges_culled", u), ref["boundaries"])
        assert rend.listed_instances() == d
        worst_off, _, _ = assert_guarded_close(rend, u, ref["image"], f"{name} cull off")
        rend.set_exp_mode(3)
        img3_off, _ = rend.render_host(u)
        same3 = np.array_equal(img3_on.view(np.uint32), img3_off.view(np.uint32))
        d3 = float(np.abs(img3_on.astype(np.float64) - img3_off).max())
        # (a quadrant the guard abandons is re-rendered whole: with other lists it may be another quadrant, within the tolerance)
        print(f"{name}: exp mode 3 on / off bit-identical {same3} (max |d| {d3:.3g}); against the checker {worst_on:.3g} / {worst_off:.3g}")
        assert d3 <= 2 * GUARD_TOL
    finally:
        rend.close()
        scene.close()


@pytest.mark.parametrize("case", SCENES[:3], ids=[c[0] for c in SCENES[:3]])
def test_passes_over_culled_lists(pkg, oracle, gpu, monkeypatch, _sort_path, case):
    """Contributions, feature maps and the lift walk the culled lists as they are: exactly what they give over the reference's."""
    name, n, kind, w, h, shift = case
    rec, ref, scene, rend, u = _setup(pkg, oracle, monkeypatch, case)
    rng = np.random.default_rng(5)
    feats = torch.from_numpy(rng.standard_normal((n, 3)).astype(np.float32)).cuda()
    vals = torch.from_numpy(rng.integers(-1, 2, (h, w, 2)).astype(np.float32)).cuda()
    # The lift adds in an unspecified order.  Counted on one pixel in 32 x 32 a Gaussian's sums stay exact in binary64 whatever the
    # order -- every term is +-w or 0 with w = fl32(alpha T) in [2^-22, 1), a multiple of 2^-45, and at most 255 of them (asserted
    # below) stay below 2^8: 53 bits hold every partial sum -- so on and off compare bit for bit.  (The contributions, integer
    # sums over EVERY pixel of the same walk, compare exactly as they are.)
    sparse = np.zeros((h, w), np.uint8)
    sparse[5::32, 9::32] = 1
    sparse_t = torch.from_numpy(sparse).cuda()
    got = {}
    try:
        for on in (True, False):
            _frame(rend, u, on)
            assert rend.tile_cull()[1] == (on and _sort_path != "1")
            wt = torch.zeros(n, dtype=torch.int64, device="cuda")
            px = torch.zeros(n, dtype=torch.int32, device="cuda")
            top = torch.zeros((h, w), dtype=torch.int32, device="cuda")
            rend.contributions(weight=wt, pixels=px, top_id=top)
            spx = torch.zeros(n, dtype=torch.int32, device="cuda")
            rend.contributions(pixels=spx, mask=sparse_t)
            assert int(spx.max()) <= 255
            fm = rend.feature_maps(features=feats, out=True, alpha=True, depth=True, median_depth=True)
            lift = rend.lift_pixels(vals, out=True, weight=True, mask=sparse_t)
            got[on] = dict(weight=wt, pixels=px, top_id=top, lift_out=lift["out"], lift_weight=lift["weight"], **{"fm_" + k: v for k, v in fm.items()})
            got[on] = {k: v.cpu().numpy() for k, v in got[on].items()}
        assert got[True]["pixels"].sum() > 0
        for k in got[True]:
            a, b = got[True][k], got[False][k]
            np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8), err_msg=k)
    finally:
        rend.close()
        scene.close()


def test_list_buffer_overflow_equal_on_and_off(pkg, oracle, gpu, monkeypatch, _sort_path):
    """The per-tile lists start one entry short of the REFERENCE's D (as tests/test_gpu_l1_one_pass.py provokes it): the frame
    overflows on the reference cursor and is re-run once, whether the cull is on -- its lists would have fitted -- or off."""
    monkeypatch.setenv("GS_SPATIAL_MIN", "0")
    rec = pkg.synth.synth_records(2000, seed=2000, kind="A")
    w = h = 64
    verts, u_ref, ref = oracle_frame(oracle, rec, w, h)
    u = pkg.camera_uniforms(pkg.make_camera(), w, h)
    d = len(ref["sorted_payload"])
    monkeypatch.setenv("GS_INITIAL_CAPACITY", str(d - 1))
    stats = {}
    for on in (True, False):
        scene = pkg.Scene.from_records(rec, device=0)
        rend = pkg.Renderer(scene)
        rend.set_level1_fused(1)
        try:
            for frame in range(2):
                img, st, (_, culled) = _frame(rend, u, on)
                assert culled == (on and _sort_path != "1")
                assert st["num_instances"] == d and st["retries"] >= 1
                if _sort_path != "1":
                    assert st["retries"] == 1 and rend.level1_fused()
                    if on:
                        assert rend.listed_instances() < d - 1, "the culled lists alone would have fitted: the reference cursor raised the overflow"
                np.testing.assert_array_equal(img.view(np.uint32), ref["image"].view(np.uint32))
                compare_stages(pkg, rend, u, ref)
                stats[(on, frame)] = st
        finally:
            rend.close()
            scene.close()
    for frame in range(2):
        assert stats[(True, frame)] == stats[(False, frame)]
