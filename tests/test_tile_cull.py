"""The alpha-cut tile box (3dgs.cpp_amd/csrc/gs_tile_cull.h) on the CPU: the header compiled alone with g++, fed the attributes of
oracle.preprocess and the cut of oracle.alpha_cut.  Two properties: the tight box lies inside the reference box, and for EVERY
(tile, Gaussian) it drops no pixel of the tile passes render.comp:68/:78 with `power` in binary32 as the shader writes it
(tile_cull_reference.py).  And one figure: how much of S(1e6)'s instances it keeps at 1920 x 1080."""
import json
import os

import numpy as np
import pytest

import tile_cull_reference as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 320, 240


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    return tc.build_rule(tmp_path_factory.mktemp("tile_cull"))


def preprocess(oracle, records, width, height):
    verts = oracle.activate_records(records)
    u = oracle.camera_uniforms(oracle.default_camera(), width, height)
    return oracle.preprocess(verts, oracle.cov3d(verts), u)


def check_frame(rule, oracle, attr, tiles):
    ids, conic, uv, cut, ref = tc.frame_inputs(oracle, attr, tiles)
    tight = tc.tight_boxes(rule, conic, uv, cut, ref)
    tc.assert_contained(ref, tight)
    gi, tx, ty = tc.dropped_tiles(ref, tight)
    tc.assert_dropped_pairs_unused(conic, uv, cut, gi, tx, ty)
    return ids, ref, tight, cut, len(gi)


@pytest.mark.parametrize("kind", ["S", "T", "A"])
def test_scene_every_dropped_tile_is_unused(pkg, oracle, rule, kind):
    attr, tiles = preprocess(oracle, pkg.synth.synth_records(20000, seed=0, kind=kind), W, H)
    _, ref, tight, _, dropped = check_frame(rule, oracle, attr, tiles)
    assert len(ref) > 100 and dropped > 0  # the scene exercises the rule


def placed(pkg, pos, log_scale, quat=(1, 0, 0, 0), opacity=0.9):
    rec = pkg.synth.synth_records(1, seed=3)
    rec[0, 0:3] = pos
    rec[0, 55:58] = log_scale
    rec[0, 58:62] = quat
    rec[0, 54] = np.log(opacity / (1.0 - opacity))
    return rec


def placed_cases(pkg):
    ls = np.log
    s8, c8 = np.sin(np.pi / 8), np.cos(np.pi / 8)
    thin = [ls(0.6), ls(0.002), ls(0.002)]
    return {
        "needle_45": placed(pkg, (0, 0, -4), thin, (c8, 0, 0, s8)),
        "needle_135": placed(pkg, (0.1, -0.1, -4), thin, (c8, 0, 0, -s8)),
        "opacity_above_cut": placed(pkg, (0, 0, -4), [ls(0.05)] * 3, opacity=1 / 255 + 2e-5),
        "opacity_below_cut": placed(pkg, (0, 0, -4), [ls(0.05)] * 3, opacity=1 / 255 - 2e-5),
        "centre_off_screen": placed(pkg, (-1.8, 0.3, -4), [ls(0.15), ls(0.02), ls(0.02)]),
        "wider_than_a_bin": placed(pkg, (0, 0, -3), [ls(0.5)] * 3),
        "faint_and_wide": placed(pkg, (0.3, 0.2, -3), [ls(0.4)] * 3, opacity=0.006),
    }


def test_placed_cases(pkg, oracle, rule):
    for name, rec in placed_cases(pkg).items():
        attr, tiles = preprocess(oracle, rec, W, H)
        assert tiles[0] != 0, name
        _, ref, tight, cut, _ = check_frame(rule, oracle, attr, tiles)
        if name.startswith("needle"):
            assert tc.kept_instances(ref) >= 16 and tc.kept_instances(tight) < tc.kept_instances(ref), (name, ref, tight)
        if name == "opacity_below_cut":
            assert cut[0] == np.inf and (tight == 0).all()
        if name == "opacity_above_cut":
            assert np.isfinite(cut[0]) and cut[0] < 0 and tc.kept_instances(tight) <= 1  # (a centre between pixels: maybe none)
        if name == "centre_off_screen":
            assert attr["uv"][0, 0] < 0 and tc.kept_instances(ref) >= 1
        if name == "wider_than_a_bin":
            assert ref[0, 2] - ref[0, 0] > 8


def test_centre_on_a_tiles_first_and_last_pixel(pkg, oracle, rule):
    """uv exactly on pixel 32 (a tile's first) and 47 (its last), radii that reach one, two and many tiles: the attributes of a
    preprocessed splat with the centre and the box (preprocess.comp:160-165) replaced."""
    attr, tiles = preprocess(oracle, placed(pkg, (0, 0, -4), [np.log(0.03)] * 3), W, H)
    base = attr[np.nonzero(tiles)[0][:1]]
    rows = []
    for ux in (32.0, 47.0, 31.0, 48.0):
        for uy in (32.0, 47.0):
            for scale in (1.0, 0.25, 0.02):
                a = base.copy()
                a["uv"][0] = (ux, uy)
                a["conic_opacity"][0, :3] *= np.float32(scale)
                r = np.float32(np.ceil(3.0 * np.sqrt(1.0 / (a["conic_opacity"][0, 0]))))
                lo = lambda c: int(np.clip(int((np.float32(c) - r) / np.float32(16)), 0, None))  # noqa: E731
                hi = lambda c: int((np.float32(c) + r + np.float32(15)) / np.float32(16))  # noqa: E731
                a["aabb"][0] = (lo(ux), lo(uy), min(hi(ux), W // 16), min(hi(uy), H // 16))
                rows.append(a)
    attr2 = np.concatenate(rows)
    _, ref, tight, _, _ = check_frame(rule, oracle, attr2, np.ones(len(attr2), np.uint32))
    assert (tc.kept_per_box(tight) >= 1).all()  # the centre's own pixel keeps an opaque splat


def test_degenerate_conics_and_cuts_keep_the_reference_box(rule):
    ref = np.array([[1, 2, 9, 7]] * 8, np.int32)
    conic = np.array([[1, 1, 1], [1, 2, 1], [0, 0, 1], [-1, 0, -1], [np.nan, 0, 1], [1, 0, np.inf], [0.5, 0.1, 0.5], [0.5, 0.1, 0.5]], np.float32)
    cut = np.array([-5, -5, -5, -5, -5, -5, -np.inf, np.nan], np.float32)
    tight = tc.tight_boxes(rule, conic, np.full((8, 2), 80.0, np.float32), cut, ref)
    np.testing.assert_array_equal(tight, ref)
    # "never kept": +inf (and any positive cut) gives the empty box
    tight = tc.tight_boxes(rule, conic[6:], np.full((2, 2), 80.0, np.float32), np.array([np.inf, 1.0], np.float32), ref[:2])
    assert (tight == 0).all()


@pytest.mark.slow
def test_kept_fraction_of_config_b(pkg, oracle, rule):
    """S(1e6) at 1920 x 1080: a float64 rectangle without slack keeps 0.647 of the reference's 4 893 565 instances (measured on the
    reference's own boxes); the binary32 rule with its slack must stay at or below 0.66.  The figure found is kept in
    profiles/r19_tile_cull_kept.json (written when GS_WRITE_PROFILES is set)."""
    attr, tiles = preprocess(oracle, pkg.synth.synth_records(1000000, seed=0), 1920, 1080)
    _, conic, uv, cut, ref = tc.frame_inputs(oracle, attr, tiles)
    tight = tc.tight_boxes(rule, conic, uv, cut, ref)
    tc.assert_contained(ref, tight)
    d_ref, d_tight = tc.kept_instances(ref), tc.kept_instances(tight)
    kept = d_tight / d_ref
    print(f"S(1e6) 1920x1080: V {len(ref)} D reference {d_ref} D tight {d_tight} kept {kept:.4f}")
    if os.environ.get("GS_WRITE_PROFILES"):
        with open(os.path.join(ROOT, "profiles", "r19_tile_cull_kept.json"), "w") as f:
            json.dump({"scene": "S(1e6) seed 0, default camera, 1920x1080", "visible": len(ref), "instances_reference": d_ref,
                       "instances_tight": d_tight, "kept": round(kept, 4)}, f, indent=1)
            f.write("\n")
    assert d_ref == 4893565
    assert kept <= 0.66
