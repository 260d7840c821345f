"""The builders of tests/limit_scenes.py stand where they say: every pinned quantity, recomputed from the oracle's stages (tile
boxes, depth bits, ranges) and the bin geometry of gs_depth_policy.h, equals what the builder promises -- exactly, with no GPU.
This is what keeps tests/test_gpu_limits.py from passing while no longer on its edge."""
import numpy as np
import pytest

import limit_scenes as ls
from helpers import oracle_frame

LEVEL2_COUNTS = [lim + d for lim in ls.LEVEL_LIMITS for d in (-1, 0, 1)]


def _check(oracle, scene):
    verts, u, ref = oracle_frame(oracle, scene.records, scene.width, scene.height)
    got = ls.measure(scene, ref)
    for key, want in scene.expect.items():
        assert got[key] == want, f"{scene.name} ({scene.pins}): {key} is {got[key]}, the builder promises {want}"
    # every small splat covers one tile: the instance count is the candidate count wherever no probe is in the scene
    if "probes" not in scene.expect:
        assert len(ref["keys"]) == got["visible"]
    return got, ref


@pytest.mark.parametrize("count", LEVEL2_COUNTS)
def test_level2_size(oracle, count):
    sc = ls.level2_size(count)
    _check(oracle, sc)
    lv = [k for k, lim in enumerate(ls.LEVEL_LIMITS + (1 << 32,)) if count <= lim][0]
    p = ls.predict(sc)
    assert (p["sort_level"], p["retries"], p["bin_tiles"], p["max_bin_entries"]) == (lv, 1 if lv else 0, 4, count)
    assert ls.predict(sc, forced=True) == ("error" if count > 65535 else p)


def test_level2_size_that_refines(oracle):
    """16385 in a bin of 8 x 8 tiles on a frame whose bins can be halved: four bins of 4 x 4 tiles, the fullest holding 4097."""
    sc = ls.level2_size(16385, shift=3)
    assert ls.can_refine(sc.width, sc.height, 3) and not ls.can_refine(128, 128, 2)
    _check(oracle, sc)
    assert sc.expect["fullest_bin"] == {3: 16385, 2: 4097}
    p = ls.predict(sc)
    assert (p["sort_level"], p["retries"], p["bin_tiles"], p["max_bin_entries"]) == (3, 1, 4, 4097)


@pytest.mark.parametrize("slab", [False, True], ids=["fast", "slab"])
@pytest.mark.parametrize("place", ls.RUN_PLACES)
@pytest.mark.parametrize("length", [64, 65, 66, 67])
def test_equal_run(oracle, length, place, slab):
    sc = ls.equal_run(length, place, slab)
    got, _ = _check(oracle, sc)
    assert got["longest_run"] == length
    if place == "straddle":
        assert got["run_start"] < ls.THREADS <= got["run_start"] + length - 1
    p = ls.predict(sc)
    if not slab:
        assert (p["sort_level"], p["retries"]) == (0, 0)
    else:
        assert (p["sort_level"], p["retries"]) == ((4, 1) if length <= ls.TIE_RUN_MAX else (5, 2))
        assert (ls.predict(sc, forced=True) == "error") == (length > ls.TIE_RUN_MAX)


@pytest.mark.parametrize("k", [63, 64, 65, 66])
def test_crowded_bucket(oracle, k):
    sc = ls.crowded_bucket(k)
    got, _ = _check(oracle, sc)
    assert got["fullest_bucket"] == k and (k > ls.MSD_BUCKET_MAX) == (k >= 65)
    assert ls.predict(sc)["sort_level"] == 0   # k_bin_fast<4>: the level whose order starts with the buckets


@pytest.mark.parametrize("kind", ["exact", "over", "most"])
def test_slab_plan(oracle, kind):
    sc = ls.slab_plan(kind)
    got, _ = _check(oracle, sc)
    sizes = got["slab_sizes"]
    assert max(sizes) <= ls.SLAB_MAX and sum(sizes) == sc.expect["fullest_bin"][2]
    assert {"exact": sizes[0] == 12288, "over": sizes[0] == 12287, "most": len(sizes) == 11}[kind]
    assert 16384 < sum(sizes) <= 65535 and ls.predict(sc)["sort_level"] == 4


def test_no_bin_of_a_frame_needs_more_than_eleven_slabs():
    """Why kMaxSlabs = 16 has no scene: the planner closes a slab only in front of a bucket that would take it beyond 12288, so
    slabs 1 + 2, 3 + 4, ... each hold more than 12288 between them and n slabs need more than floor(n / 2) x 12288 candidates.
    Eleven fit a bin of <= 65535 (buckets of 1 and 12288 in turn: 61446); a twelfth slab needs a sixth such pair, more than
    73728.  Checked against the restated planner on the extreme histograms."""
    worst = np.zeros(ls.MSD_BUCKETS, np.int64)
    worst[:11] = [1, 12288] * 5 + [1]
    assert len(ls.plan_slabs(worst)) == 11 and worst.sum() == 61446
    worst[11] = 12288                                  # the cheapest twelfth slab: the bin no longer fits level 4
    assert len(ls.plan_slabs(worst)) == 12 and worst.sum() > 65535
    # no histogram of <= 65535 does better: a pair of neighbouring slabs below 12289 would have been one slab
    for first in (1, 12288):
        h = np.zeros(ls.MSD_BUCKETS, np.int64)
        h[:12] = [first, 12289 - first] * 6
        assert len(ls.plan_slabs(h)) == 12 and h.sum() == 6 * 12289 > 65535


@pytest.mark.parametrize("n,culled", [(1023, 0), (1024, 0), (1025, 0), (1023, 300), (1024, 300), (1025, 300)])
def test_level1_count(oracle, n, culled):
    sc = ls.level1_count(n, culled)
    got, _ = _check(oracle, sc)
    assert got["visible"] == n and got["n"] == n + culled


@pytest.mark.parametrize("blocks", [31, 32, 33, 255, 256, 257])
def test_level1_blocks(oracle, blocks):
    sc = ls.level1_blocks(blocks)
    got, _ = _check(oracle, sc)
    assert got["l1_blocks"] == blocks and got["n"] == 1024 * blocks - 1


@pytest.mark.parametrize("rows,cols", ls.BIG_BOXES)
def test_big_box(oracle, rows, cols):
    sc = ls.big_box(rows, cols)
    got, _ = _check(oracle, sc)
    assert all(bx * by == rows * cols for bx, by in got["probes"].values())
    assert (rows * cols > ls.L1_BIG_BOX) == (rows * cols >= 13)
    assert got["largest_other_box"] == 1


@pytest.mark.parametrize("k", ls.BLEND_LENGTHS)
def test_blend_chunk(oracle, k):
    sc = ls.blend_chunk(k)
    got, ref = _check(oracle, sc)
    assert got["tile_lists"][(2, 1)] == k and len(got["tile_lists"]) == 2
    # weak opacities: no pixel's transmittance comes near the 1e-4 cut, so no pixel stops before the end of its list
    a = ref["attr"]["conic_opacity"][:, 3].astype(np.float64)
    assert a.max() < 0.0201 and (1.0 - a.max()) ** max(got["tile_lists"].values()) > 1e-3
    assert (ref["image"][..., :3] != 0).any()


# ------------------------------------------------------------------------------------------------ guard triggers
def _image_of(oracle):
    return lambda rec: oracle_frame(oracle, rec, ls.GUARD_FRAME, ls.GUARD_FRAME)[2]["image"]


def _check_tuned(oracle, sc):
    """The tuned layers stand one binary32 step of their logit from the cut: the reference breaks at every site as built, and at
    none with each last layer one step weaker; every entry of the tile is kept at its own site's pixel (alpha >= 1/255 there)."""
    got, ref = _check(oracle, sc)
    g = sc.guard
    assert ls.breaks_at(ref["image"], g["sites"]).all()
    weaker, _ = ls._stacks(g["sites"], g["layers"], g["final_bits"] - 1)
    assert not ls.breaks_at(_image_of(oracle)(weaker), g["sites"]).any()
    a = ref["attr"]
    uv = np.round(a["uv"]).astype(int)
    assert {tuple(p) for p in uv.tolist()} == set(g["sites"]) and np.abs(a["uv"] - uv).max() < 1e-3
    assert (a["conic_opacity"][:, 3] >= 1.0 / 255.0).all()
    return got


@pytest.mark.parametrize("kept", [384, 385])
def test_guard_list(oracle, kept):
    sc = ls.guard_list(kept, _image_of(oracle))
    got = _check_tuned(oracle, sc)
    assert got["tile_lists"] == {(1, 1): kept} and sc.guard["want"] == ("resolved" if kept == 384 else "redo")


@pytest.mark.parametrize("count", [8, 9])
def test_guard_resolves(oracle, count):
    sc = ls.guard_resolves(count, _image_of(oracle))
    got = _check_tuned(oracle, sc)
    assert len(sc.guard["sites"]) == count and got["tile_lists"] == {(1, 1): 40 * count} and 40 * count <= ls.GUARD_LIST
    xs = np.asarray(sc.guard["sites"])
    assert (xs >= 24).all() and (xs < 32).all()          # one quadrant of tile (1, 1)


@pytest.mark.parametrize("kept", [4095, 4096, 4097])
def test_guard_pairs(oracle, kept):
    sc = ls.guard_pairs(kept)
    got, ref = _check(oracle, sc)
    assert got["tile_lists"] == {(1, 1): kept} and sc.guard["want"] == ("clean" if kept <= 4096 else "redo")
    # a pixel two or more away from the splats never blends anything: it is what keeps the quadrant walking to the list's end
    assert not ref["image"][24, 24, :3].any() and ref["image"][27, 27, :3].any()
