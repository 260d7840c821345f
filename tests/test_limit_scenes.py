"""The builders of tests/limit_scenes.py stand where they say: every pinned quantity, recomputed from the oracle's stages (tile
boxes, depth bits, ranges) and the bin geometry of gs_depth_policy.h, equals what the builder promises -- exactly, with no GPU.
This is what keeps tests/test_gpu_limits.py from passing while no longer on its edge.

Also here, because the wave patterns in spatial order rest on it: the spatial read order of gs_host_math.h's spatial_order (driven through
tests/native/spatial_order_sim.cpp) against its numpy restatement limit_scenes.morton_order, exactly."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import float64_check as chk
import limit_scenes as ls
from float64_cases import Frame
from helpers import oracle_frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "3dgs.cpp_amd", "csrc")

LEVEL2_COUNTS = [lim + d for lim in ls.LEVEL_LIMITS for d in (-1, 0, 1)]


def _check(oracle, scene):
    verts, u, ref = oracle_frame(oracle, scene.records, scene.width, scene.height)
    got = ls.measure(scene, ref)
    for key, want in scene.expect.items():
        assert got[key] == want, f"{scene.name} ({scene.pins}): {key} is {got[key]}, the builder promises {want}"
    # every small splat covers one tile: the instance count is the candidate count wherever no probe is in the scene
    if "probes" not in scene.expect and "probe_tiles" not in scene.expect:
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


# ------------------------------------------------------------------------------------------------ k_bin_build
@pytest.mark.parametrize("shift", [4, 5])
@pytest.mark.parametrize("count", ls.BUILD_COUNTS + (16385,))
def test_build_size(oracle, count, shift):
    """The fullest bin of 16 x 16 or 32 x 32 tiles holds exactly `count`; up to 16384 the frame stays at level 0 -- k_bin_build's
    capacity is 16384 at every level -- and 16385 halves the bins first, a quarter of the candidates in each."""
    sc = ls.build_size(count, shift)
    assert (sc.width, sc.height) == ((512, 512) if shift == 4 else (1024, 1024)) and sc.env == {"GS_BIN_SHIFT": str(shift)}
    got, ref = _check(oracle, sc)
    assert got["fullest_bin"][shift] == count and ls.base_shift(2 << shift, 2 << shift, shift) == shift
    # round robin over the bin's tiles: the lists of the bin differ by one at most, and every tile of it has one from S^2 on
    b = ref["boundaries"].astype(np.int64)
    lens = (b[1::2] - b[0::2]).reshape(2 << shift, 2 << shift)[1 << shift:, 1 << shift:]
    assert lens.sum() == count and lens.max() - lens.min() <= 1
    bits = ref["attr"]["depth"][-count:].view(np.uint32)
    assert len(np.unique(bits)) == count and (count < 3 or (np.diff(bits.astype(np.int64)) < 0).any())   # distinct, not in id order
    p = ls.predict(sc)
    assert p == ls.predict(sc, forced=True)
    if count <= ls.BUILD_MAX:
        assert (p["sort_level"], p["retries"], p["bin_tiles"], p["max_bin_entries"]) == (0, 0, 1 << shift, count)
    else:
        assert ls.can_refine(sc.width, sc.height, shift) and sc.expect["fullest_bin"] == {shift: 16385, shift - 1: 4097}
        assert (p["sort_level"], p["retries"], p["bin_tiles"], p["max_bin_entries"]) == (3, 1, 1 << (shift - 1), 4097)


@pytest.mark.parametrize("shift,count", [(s, c) for s in (3, 4, 5) for c in ls.BUILD_GLOBAL_COUNTS] + [(4, ls.BUILD_STREAMED), (5, ls.BUILD_STREAMED)])
def test_build_size_on_the_global_path(oracle, shift, count):
    """The same scenes as the streamed forms run them (R2 = 1, 4, 16): level 5 at once, the scene's own bins, no re-run whatever
    the count; 70000 single-tile splats are 70000 instances."""
    sc = ls.build_size(count, shift)
    got, ref = _check(oracle, sc)
    assert got["fullest_bin"][shift] == count and len(ref["keys"]) == sc.expect["n"] <= 70600
    assert ls.predict(sc, sort_path=1) == dict(sort_level=5, sort_path=1, retries=0, bin_tiles=1 << shift, max_bin_entries=count,
                                               num_bin_entries=sc.expect["n"])
    assert sc.width * sc.height <= 1 << 20


@pytest.mark.parametrize("count", [16384, 16385])
def test_build_unrefinable(oracle, count):
    """4112 x 256: bins of 16 x 16 tiles by the frame's own size, 17 x 1 of them, the last one tile wide; they cannot be halved, so
    the 16385th candidate sends the frame straight to the global path -- once -- or is `bin too full` where bin-local is forced."""
    sc = ls.build_unrefinable(count)
    tx, ty = ls.tiles_across(sc.width), ls.tiles_across(sc.height)
    assert (tx, ty) == (257, 16) and ls.base_shift(tx, ty, 3) == 4 and not ls.can_refine(sc.width, sc.height, 3) and not sc.env
    got, _ = _check(oracle, sc)
    assert got["bin_counts"][4] == {(1, 0): count, (16, 0): 300} and got["tile_columns_of_the_last_bin"] == 1
    p, forced = ls.predict(sc), ls.predict(sc, forced=True)
    if count == 16384:
        assert (p["sort_path"], p["sort_level"], p["retries"]) == (2, 0, 0) and forced == p
    else:
        assert (p["sort_path"], p["sort_level"], p["retries"], p["bin_tiles"]) == (1, 5, 1, 16) and forced == "bin too full"


@pytest.mark.parametrize("shift", [4, 5])
def test_build_one_tile(oracle, shift):
    sc = ls.build_one_tile(shift)
    got, ref = _check(oracle, sc)
    s = 1 << shift
    assert got["longest_tile_list"] == ((s + 5, s + 3), 16384) and got["fullest_bin"][shift] == 16384
    # nothing else in that bin: its other tiles' lists are empty
    b = ref["boundaries"].astype(np.int64)
    lens = (b[1::2] - b[0::2]).reshape(2 * s, 2 * s)[s:, s:]
    assert lens.sum() == 16384 and np.count_nonzero(lens) == 1
    assert (ls.predict(sc)["sort_level"], ls.predict(sc)["retries"]) == (0, 0)


@pytest.mark.parametrize("shift", [4, 5])
def test_build_boxes(oracle, shift):
    sc = ls.build_boxes(shift)
    got, ref = _check(oracle, sc)
    s = 1 << shift
    boxes = dict(zip(ls.BOX_PROBES, [got["probe_tiles"][p] for p in sorted(got["probe_tiles"], key=list(sc.expect["probe_tiles"]).index)]))
    assert boxes["whole_bin"] == (s, s, 2 * s, 2 * s)
    assert boxes["tile_row"] == (s, 2 * s - 1, 2 * s, 2 * s) and boxes["tile_column"] == (2 * s - 1, s, 2 * s, 2 * s)
    x0, y0, x1, y1 = boxes["four_bins"]
    assert x0 < s < x1 and y0 < s < y1 and (x1 - x0, y1 - y0) == (6, 6)
    x0, y0, x1, y1 = boxes["frame_edge"]
    assert x1 == 2 * s == ls.tiles_across(sc.width) and (x1 - x0, y1 - y0) == (4, 6)
    # off the frame's edge the box would go on: the clamp to the tile grid is what cuts it (preprocess.comp:161-164)
    edge = list(sc.expect["probe_tiles"])[4]
    assert (ref["attr"]["uv"][edge, 0] + ref["attr"]["color_radii"][edge, 3] + 15) // 16 > 2 * s
    assert got["largest_other_tile_box"] == 1 and got["fullest_bin"][shift] == 3000 and got["instances"] == len(ref["keys"])
    assert (ref["attr"]["conic_opacity"][list(sc.expect["probe_tiles"]), 3] < 0.02).all()     # faint
    # the probes are among the bin's candidates at lanes 5 and 63, two neighbours and lane 0 of their chunks of 64
    first = sc.expect["n"] - 3000
    assert [(p - first) % 64 for p in sc.expect["probe_tiles"]] == [5, 63, 8, 9, 0]


@pytest.mark.parametrize("shift", [4, 5])
@pytest.mark.parametrize("place", ls.RUN_PLACES)
@pytest.mark.parametrize("length", [2, 100])
def test_equal_run_in_a_build_bin(oracle, length, place, shift):
    """3000 candidates in all: three rounds, 192 elements of the list per wave; the straddling run crosses element 192."""
    sc = ls.equal_run(length, place, False, shift=shift)
    got, _ = _check(oracle, sc)
    assert got["longest_run"] == length and got["fullest_bin"][shift] == 3000 and -(-3000 // ls.THREADS) * ls.WAVE == 192
    if place == "straddle":
        assert got["run_start"] < 192 <= got["run_start"] + length - 1 and (length < 31 or got["run_start"] == 192 - 30)
    p = ls.predict(sc)
    assert (p["sort_level"], p["retries"]) == (0, 0) and ls.predict(sc, forced=True) == p


def test_build_scenes_notice_a_missed_edge(oracle):
    """The re-measurement is sensitive: one candidate more or fewer in the fullest bin, a probe moved by a tile, a candidate of
    the one-tile scene in the next tile, the run one element later -- and the pinned quantities no longer hold."""
    sc = ls.build_size(16384, 4)
    sc.records = sc.records[:-1]
    with pytest.raises(AssertionError, match="the builder promises"):
        _check(oracle, sc)
    sc = ls.build_unrefinable(16385)
    sc.records = np.concatenate([sc.records, sc.records[300:301]])         # (one more in bin 1)
    with pytest.raises(AssertionError, match="the builder promises"):
        _check(oracle, sc)
    sc = ls.build_boxes(5)
    row = list(sc.expect["probe_tiles"])[1]
    sc.records[row, 1] -= np.float32(16.0 / (sc.width / (2.0 * np.tan(np.radians(ls.FOV) / 2.0))) * sc.records[row, 2])   # 16 px up
    with pytest.raises(AssertionError, match="probe_tiles"):
        _check(oracle, sc)
    sc = ls.build_one_tile(4)
    moved = ls._splats(sc.records[-1:, 2].copy().view(np.uint32) & np.uint32(0x7FFFFFFF), [22], [19], sc.width, sc.height)
    sc.records[-1] = moved[0]
    with pytest.raises(AssertionError, match="longest_tile_list"):
        _check(oracle, sc)
    sc = ls.equal_run(100, "straddle", False, shift=4)
    sc.expect["run_start"] += 1
    with pytest.raises(AssertionError, match="run_start"):
        _check(oracle, sc)


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


L1_COUNTS = [(1023, 0), (1024, 0), (1025, 0), (1023, 300), (1024, 300), (1025, 300)]


@pytest.mark.parametrize("n,culled", L1_COUNTS + [c for c in ls.ONE_PASS_L1_COUNTS if c not in L1_COUNTS])
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


# ------------------------------------------------------------------------------------------------ the spatial read order
@pytest.fixture(scope="module")
def spatial_sim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("spatial") / "libspatial_order_sim.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC,
                           os.path.join(ROOT, "tests", "native", "spatial_order_sim.cpp"), "-o", out])
    lib = C.CDLL(out)
    fp = C.POINTER(C.c_float)
    lib.so_order.argtypes = [fp, fp, fp, C.c_uint64, C.POINTER(C.c_uint32)]
    lib.so_order.restype = None
    lib.so_spread21.argtypes = [C.c_uint64]
    lib.so_spread21.restype = C.c_uint64

    def order(pos):
        planes = [np.ascontiguousarray(pos[:, k], np.float32) for k in range(3)]
        out = np.zeros(len(pos), np.uint32)
        lib.so_order(*[p.ctypes.data_as(fp) for p in planes], len(pos), out.ctypes.data_as(C.POINTER(C.c_uint32)))
        return out
    order.spread21 = lib.so_spread21
    return order


def _spatial_cases():
    rng = np.random.default_rng(7)
    n = 5000
    rnd = rng.normal(0.0, 3.0, (n, 3)).astype(np.float32)
    dup = rnd.copy()
    dup[n // 2:] = dup[:n - n // 2]                              # every position twice: the code ties, the id decides
    dup[::7] = dup[0]                                            # ... and one of them hundreds of times
    flat = rnd.copy()
    flat[:, 1] = np.float32(-2.5)                                # hi = lo + 1 on y
    far = rnd.copy()
    far[:, 2] = np.float32(3e9)                                  # lo + 1 == lo in binary32: 0 / 0 on z, cell 0
    odd = rnd.copy()
    odd[5::11, 0] = np.nan
    odd[3::13, 1] = np.inf
    odd[2::17, 2] = -np.inf
    odd[100] = (np.nan, np.inf, -np.inf)
    none = np.full((40, 3), np.nan, np.float32)                  # no finite coordinate at all: every code 0, id order
    coarse = (rng.integers(0, 4, (n, 3)) * 0.25).astype(np.float32)   # 64 distinct positions, on cell borders
    return dict(random=rnd, duplicates=dup, constant_axis=flat, constant_axis_far=far, non_finite=odd, nothing_finite=none,
                cell_borders=coarse, one=rnd[:1], two=rnd[:2], empty=rnd[:0])


@pytest.mark.parametrize("name", list(_spatial_cases()))
def test_spatial_order_header_against_numpy(spatial_sim, name):
    pos = _spatial_cases()[name]
    got, want = spatial_sim(pos), ls.morton_order(pos)
    np.testing.assert_array_equal(got, want)
    assert np.array_equal(np.sort(got), np.arange(len(pos)))
    if name == "nothing_finite":
        assert np.array_equal(got, np.arange(len(pos)))
    if name == "duplicates":
        rank = np.argsort(got)                                   # ties go by id: of two Gaussians in one place the lower id is read first
        half = len(pos) // 2
        same = (pos[:half] == pos[half:2 * half]).all(axis=1)
        assert same.sum() > 1000 and (rank[:half][same] < rank[half:2 * half][same]).all()
        crowd = np.arange(0, len(pos), 7)
        assert (np.diff(rank[crowd]) > 0).all()                  # the hundreds in one place: in id order


def test_spatial_order_bit_layout(spatial_sim):
    """x is the lowest bit of each triple: bit b of a cell lands on bit 3 b of the spread value; 21 bits, no more."""
    for b in range(21):
        assert spatial_sim.spread21(1 << b) == 1 << (3 * b)
    assert spatial_sim.spread21(1 << 21) == 0 and spatial_sim.spread21((1 << 21) - 1) == sum(1 << (3 * b) for b in range(21))
    # two points that differ in x alone, in y alone, in z alone, from a common corner: x moves the order least
    pos = np.array([[0, 0, 0], [0, 0, 1], [0, 1, 0], [1, 0, 0], [1, 1, 1]], np.float32)
    np.testing.assert_array_equal(spatial_sim(pos), [0, 3, 2, 1, 4])
    np.testing.assert_array_equal(ls.morton_order(pos), [0, 3, 2, 1, 4])


# ------------------------------------------------------------------------------------------------ preprocess, wave by wave
@pytest.mark.parametrize("tail", ls.WAVE_TAILS)
@pytest.mark.parametrize("order", ["index", "spatial"])
def test_wave_patterns(oracle, spatial_sim, order, tail):
    sc = ls.wave_patterns(order, tail)
    got, ref = _check(oracle, sc)
    masks = got["wave_masks"]
    counts = [bin(m).count("1") for m in masks]
    print(f"{sc.name}: N {got['n']}, V {got['visible']}, visible lanes per wave in read order {counts}")
    assert set(ls.WAVE_COUNTS) <= set(counts[:63]) and len(masks) == (64 if tail == "ends_group" else 65)
    assert masks.count(1) == 1 and masks.count(1 << 63) == 1    # "only lane 0", "only lane 63"
    assert got["ragged_lanes"] == ls.WAVE_RAGGED and got["waves_after_the_ragged_one"] == (0 if tail == "ends_group" else 3)
    last = masks[-1]
    assert last >> ls.WAVE_RAGGED == 0 and ((last & 1, last >> (ls.WAVE_RAGGED - 1)) == ((1, 1) if order == "index" else (1, 0)))
    # the order the kernels read in is the header's, and in spatial order it is the scramble the builder set out to get
    read = ls.read_order(sc)
    if order == "spatial":
        np.testing.assert_array_equal(spatial_sim(sc.records[:, :3]), read)
        n = len(read)
        np.testing.assert_array_equal(read, (np.arange(n, dtype=np.int64) * ls.PRIME + 12345) % n)
    # the float64 reference sees the same Gaussians, and the oracle's taps are its frame within float64_check's bounds
    fr = Frame(sc.name, sc.records, fov=ls.FOV, width=sc.width, height=sc.height)
    np.testing.assert_array_equal(chk.reference(fr)["pre"]["tiles"] > 0, ref["tiles"] != 0)
    out = dict(chk.outputs_from_oracle(oracle, ref), image=None)
    rep = chk.assert_matches_float64(out, fr)
    assert (rep["radius_explained"], rep["box_explained"], rep["visibility_explained"]) == (0, 0, 0)
    # SH rest coefficients that matter: the colour differs from the DC term's alone
    vis = ref["tiles"] != 0
    assert np.abs(ref["attr"]["color_radii"][vis, :3] - (0.28209479177387814 * sc.records[vis, 6:9] + 0.5)).max() > 0.5


def test_wave_patterns_notice_a_shifted_mask(oracle):
    """The re-measurement is sensitive: the same Gaussians one read slot later (index order), or two ids exchanged between a
    visible and a culled slot (spatial order), and the pinned masks no longer hold."""
    sc = ls.wave_patterns("index")
    sc.records = np.roll(sc.records, 1, axis=0)
    with pytest.raises(AssertionError, match="wave_masks"):
        _check(oracle, sc)
    sc = ls.wave_patterns("spatial")
    read = ls.read_order(sc)
    vis_slot = 64 * 2 + 0                                        # wave 2 is (count 4, lowest): its lane 0 is visible, lane 5 is not
    a, b = read[vis_slot], read[vis_slot + 5]
    x = sc.records[[a, b], 0].copy()
    sc.records[[a, b]] = sc.records[[b, a]]
    sc.records[[a, b], 0] = x                                    # (x stays with the id, so the read order stays)
    np.testing.assert_array_equal(ls.read_order(sc), read)
    with pytest.raises(AssertionError, match="wave_masks"):
        _check(oracle, sc)


def test_dense_lists_full(oracle):
    sc = ls.dense_lists_full()
    got, _ = _check(oracle, sc)
    assert got["list_fill"] == dict(lists=256, slots=1024, fewest=1024, most=1024) and got["n"] == got["visible"] == 262144
    # one workgroup fewer and the last list is a quarter short; one more and the lists grow by a whole level-1 block
    assert ls.vis_region_slots(262144 - 256) == 1024 and ls.vis_region_slots(262144 + 1) == 2048
    p = ls.predict(sc)
    assert (p["sort_level"], p["retries"]) == (0, 0)


# ------------------------------------------------------------------------------------------------ the one-pass level 1
def test_candidate_capacity_restated():
    """gs_renderer::init: min(max(2^18, 2 N), max(2^20, 8 N)), and what the two test knobs make of it; region_cap divides it by
    the on-screen bins, rounding down."""
    assert ls.candidate_capacity(1) == 1 << 18 and ls.candidate_capacity(131072) == 1 << 18 and ls.candidate_capacity(131073) == 262146
    assert ls.candidate_capacity(66136) == 262144                        # level2_size(65536): 4 bins of 65536 records
    assert ls.candidate_capacity(1 << 28) == 1 << 29 and ls.candidate_capacity(1 << 29) == ls.MAX_INSTANCES   # the instance maximum
    assert ls.candidate_capacity(5000, {"GS_INITIAL_CAPACITY": "3000"}) == 3000       # the lists' knob caps the candidates too
    assert ls.candidate_capacity(5000, {"GS_INITIAL_CAPACITY": "100"}) == 256
    assert ls.candidate_capacity(5000, {"GS_INITIAL_CAND_CAPACITY": "70000"}) == 70000
    assert ls.candidate_capacity(5000, {"GS_INITIAL_CAND_CAPACITY": "70000", "GS_INITIAL_CAPACITY": "3000"}) == 3000
    assert ls.region_cap(262144, 4) == 65536 and ls.region_cap(262144, 48) == 5461 and ls.region_cap(100, 0) == 0
    assert ls.screen_bins(128, 128, 2) == 4 and ls.screen_bins(1152, 128, 3) == 9 and ls.screen_bins(4112, 256, 4) == 17


def test_one_pass_regions_hold_the_fullest_bin():
    """Every scene test_gpu_limits.py runs on the one-pass level 1, at every bin edge the policy passes through on the way: the
    region a bin owns holds the fullest bin (a region that ran over would add a re-run and a hold, and the case would no longer
    test its own edge), and the candidate buffer holds E1.  level2_size(65536): the region holds EXACTLY the fullest bin."""
    seen = 0
    for sc, exact in ls.one_pass_scenes():
        cand = ls.candidate_capacity(sc.expect["n"], sc.env)
        tried = ls.attempts(sc)
        assert len(tried) == ls.predict(sc)["retries"] + 1
        for shift, level in tried:
            cap = ls.region_cap(cand, ls.screen_bins(sc.width, sc.height, shift))
            fullest = sc.expect["fullest_bin"][shift]
            assert cap >= fullest, f"{sc.name}: a region of {cap} records for a bin of {fullest} with bins of 2^{shift} tiles"
            assert not exact or cap == fullest, f"{sc.name}: a region of {cap} records is not full with {fullest}"
            assert sc.expect["bin_entries"][shift] <= cand
        seen += 1
    assert seen == 12 + 1 + 3 + 1 + 32 + 4 + 3 + 5 + 8 + 1
    # the last slot the slabs address is the last record of the region, and of the whole buffer
    sc = ls.level2_size(65536)
    assert ls.candidate_capacity(sc.expect["n"]) == 4 * 65536 and ls.one_pass_final(ls.predict(sc)) is False
    assert ls.one_pass_final(ls.predict(ls.level2_size(65535))) and not ls.one_pass_final(ls.predict(ls.build_size(*ls.ONE_PASS_REFUSAL)))


@pytest.mark.parametrize("tail", ls.WAVE_TAILS)
@pytest.mark.parametrize("order", ["index", "spatial"])
def test_one_pass_regions_of_the_wave_patterns(oracle, order, tail):
    """The same for test_preprocess_at_every_visible_lane_count's scenes (9 x 1 bins of 8 x 8 tiles, level 0, no re-run)."""
    sc = ls.wave_patterns(order, tail)
    _, _, ref = oracle_frame(oracle, sc.records, sc.width, sc.height)
    shift = ls.base_shift(ls.tiles_across(sc.width), ls.tiles_across(sc.height), sc.min_shift)
    fullest = max(len(v) for v in ls.bin_members(ref, shift).values())
    cap = ls.region_cap(ls.candidate_capacity(sc.expect["n"], sc.env), ls.screen_bins(sc.width, sc.height, shift))
    assert shift == 3 and fullest <= ls.LEVEL_LIMITS[0] and cap >= fullest


@pytest.mark.parametrize("extra", [False, True], ids=["at", "over"])
def test_wide_ratio(oracle, extra):
    """E1 = 8 V with every box 4 x 2 bins, and 8 V + 1 with one of 3 x 3: either side of L1FusedPolicy's wide-splat exit."""
    sc = ls.wide_ratio(extra)
    got, ref = _check(oracle, sc)
    ids, x0, y0, x1, y1 = ls.bin_boxes(ref, 2)
    shapes = sorted(set(zip((x1 - x0).tolist(), (y1 - y0).tolist())))
    assert shapes == ([(3, 3), (4, 2)] if extra else [(4, 2)]) and len(ids) == got["visible"] == 320
    e1 = got["bin_entries"][2]
    assert e1 == 8 * got["visible"] + extra and (e1 > ls.WIDE_RATIO * got["visible"]) == extra
    # the region: 5/4 of the fullest bin and more (L1FusedPolicy::cap_suffices), so only the ratio can keep the path off
    cap = ls.region_cap(ls.candidate_capacity(sc.expect["n"], sc.env), ls.screen_bins(sc.width, sc.height, 2))
    assert 4 * cap >= 5 * got["fullest_bin"][2] and ls.predict(sc)["retries"] == 0
    assert len(np.unique(ref["attr"]["depth"][ids].view(np.uint32))) == len(ids)


# ------------------------------------------------------------------------------------------------ the global path's grid
RADIX_CASES =[(n, None) for n in ls.RADIX_SIZES] + [(ls.RADIX_SIZES[1], v) for v in ls.RADIX_SMALL_V]


@pytest.mark.parametrize("n,v", RADIX_CASES)
def test_radix_blocks(oracle, n, v):
    sc = ls.radix_blocks(n, v)
    got, ref = _check(oracle, sc)
    r = got["radix"]
    print(f"{sc.name}: N {got['n']}, V {got['visible']}, {r}")
    assert (r["blocks"], r["per"]) == {524288: (256, 1), 524289: (257, 2), 1048577: (513, 3), 1572865: (769, 4),
                                       2097152: (1024, 4), 2097153: (1024, 4)}[n]
    assert r["blocks_owning_two_tiles"] == (1 if n == 2097153 else 0)
    if v is None:
        assert 10000 < got["visible"] < 50000 and (n != 2097153 or r["carry_shares_a_digit"] == [True] * 4)
        ids = np.nonzero(ref["tiles"])[0]
        whole = np.bincount(ids // ls.SORT_TILE, minlength=-(-n // ls.SORT_TILE))
        full = [t for t in ls._radix_whole_tiles(n)]
        assert all(whole[t] == min(ls.SORT_TILE, n - t * ls.SORT_TILE) for t in full) and whole.min() >= 1
    else:
        assert got["visible"] == v and r["tiles_of_the_later_passes"] == -(-v // 2048)
    # in the passes after the first (V keys, the grid still sized by N) at most one tile per block, and most blocks none
    t0, t1 = ls.radix_tiles_of_block(got["visible"], r["blocks"])
    assert (t1 - t0).max() == 1 and (t1 - t0 == 0).sum() == r["blocks"] - r["tiles_of_the_later_passes"] > r["blocks"] // 2


def test_radix_blocks_notice_a_perturbed_grid(oracle, monkeypatch):
    """The re-measurement is sensitive: one Gaussian fewer and no block owns two tiles; a grid restated with 1023 blocks, or
    tiles of 2047 keys, and the pinned numbers no longer hold."""
    sc = ls.radix_blocks(2097153)
    short = ls.LimitScene(sc.name, sc.records[:-1], sc.width, sc.height, sc.env, sc.pins, sc.expect)
    with pytest.raises(AssertionError, match="the builder promises"):
        _check(oracle, short)
    sc = ls.radix_blocks(524289, 2048)
    for name, value in (("SORT_MAX_BLOCKS", 256), ("SORT_TILE", 2047), ("SCAN_THREADS", 128)):
        with monkeypatch.context() as mp:
            mp.setattr(ls, name, value)
            with pytest.raises(AssertionError, match="radix"):
                _check(oracle, sc)
    _check(oracle, sc)
