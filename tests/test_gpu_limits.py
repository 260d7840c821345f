"""The per-frame kernels at the exact edge of their capacities and of their cooperative steps (scenes: tests/limit_scenes.py; that
they stand on the edge: tests/test_limit_scenes.py, on the CPU).  Every case: the stage taps bit for bit against the oracle, the
image bit for bit in exp mode 2, the default blend (mode 3) within the guarded tolerance, and the frame's stats -- level, path,
re-runs, bin edge, fullest bin, candidates -- equal to what the restated policy predicts for a fresh renderer.  A case that is
no longer on its edge FAILS: the pinned quantity is re-measured from the oracle's stages here too.

Binning and blend: every capacity.  k_bin_build, the level-2 kernel of bins of 16 x 16 and 32 x 32 tiles and of every bin size on
the global path, in its five instantiations: its one capacity (16384 at every bin-local level), the sort rounds of 1024, equal
depths across a wave's run of the list, a tile that takes all 16384, boxes clipped to the bin, a bin cut by the frame's edge, the
streamed lists of the global path up to 70000, and the list buffer running over inside the kernel.  k_preprocess: every count
of visible lanes of a wave at which its SH fetch, its run of slots in the dense lists or its record store changes shape, under
every combination of SH storage, read order, form of level 1 (planes, dense lists, one pass) and the antialiased mode, and the
dense lists full to their last slot.  The global depth order: every shape of its grid.

Which form of level 1 ran is part of every case: _assert_frame asserts level1_fused() of the frame that finally retired.  These
scenes are read in scene-id order and have no spatial copy, so by rule they run the three level-1 kernels; the test_one_pass_*
cases force the one-pass level 1 (k_preprocess files the bin candidates itself; level 2 reads the bins' cursors) onto the same
level-2 and level-1 edges, and a region of the candidate buffer that is full to its last record.

Not covered, and why:
  * k_bin_build's one-pass branch (bin_candidates / bin_offset / bin_close_one_pass / one_pass_visible inside it): unreachable, the
    one-pass level 1 needs bins of at most 8 x 8 tiles and k_bin_build orders bins of 16 x 16 and more, or the global path's
    (test_one_pass_refused_by_bins_of_16x16_tiles: the switch does not engage there).
  * kMaxSlabs = 16 and the planner's `remaining > MAXC` exit: a bin of <= 65535 candidates cannot be cut into more than 11
    slabs of <= 12288 (tests/test_limit_scenes.py::test_no_bin_of_a_frame_needs_more_than_eleven_slabs).  The nearest
    reachable case, 11 slabs of which five are full, is test_slab_planning[most].
  * kMsdBucketMax has no counter: 64 and 65 keys in a bucket must give the same lists, so those cases pin that BOTH orders are
    right at the hand-over, not which one ran.
  * k_preprocess's `det <= 0` exit: the 0.3 dilation keeps the determinant positive for every finite covariance, so no culled
    lane of the wave patterns takes it (they take the near cut, on either side of the camera, and the empty tile box).
  * a block of the radix passes that owns MORE than two tiles, and a carry between a block's tiles in the passes after the
    first: both need more than 2 097 152 keys (N > 3 145 728, V > 2 097 152); the full-size tests run them.
"""
import numpy as np
import pytest

import aa_reference as aa
import float64_check as chk
import limit_scenes as ls
import np_reference as npr
from float64_cases import Frame
from helpers import assert_guarded_close, assert_images_identical, compare_stages, expected_depth_order, oracle_frame

pytestmark = pytest.mark.gpu

STAT_KEYS = ("sort_path", "sort_level", "retries", "bin_tiles", "max_bin_entries", "num_bin_entries")


def _frame(pkg, oracle, monkeypatch, scene, extra_env=None):
    """The oracle's frame, the check that the scene is on its edge, and a fresh renderer under the scene's environment."""
    monkeypatch.delenv("GS_SORT_PATH", raising=False)
    for k, v in {**scene.env, **(extra_env or {})}.items():
        monkeypatch.setenv(k, v)
    verts, u_ref, ref = oracle_frame(oracle, scene.records, scene.width, scene.height)
    got = ls.measure(scene, ref)
    for key, want in scene.expect.items():
        assert got[key] == want, f"{scene.name} missed its edge ({scene.pins}): {key} is {got[key]}, not {want}"
    gs = pkg.Scene.from_records(scene.records, device=0)
    u = pkg.camera_uniforms(pkg.make_camera(), scene.width, scene.height)
    assert u.tobytes() == u_ref.tobytes()
    return gs, pkg.Renderer(gs), u, ref


def _assert_frame(pkg, rend, u, ref, scene, want, label, fused, grows=False):
    """One frame: stats as predicted, every stage and the mode-2 image exact, the default blend within the guarded tolerance.
    fused: what level1_fused() must say of the frame that finally retired -- k_preprocess filed the level-1 candidates itself.
    grows: the buffers start too small -- at least one re-run more than predicted, everything else as predicted."""
    img, _ = rend.render_host(u)
    took = rend.level1_fused()
    st = rend.stats()
    assert took == fused, f"{label}: the frame that retired {'took' if took else 'did not take'} the one-pass level 1"
    have = {k: getattr(st, k) for k in STAT_KEYS}
    print(f"{label}: {have}")
    if want is not None and grows:
        assert have["retries"] >= want["retries"] + 1, f"{label}: {have['retries']} re-runs with buffers that start too small"
        have["retries"] = want["retries"]
    if want is not None:
        assert have == {k: want[k] for k in STAT_KEYS}, f"{label}: stats {have}, predicted {want}"
    assert st.num_visible == scene.expect["visible"] and st.num_gaussians == scene.expect["n"]
    compare_stages(pkg, rend, u, ref)
    assert_images_identical(img, ref["image"], label=label)
    worst, redo, resolved = assert_guarded_close(rend, u, ref["image"], label=f"{label}, default blend")
    print(f"{label}: default blend max |d| {worst:.3g}, quadrants re-rendered {redo}, breaks resolved {resolved}")
    return st


BIN_TOO_FULL = "a bin holds more candidates than the bin-local sort can order"   # gs_renderer.cpp: DepthPolicy::kBinTooFull


def _run(pkg, oracle, monkeypatch, scene, forced=False, extra_env=None, global_path=False, grows=False, one_pass=False):
    """global_path: gs_set_sort_path(1), the global depth order at once (level 5, no re-run, the scene's own bins).
    one_pass: gs_set_level1_fused(1) before the first frame (these scenes are read in scene-id order and have no spatial copy: by
    rule they run the three level-1 kernels).  The frame that finally retires is then a one-pass frame exactly when it is
    bin-local with bins of at most 8 x 8 tiles, and the re-runs are the predicted ones EXACTLY: a region that ran over would add
    one, and a hold (tests/test_limit_scenes.py::test_one_pass_regions_hold_the_fullest_bin)."""
    gs, rend, u, ref = _frame(pkg, oracle, monkeypatch, scene, extra_env)
    try:
        assert not (forced and global_path) and not (one_pass and (forced or global_path or grows))
        want = ls.predict(scene, forced, sort_path=1 if global_path else 0) if "fullest_bin" in scene.expect else None
        assert not one_pass or isinstance(want, dict)
        rend.set_sort_path(1 if global_path else 2 if forced else 0)
        if one_pass:
            rend.set_level1_fused(1)
        fused = one_pass and ls.one_pass_final(want)
        label = f"{scene.name}{' forced' if forced else ' global' if global_path else ''}{' one-pass' if one_pass else ''}{' ' + str(extra_env) if extra_env else ''}"
        if want in ("error", "bin too full"):
            with pytest.raises(pkg.GsError) as e:
                rend.render_host(u)
            assert e.value.code == -5
            print(f"{label}: raised {e.value}")
            if want == "bin too full":
                assert BIN_TOO_FULL in str(e.value), f"{label}: the error of another failure: {e.value}"
            return None
        return _assert_frame(pkg, rend, u, ref, scene, want, label, fused, grows)
    finally:
        rend.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ level-2 sizes
@pytest.mark.parametrize("delta", [-1, 0, 1])
@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_level2_size_in_lds(pkg, oracle, gpu, monkeypatch, level, delta):
    """kBinSortLimit[0..3] = 4096 / 8192 / 12288 / 16384: L - 1 and L candidates run k_bin_fast<4 / 8 / 12 / 16>, L + 1 is re-run
    once at the next level (16385: depth slabs, since bins of 4 x 4 tiles cannot be refined)."""
    count = ls.LEVEL_LIMITS[level] + delta
    st = _run(pkg, oracle, monkeypatch, ls.level2_size(count))
    assert st.sort_level == level + (delta > 0) and st.max_bin_entries == count and st.retries == (st.sort_level > 0)
    _run(pkg, oracle, monkeypatch, ls.level2_size(count), forced=True)


def test_level2_16385_refines_the_bins_first(pkg, oracle, gpu, monkeypatch):
    """The other successor of 16384 + 1: where the bins can be halved they are, and the frame stays at the largest in-LDS order."""
    st = _run(pkg, oracle, monkeypatch, ls.level2_size(16385, shift=3))
    assert (st.bin_tiles, st.sort_level, st.retries, st.max_bin_entries) == (4, 3, 1, 4097)


@pytest.mark.parametrize("queue", ["1", "0"])
@pytest.mark.parametrize("count", [16385, 65534, 65535])
def test_level2_size_in_slabs(pkg, oracle, gpu, monkeypatch, count, queue):
    """Level 4 from its first candidate to its last, with the one-launch queue (GS_L2_QUEUE=1) and with k_bin_slabs + k_slab_work."""
    for forced in (False, True):
        st = _run(pkg, oracle, monkeypatch, ls.level2_size(count), forced=forced, extra_env={"GS_L2_QUEUE": queue})
        assert (st.sort_path, st.sort_level, st.retries, st.max_bin_entries) == (2, 4, 1, count)


@pytest.mark.parametrize("queue", ["1", "0"])
def test_level2_65536_leaves_the_bin_local_path(pkg, oracle, gpu, monkeypatch, queue):
    """One candidate beyond the slabs' 16-bit slot: the documented overflow error when the bin-local path is forced, the global
    path with the same lists in automatic mode."""
    sc = ls.level2_size(65536)
    assert _run(pkg, oracle, monkeypatch, sc, forced=True, extra_env={"GS_L2_QUEUE": queue}) is None
    st = _run(pkg, oracle, monkeypatch, sc, extra_env={"GS_L2_QUEUE": queue})
    assert (st.sort_path, st.sort_level, st.retries, st.max_bin_entries) == (1, 5, 1, 65536)


# ------------------------------------------------------------------------------------------------ equal-depth runs
@pytest.mark.parametrize("place", ls.RUN_PLACES)
@pytest.mark.parametrize("length", [64, 65, 66, 67])
def test_equal_depth_run_in_a_fast_bin(pkg, oracle, gpu, monkeypatch, length, place):
    """The tie step's run limit in k_bin_fast<4>: a run's first element counts at most 64 more, so 65 are ordered in place and 66
    take the second attempt (records rewritten in id order).  Either way the bin stays bin-local and the lists are exact."""
    for forced in (False, True):
        st = _run(pkg, oracle, monkeypatch, ls.equal_run(length, place, slab=False), forced=forced)
        assert (st.sort_path, st.sort_level, st.retries) == (2, 0, 0)


@pytest.mark.parametrize("queue", ["1", "0"])
@pytest.mark.parametrize("place", ls.RUN_PLACES)
@pytest.mark.parametrize("length", [64, 65, 66, 67])
def test_equal_depth_run_in_a_slab(pkg, oracle, gpu, monkeypatch, length, place, queue):
    """The same limit inside a depth slab, which has no second attempt: 64 and 65 stay at level 4; 66 and 67 send the frame to
    the global path (automatic) or raise (forced bin-local)."""
    sc = ls.equal_run(length, place, slab=True)
    env = {"GS_L2_QUEUE": queue}
    st = _run(pkg, oracle, monkeypatch, sc, extra_env=env)
    forced = _run(pkg, oracle, monkeypatch, sc, forced=True, extra_env=env)
    if length <= 65:
        assert (st.sort_path, st.sort_level, st.retries) == (2, 4, 1) and forced.sort_level == 4
    else:
        assert (st.sort_path, st.sort_level, st.retries) == (1, 5, 2) and forced is None


# ------------------------------------------------------------------------------------------------ k_bin_build
@pytest.mark.parametrize("shift", [4, 5])
@pytest.mark.parametrize("count", ls.BUILD_COUNTS)
def test_build_size_in_lds(pkg, oracle, gpu, monkeypatch, count, shift):
    """k_bin_build<4 / 16, 1024, true>: one candidate, a chunk of 64 and one more, a sort round of 1024 one short, full and one
    more (1025: two rounds, a wave owns 128 elements instead of 64), and its capacity -- 16383 and 16384, at LEVEL 0, since the
    kernel holds 16384 at every level.  No re-run at any of them, in automatic and in forced mode."""
    for forced in (False, True):
        st = _run(pkg, oracle, monkeypatch, ls.build_size(count, shift), forced=forced)
        assert (st.sort_path, st.sort_level, st.retries, st.max_bin_entries, st.bin_tiles) == (2, 0, 0, count, 1 << shift)


@pytest.mark.parametrize("shift", [4, 5])
def test_build_16385_refines_the_bins_first(pkg, oracle, gpu, monkeypatch, shift):
    """One beyond k_bin_build's capacity where the bins can be halved: one re-run with bins of half the edge (k_bin_fast<16> below
    shift 4, k_bin_build<4> below shift 5), a quarter of the candidates in each."""
    for forced in (False, True):
        st = _run(pkg, oracle, monkeypatch, ls.build_size(16385, shift), forced=forced)
        assert (st.bin_tiles, st.sort_path, st.sort_level, st.retries, st.max_bin_entries) == (1 << (shift - 1), 2, 3, 1, 4097)


@pytest.mark.parametrize("count", [16384, 16385])
def test_build_capacity_where_the_bins_cannot_be_halved(pkg, oracle, gpu, monkeypatch, count):
    """A frame 4112 px wide runs with bins of 16 x 16 tiles by itself, 17 x 1 of them (the last one tile wide), and they cannot be
    halved.  16384 in a bin: level 0.  16385: such bins have no slabs -- level 4 is the same kernel with the same capacity -- so
    the frame goes to the global path with ONE re-run, and forced bin-local mode says that the bin is too full (not that its
    depths are too crowded: no slab ever saw it)."""
    sc = ls.build_unrefinable(count)
    st = _run(pkg, oracle, monkeypatch, sc)
    forced = _run(pkg, oracle, monkeypatch, sc, forced=True)
    if count == 16384:
        assert (st.sort_path, st.sort_level, st.retries, st.bin_tiles) == (2, 0, 0, 16) and forced.sort_level == 0
    else:
        assert (st.sort_path, st.sort_level, st.retries, st.bin_tiles) == (1, 5, 1, 16) and forced is None


@pytest.mark.parametrize("shift", [4, 5])
def test_build_one_tile_takes_every_candidate(pkg, oracle, gpu, monkeypatch, shift):
    """16384 candidates in one tile of the bin: every chunk adds 64 to that tile's 16-bit count of the round, every round of 16
    chunks moves its ping-pong cursor by 1024, sixteen times over."""
    for forced in (False, True):
        st = _run(pkg, oracle, monkeypatch, ls.build_one_tile(shift), forced=forced)
        assert (st.sort_path, st.sort_level, st.retries, st.max_bin_entries) == (2, 0, 0, 16384)
    st = _run(pkg, oracle, monkeypatch, ls.build_one_tile(shift), global_path=True)
    assert (st.sort_path, st.sort_level, st.retries) == (1, 5, 0)


@pytest.mark.parametrize("shift", [4, 5])
def test_build_boxes_clipped_to_the_bin(pkg, oracle, gpu, monkeypatch, shift):
    """packed_cover_masks and the transpose over 256 and 1024 tile slots: a box that is the whole bin, one tile row of it, one tile
    column, a box over the corner of four bins (clipped into each) and one cut by the frame's edge, among single-tile boxes --
    with the boxes cached in LDS (R2 = 4) and recomputed (R2 = 16), sorted and streamed."""
    for mode in (dict(), dict(forced=True), dict(global_path=True)):
        st = _run(pkg, oracle, monkeypatch, ls.build_boxes(shift), **mode)
        assert st.retries == 0 and st.max_bin_entries == 3000 and st.bin_tiles == 1 << shift


@pytest.mark.parametrize("shift", [4, 5])
@pytest.mark.parametrize("place", ls.RUN_PLACES)
@pytest.mark.parametrize("length", [2, 100])
def test_equal_depth_run_in_a_build_bin(pkg, oracle, gpu, monkeypatch, length, place, shift):
    """k_bin_build has no tie step: its four passes are stable and its candidates arrive in id order, so equal depths must come
    out in id order whatever their number -- at the list's start, its end, across the border between two waves' elements
    (3000 candidates: three rounds, 192 elements per wave) and with the ids scattered over every wave.  No limit, no re-run."""
    for forced in (False, True):
        st = _run(pkg, oracle, monkeypatch, ls.equal_run(length, place, False, shift=shift), forced=forced)
        assert (st.sort_path, st.sort_level, st.retries) == (2, 0, 0)


@pytest.mark.parametrize("shift,count", [(s, c) for s in (3, 4, 5) for c in ls.BUILD_GLOBAL_COUNTS] + [(4, ls.BUILD_STREAMED), (5, ls.BUILD_STREAMED)])
def test_build_size_streamed(pkg, oracle, gpu, monkeypatch, shift, count):
    """k_bin_build<1 / 4 / 16, 1024, false>: the bin's list arrives ordered and is streamed, ids read back from LDS per fill round:
    one candidate, a round one short, full and one more, and beyond every capacity of the sorted forms (16385; 70000)."""
    st = _run(pkg, oracle, monkeypatch, ls.build_size(count, shift), global_path=True)
    assert (st.sort_path, st.sort_level, st.retries, st.max_bin_entries, st.bin_tiles) == (1, 5, 0, count, 1 << shift)


@pytest.mark.parametrize("shift,global_path", [(4, False), (5, False), (3, True), (4, True), (5, True)])
def test_build_list_buffer_runs_over(pkg, oracle, gpu, monkeypatch, shift, global_path):
    """Buffers that start at 256 entries: the candidate buffer grows first, then a frame overflows the list buffer INSIDE
    k_bin_build -- saturated ranges, stores dropped by the bounded buffer resource -- and is re-run; the lists are exact."""
    st = _run(pkg, oracle, monkeypatch, ls.build_size(1025, shift), global_path=global_path, extra_env={"GS_INITIAL_CAPACITY": "256"}, grows=True)
    assert st.retries >= 1 and st.max_bin_entries == 1025 and st.sort_path == (1 if global_path else 2)


# ------------------------------------------------------------------------------------------------ crowded bucket
@pytest.mark.parametrize("k", [63, 64, 65, 66])
def test_crowded_depth_bucket(pkg, oracle, gpu, monkeypatch, k):
    """kMsdBucketMax = 64 keys in one of the 4096 depth buckets: 64 are ranked inside the bucket, 65 hand the bin to the stable
    passes.  The kernel has no counter for which order ran: parity of the lists and the image at each k is the assertion."""
    st = _run(pkg, oracle, monkeypatch, ls.crowded_bucket(k))
    assert (st.sort_path, st.sort_level, st.retries) == (2, 0, 0)


# ------------------------------------------------------------------------------------------------ slab planning
@pytest.mark.parametrize("queue", ["1", "0"])
@pytest.mark.parametrize("kind", ["exact", "over", "most"])
def test_slab_planning(pkg, oracle, gpu, monkeypatch, kind, queue):
    """A slab full to its last place (12288), a slab that closes at 12287 because the next bucket would make it 12289, and the
    most slabs a bin of <= 65535 can be cut into (11; see the module docstring for kMaxSlabs)."""
    for forced in (False, True):
        st = _run(pkg, oracle, monkeypatch, ls.slab_plan(kind), forced=forced, extra_env={"GS_L2_QUEUE": queue})
        assert (st.sort_path, st.sort_level, st.retries) == (2, 4, 1)


# ------------------------------------------------------------------------------------------------ level 1
def _level1(pkg, oracle, monkeypatch, scene, dense_min, sort_path, one_pass=False):
    """one_pass: as _run's -- the switch forces the one-pass level 1, which then is what ran (bin-local, bins of 8 x 8 tiles or less)."""
    gs, rend, u, ref = _frame(pkg, oracle, monkeypatch, scene, {"GS_L1_DENSE_MIN": dense_min})
    try:
        rend.set_sort_path(sort_path)
        if one_pass:
            rend.set_level1_fused(1)
        want = ls.predict(scene)
        assert want["retries"] == 0 and want["sort_level"] == 0   # these scenes are about level 1: no bin beyond 4096
        if sort_path == 1:
            want.update(sort_path=1, sort_level=ls.GLOBAL_LEVEL)
        fused = one_pass and ls.one_pass_final(want)
        assert fused == (one_pass and sort_path == 0)
        _assert_frame(pkg, rend, u, ref, scene, want, f"{scene.name} dense_min {dense_min} path {sort_path}{' one-pass' if one_pass else ''}", fused)
    finally:
        rend.close()
        gs.close()


@pytest.mark.parametrize("dense_min", ["0", "1000000000"])
@pytest.mark.parametrize("n,culled", [(1023, 0), (1024, 0), (1025, 0), (1023, 300), (1024, 300), (1025, 300)])
def test_level1_items_around_one_block(pkg, oracle, gpu, monkeypatch, n, culled, dense_min):
    """kL1Items = 1024: N (the planes' items) and V (the dense lists' and the global path's items) one short of a block, a whole
    block, one beyond."""
    for sort_path in (0, 1):
        _level1(pkg, oracle, monkeypatch, ls.level1_count(n, culled), dense_min, sort_path)


@pytest.mark.parametrize("dense_min", ["0", "1000000000"])
@pytest.mark.parametrize("blocks", [31, 32, 33, 255, 256, 257])
def test_level1_block_counts_around_the_xcd_runs(pkg, oracle, gpu, monkeypatch, blocks, dense_min):
    """kL1XcdRun = 32 blocks per XCD run and 8 runs per round (l1_grid, l1_block): one run short by a block, exact, one over; the
    same for a whole round of 256."""
    _level1(pkg, oracle, monkeypatch, ls.level1_blocks(blocks), dense_min, 0)


@pytest.mark.parametrize("dense_min", ["0", "1000000000"])
@pytest.mark.parametrize("rows,cols", ls.BIG_BOXES)
def test_level1_bin_box_at_the_wave_emission_limit(pkg, oracle, gpu, monkeypatch, rows, cols, dense_min):
    """kL1BigBox = 12: bin boxes of exactly 12 bins are emitted by their own lane, boxes of 13 and 14 by the whole wave -- in
    k_l1_hist and in the scatter alike, or the counts and the lists disagree."""
    for sort_path in (0, 1):
        _level1(pkg, oracle, monkeypatch, ls.big_box(rows, cols), dense_min, sort_path)


# ------------------------------------------------------------------------------------------------ the same edges, one-pass level 1
# Level 2 then takes a bin's count from its cursor and its offset from (on-screen index) x (region size), and produces V, E1, the
# fullest bin and the overflow flag itself (gs_bin_l2.hip: bin_candidates, bin_offset, bin_close_one_pass, one_pass_visible) -- in
# k_bin_fast<4 / 8 / 12 / 16>, k_bin_slabs + k_slab_work and k_bin_queue; k_preprocess counts and files the candidates.  Automatic
# sort mode, the switch forced (_run: one_pass).  Everything _assert_frame checks, and that the frame that retired was a one-pass one.
@pytest.mark.parametrize("delta", [-1, 0, 1])
@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_one_pass_level2_size_in_lds(pkg, oracle, gpu, monkeypatch, level, delta):
    """test_level2_size_in_lds: the frame re-run one level up is a one-pass frame again (its cursors were zeroed by the frame
    that overflowed), and max_bin_entries / num_bin_entries are bin_close_one_pass's."""
    count = ls.LEVEL_LIMITS[level] + delta
    st = _run(pkg, oracle, monkeypatch, ls.level2_size(count), one_pass=True)
    assert st.sort_level == level + (delta > 0) and st.max_bin_entries == count and st.retries == (st.sort_level > 0)


def test_one_pass_level2_16385_refines_the_bins_first(pkg, oracle, gpu, monkeypatch):
    """The re-run has bins of half the edge: 16 regions of a sixteenth of the buffer where the first attempt had 4 of a quarter."""
    st = _run(pkg, oracle, monkeypatch, ls.level2_size(16385, shift=3), one_pass=True)
    assert (st.bin_tiles, st.sort_level, st.retries, st.max_bin_entries) == (4, 3, 1, 4097)


@pytest.mark.parametrize("queue", ["1", "0"])
@pytest.mark.parametrize("count", ls.ONE_PASS_SLAB_COUNTS)
def test_one_pass_level2_size_in_slabs(pkg, oracle, gpu, monkeypatch, count, queue):
    """Level 4 from its first candidate to its last: k_bin_queue reads every bin's cursor to rank the bins and again when it claims
    one.  At 66 135 Gaussians k_preprocess's 256 strided counters of visible Gaussians wrap: num_visible is one_pass_visible's sum."""
    st = _run(pkg, oracle, monkeypatch, ls.level2_size(count), extra_env={"GS_L2_QUEUE": queue}, one_pass=True)
    assert (st.sort_path, st.sort_level, st.retries, st.max_bin_entries) == (2, 4, 1, count)


@pytest.mark.parametrize("queue", ["1", "0"])
def test_one_pass_level2_65536_fills_its_region(pkg, oracle, gpu, monkeypatch, queue):
    """The region of the default candidate buffer holds exactly 65536 here, and it is the buffer's last: full to its last record it
    does not count as overflowed (no hold, no re-run for its sake) -- but the bin is beyond the slabs' 16-bit slot, so the frame ends
    on the global path with ONE re-run, and that frame is not a one-pass one."""
    st = _run(pkg, oracle, monkeypatch, ls.level2_size(65536), extra_env={"GS_L2_QUEUE": queue}, one_pass=True)
    assert (st.sort_path, st.sort_level, st.retries, st.max_bin_entries) == (1, 5, 1, 65536)


@pytest.mark.parametrize("place", ls.RUN_PLACES)
@pytest.mark.parametrize("length", [64, 65, 66, 67])
def test_one_pass_equal_depth_run_in_a_fast_bin(pkg, oracle, gpu, monkeypatch, length, place):
    """test_equal_depth_run_in_a_fast_bin with the bin's records in whatever order the workgroups' reservations fell."""
    st = _run(pkg, oracle, monkeypatch, ls.equal_run(length, place, slab=False), one_pass=True)
    assert (st.sort_path, st.sort_level, st.retries) == (2, 0, 0)


@pytest.mark.parametrize("queue", ["1", "0"])
@pytest.mark.parametrize("place", ls.RUN_PLACES)
@pytest.mark.parametrize("length", [64, 65, 66, 67])
def test_one_pass_equal_depth_run_in_a_slab(pkg, oracle, gpu, monkeypatch, length, place, queue):
    """test_equal_depth_run_in_a_slab: candidates of equal depth arrive in an order that differs from run to run, and 64 and 65 of
    them must still come out in id order; 66 and 67 end on the global path (two re-runs), which is not a one-pass frame."""
    st = _run(pkg, oracle, monkeypatch, ls.equal_run(length, place, slab=True), extra_env={"GS_L2_QUEUE": queue}, one_pass=True)
    assert (st.sort_path, st.sort_level, st.retries) == ((2, 4, 1) if length <= 65 else (1, 5, 2))


@pytest.mark.parametrize("k", [63, 64, 65, 66])
def test_one_pass_crowded_depth_bucket(pkg, oracle, gpu, monkeypatch, k):
    st = _run(pkg, oracle, monkeypatch, ls.crowded_bucket(k), one_pass=True)
    assert (st.sort_path, st.sort_level, st.retries) == (2, 0, 0)


@pytest.mark.parametrize("queue", ["1", "0"])
@pytest.mark.parametrize("kind", ["exact", "over", "most"])
def test_one_pass_slab_planning(pkg, oracle, gpu, monkeypatch, kind, queue):
    st = _run(pkg, oracle, monkeypatch, ls.slab_plan(kind), extra_env={"GS_L2_QUEUE": queue}, one_pass=True)
    assert (st.sort_path, st.sort_level, st.retries) == (2, 4, 1)


@pytest.mark.parametrize("rows,cols", ls.BIG_BOXES)
def test_one_pass_bin_box_at_the_wave_emission_limit(pkg, oracle, gpu, monkeypatch, rows, cols):
    """kL1BigBox = 12, which k_preprocess restates from k_l1_hist: a box of exactly 12 bins is emitted by its own lane, one of 13
    or 14 by the whole wave -- in the kernel's counting half and in its filing half alike, or a bin's cursor and its records disagree."""
    _level1(pkg, oracle, monkeypatch, ls.big_box(rows, cols), "1000000000", 0, one_pass=True)


@pytest.mark.parametrize("n,culled", ls.ONE_PASS_L1_COUNTS)
def test_one_pass_items_around_one_workgroup(pkg, oracle, gpu, monkeypatch, n, culled):
    """k_preprocess's workgroup of 256: one short of it, one workgroup, one beyond, and four and a ragged fifth -- whose lanes
    without a Gaussian still take part in the barriers of the counting and the filing half and reserve nothing."""
    _level1(pkg, oracle, monkeypatch, ls.level1_count(n, culled), "1000000000", 0, one_pass=True)


def test_one_pass_refused_by_bins_of_16x16_tiles(pkg, oracle, gpu, monkeypatch):
    """The switch asks, the frame's structure refuses: k_bin_build's bins take their candidates in id order from the three kernels."""
    st = _run(pkg, oracle, monkeypatch, ls.build_size(*ls.ONE_PASS_REFUSAL), one_pass=True)
    assert (st.sort_path, st.sort_level, st.retries, st.max_bin_entries, st.bin_tiles) == (2, 0, 0, 1025, 16)
    assert not ls.one_pass_final(ls.predict(ls.build_size(*ls.ONE_PASS_REFUSAL)))


# ------------------------------------------------------------------------------------------------ blend chunks
@pytest.mark.parametrize("lockstep", [0, 1])
@pytest.mark.parametrize("k", ls.BLEND_LENGTHS)
def test_blend_list_lengths_around_the_chunks(pkg, oracle, gpu, monkeypatch, k, lockstep):
    """The blend walks a list in chunks of 64, ids fetched two chunks ahead and records one: lists that end one short of a
    chunk, on it and one beyond, for one, two and three chunks, with every entry walked (no pixel stops early)."""
    scene = ls.blend_chunk(k)
    gs, rend, u, ref = _frame(pkg, oracle, monkeypatch, scene)
    try:
        rend.set_blend_lockstep(lockstep)
        st = _assert_frame(pkg, rend, u, ref, scene, None, f"{scene.name} lockstep {lockstep}", False)
        assert st.num_instances == scene.expect["instances"]
        ranges = rend.stage("ranges", u).astype(np.int64)
        tx = ls.tiles_across(scene.width)
        assert ranges[2 * (1 * tx + 2) + 1] - ranges[2 * (1 * tx + 2)] == k
    finally:
        rend.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ guard triggers
def _guard_case(pkg, oracle, monkeypatch, scene):
    """Mode 2 exact and mode 3 within the guarded tolerance like every case; then the default blend's counters, and the quadrant
    under test bit for bit against the reference where it was re-rendered with the reference's arithmetic."""
    gs, rend, u, ref = _frame(pkg, oracle, monkeypatch, scene)
    try:
        _assert_frame(pkg, rend, u, ref, scene, None, scene.name, False)
        rend.set_exp_mode(3)
        rend.set_blend_contraction(False)
        img, _ = rend.render_host(u)
        st = rend.stats()
        rend.set_exp_mode(2)
        redo, resolved = int(st.blend_redo), int(st.blend_resolved)
        print(f"{scene.name}: quadrants re-rendered {redo}, breaks resolved {resolved}")
        q = ls.GUARD_QUADRANT
        same = np.array_equal(img[q][..., :3].view(np.uint32), np.ascontiguousarray(ref["image"][q][..., :3]).view(np.uint32))
        return redo, resolved, same
    finally:
        rend.close()
        gs.close()


def _oracle_image(oracle):
    return lambda rec: oracle_frame(oracle, rec, ls.GUARD_FRAME, ls.GUARD_FRAME)[2]["image"]


@pytest.mark.parametrize("kept", [384, 385])
def test_guard_list_of_kept_entries(pkg, oracle, gpu, monkeypatch, kept):
    """kGuardList = 384: a break decision inside the window at the quadrant's 384th kept entry is replayed from the wave's list;
    at the 385th the list does not hold it and the quadrant is re-rendered with the reference's arithmetic."""
    redo, resolved, same = _guard_case(pkg, oracle, monkeypatch, ls.guard_list(kept, _oracle_image(oracle)))
    if kept == 384:
        assert (redo, resolved) == (0, 1)
    else:
        assert redo == 1 and same


@pytest.mark.parametrize("count", [8, 9])
def test_guard_replays_per_quadrant(pkg, oracle, gpu, monkeypatch, count):
    """kGuardMaxResolves = 8: eight pixels of a quadrant with their break decision inside the window are eight replays; the ninth
    gives the quadrant up."""
    redo, resolved, same = _guard_case(pkg, oracle, monkeypatch, ls.guard_resolves(count, _oracle_image(oracle)))
    if count == 8:
        assert (redo, resolved) == (0, 8)
    else:
        assert redo == 1 and same


@pytest.mark.parametrize("kept", [4095, 4096, 4097])
def test_guard_pairs_per_quadrant(pkg, oracle, gpu, monkeypatch, kept):
    """kGuardMaxPairs = 4096 kept entries per quadrant, the n of the coarse window: 4096 are blended by the guarded loop, 4097 are
    not."""
    redo, resolved, same = _guard_case(pkg, oracle, monkeypatch, ls.guard_pairs(kept))
    if kept <= 4096:
        assert redo == 0
    else:
        assert redo == 1 and same


# ------------------------------------------------------------------------------------------------ preprocess, wave by wave
AA_RECORD_TAPS = ("radius", "conic_opacity", "uv_rg", "b", "alpha_cut")
_wave_refs = {}


def _wave_reference(oracle, order, tail, sh16):
    """The scene, the oracle's frame of it (on coefficients rounded to binary16 where the scene is read from that storage), its
    re-measured pins and the float64 frame description: computed once per (order, tail, storage), shared by the cases, read only."""
    key = (order, tail, sh16)
    if key not in _wave_refs:
        scene = ls.wave_patterns(order, tail)
        verts, u_ref, ref = oracle_frame(oracle, scene.records, scene.width, scene.height)
        got = ls.measure(scene, ref)
        for name, want in scene.expect.items():
            assert got[name] == want, f"{scene.name} missed its pattern: {name} is {got[name]}, not {want}"
        if sh16:
            verts["sh"] = verts["sh"].astype(np.float16).astype(np.float32)
            ref = oracle.stages(verts, u_ref)
        frame = Frame(scene.name, scene.records, fov=ls.FOV, width=scene.width, height=scene.height, sh16=sh16)
        _wave_refs[key] = (scene, verts, u_ref, ref, frame)
    return _wave_refs[key]


def _all_taps(rend, u):
    """Every stage tap of the last frame, the record's fields of the visible Gaussians only."""
    tiles = rend.stage("tiles")
    vis = tiles != 0
    out = dict(tiles=tiles, depth=rend.stage("depth")[vis], aabb=rend.stage("aabb").reshape(-1, 4)[vis])
    for name in AA_RECORD_TAPS:
        t = rend.stage(name)
        out[name] = (t.reshape(len(tiles), -1)[vis] if t.size != len(tiles) else t[vis]).view(np.uint32)
    for name in ("sorted_tile", "sorted_gid"):
        out[name] = rend.stage(name)
    out["ranges"] = rend.stage("ranges", u)
    return out


# The three forms of level 1, by name: (GS_L1_DENSE_MIN, gs_set_level1_fused on every renderer of the test; None: its default).
# planes: k_l1_hist / k_l1_scan / k_l1_scatter_any_order over the N-wide planes -- switched off explicitly, because a spatially
# ordered scene below dense_min takes the one-pass form by rule; dense_lists: the three kernels over the dense lists;
# one_pass: k_preprocess files the candidates itself -- forced, because in index order the rule refuses for lack of a spatial copy.
LEVEL1_FORMS = {"planes": ("1000000000", 0), "dense_lists": ("0", None), "one_pass": ("1000000000", 1)}


@pytest.mark.parametrize("antialiased", [False, True], ids=["plain", "antialiased"])
@pytest.mark.parametrize("level1", list(LEVEL1_FORMS))
@pytest.mark.parametrize("order", ["index", "spatial"])
@pytest.mark.parametrize("sh16", [False, True], ids=["fp32", "binary16"])
@pytest.mark.parametrize("tail", ls.WAVE_TAILS)
def test_preprocess_at_every_visible_lane_count(pkg, oracle, gpu, monkeypatch, tail, sh16, order, level1, antialiased):
    """k_preprocess's wave-cooperative steps -- the LDS-DMA fetch of the SH blocks by rank, the wave's run of slots in the dense
    lists or the one-pass level 1's count and filing of the bin candidates, the four-lanes-per-record store through the scene ids
    -- at every count and placement of visible lanes (limit_scenes.wave_patterns), for each combination of SH storage, read order,
    form of level 1 (LEVEL1_FORMS) and the antialiased mode.  The plain frame: every tap and the mode-2 image bit for bit against
    the oracle, the default blend within the guarded tolerance, V and N, and the taps against float64.  The antialiased frame
    (k_preprocess<true, 4> in the one-pass form): test_gpu_antialiased.py's contract.  Every frame ran the form the case is named for."""
    scene, verts, u_ref, ref, frame = _wave_reference(oracle, order, tail, sh16)
    dense_min, switch = LEVEL1_FORMS[level1]
    fused = level1 == "one_pass"
    monkeypatch.delenv("GS_SORT_PATH", raising=False)
    for k, v in {**scene.env, "GS_L1_DENSE_MIN": dense_min}.items():
        monkeypatch.setenv(k, v)
    label = f"{scene.name} {'binary16' if sh16 else 'fp32'} {level1}"
    u = pkg.camera_uniforms(pkg.make_camera(), scene.width, scene.height)
    assert u.tobytes() == u_ref.tobytes()
    gs = pkg.Scene.from_records(scene.records, device=0)
    made = [gs]
    try:
        if sh16:
            gs.quantize_sh()
        rend = pkg.Renderer(gs)
        made.append(rend)
        if switch is not None:
            rend.set_level1_fused(switch)
        _assert_frame(pkg, rend, u, ref, scene, None, label, fused)
        assert rend.level1_fused() == fused, f"{label}: the default blend's frame"
        out = chk.outputs_from_hip(rend, u)
        rep = chk.assert_matches_float64(out, frame, label=f"{label} (HIP taps)")
        assert (rep["radius_explained"], rep["box_explained"], rep["visibility_explained"]) == (0, 0, 0)
        if not antialiased:
            return
        off = _all_taps(rend, u)
        plain = rend.stage("conic_opacity").reshape(-1, 4)[:, 3].copy()
        rend.set_antialiased(True)
        img_on, _ = rend.render_host(u)
        assert rend.level1_fused() == fused, f"{label}: the antialiased frame"
        st = rend.stats()
        assert st.num_visible == scene.expect["visible"] and st.num_gaussians == scene.expect["n"]
        on = _all_taps(rend, u)
        # taps other than the opacity and its alpha cut: the mode-off frame's
        for name in off:
            if name not in ("conic_opacity", "alpha_cut"):
                np.testing.assert_array_equal(on[name], off[name], err_msg=f"{label}: tap {name} with the mode on")
        np.testing.assert_array_equal(on["conic_opacity"][:, :3], off["conic_opacity"][:, :3])
        vis = on["tiles"] != 0
        scaled = rend.stage("conic_opacity").reshape(-1, 4)[:, 3]
        assert (scaled[vis] < plain[vis]).all() and (on["alpha_cut"].view(np.float32) >= off["alpha_cut"].view(np.float32)).all()
        # the frame: the plain frame of S', on the device and from the oracle
        prime = verts.copy()
        prime["scale_opacity"][vis, 3] = scaled[vis]
        s2 = pkg.Scene.from_vertices(prime, device=0)
        made.append(s2)
        if sh16:
            s2.quantize_sh()
        r2 = pkg.Renderer(s2)
        made.append(r2)
        if switch is not None:
            r2.set_level1_fused(switch)
        img2, _ = r2.render_host(u)
        assert r2.level1_fused() == fused, f"{label}: the plain frame of S'"
        np.testing.assert_array_equal(img_on.view(np.uint32), img2.view(np.uint32))
        two = _all_taps(r2, u)
        for name in on:
            np.testing.assert_array_equal(on[name], two[name], err_msg=f"{label}: tap {name}, mode on vs the plain frame of S'")
        ref2 = oracle.stages(prime, u_ref)
        assert_images_identical(img_on, ref2["image"], label=f"{label}: antialiased frame vs the oracle on S'")
        assert (ref2["image"][..., :3] != 0).any()
        compare_stages(pkg, rend, u, ref2)
        np.testing.assert_array_equal(on["alpha_cut"], oracle.alpha_cut(prime["scale_opacity"][:, 3])[vis].view(np.uint32))
        assert_guarded_close(rend, u, ref2["image"], label=f"{label}: antialiased, default blend vs the oracle on S'")
        # the factor against float64, within aa_reference's bound
        pre = npr.preprocess(npr.activate(scene.records), frame.camera64())
        sub = {k: (v[vis] if isinstance(v, np.ndarray) and v.shape[:1] == (len(vis),) else v) for k, v in pre.items()}
        comp_gpu = scaled[vis].astype(np.float64) / plain[vis]
        want = aa.comp64(sub)
        bad = aa.comp_violations(comp_gpu, sub, want)
        worst = float((np.abs(comp_gpu ** 2 - want ** 2) / aa.comp_tolerance(sub)).max())
        print(f"{label}: comp in [{comp_gpu.min():.3g}, {comp_gpu.max():.3g}], worst |d comp^2| / bound = {worst:.3g}")
        assert not bad.any(), f"{label}: {bad.sum()} of {len(bad)} factors outside the bound; worst |d comp^2| / bound = {worst:.3g}"
    finally:
        for o in reversed(made):
            o.close()


def test_dense_lists_full_to_the_last_slot(pkg, oracle, gpu, monkeypatch):
    """262144 Gaussians, all visible: each of the 256 dense lists receives exactly its 1024 slots' worth, from four workgroups."""
    _level1(pkg, oracle, monkeypatch, ls.dense_lists_full(), "0", 0)


# ------------------------------------------------------------------------------------------------ the global path's grid
@pytest.mark.parametrize("n,v", [(n, None) for n in ls.RADIX_SIZES] + [(ls.RADIX_SIZES[1], v) for v in ls.RADIX_SMALL_V])
def test_global_depth_order_grid(pkg, oracle, gpu, monkeypatch, n, v):
    """The radix passes' grid, blocks = min(1024, ceil(N / 2048)): k_radix_scan's 1, 2, 3 and 4 entries per thread (256 | 257,
    513, 769 blocks), 1024 blocks of one tile each and 1024 blocks of which the last owns two (the carry between a block's tiles),
    with the later passes running over V << N keys -- one tile one key short, full, and one key into the next among them."""
    scene = ls.radix_blocks(n, v)
    gs, rend, u, ref = _frame(pkg, oracle, monkeypatch, scene)
    try:
        rend.set_sort_path(1)
        img, _ = rend.render_host(u)
        st = rend.stats()
        print(f"{scene.name}: {scene.pins}; sort_path {st.sort_path}, retries {st.retries}, V {st.num_visible}")
        assert (st.sort_path, st.retries, st.num_visible, st.num_gaussians) == (1, 0, scene.expect["visible"], n)
        vis = np.nonzero(ref["tiles"])[0]
        bits = ref["attr"]["depth"][vis].view(np.uint32)
        want = vis[np.lexsort((vis, bits))].astype(np.uint32)
        np.testing.assert_array_equal(want, expected_depth_order(ref["attr"], ref["tiles"]))
        got = rend.stage("depth_order")
        bad = np.nonzero(got != want)[0] if len(got) == len(want) else None
        assert bad is not None and len(bad) == 0, (f"{scene.name}: the depth order has {len(got)} entries for {len(want)}" if bad is None else
                                                  f"{scene.name}: the depth order differs at {len(bad)} places, first {bad[:4]}")
        compare_stages(pkg, rend, u, ref)
        assert_images_identical(img, ref["image"], label=scene.name)
    finally:
        rend.close()
        gs.close()
