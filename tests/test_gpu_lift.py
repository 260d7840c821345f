"""gs_lift_pixels on the device (gs_lift.hip) against its definition restated in numpy (tests/lift_reference.py, pinned to the
oracle's image by tests/test_lift_api.py).  The sums are binary64 and the order of the adds is unspecified, so there are two
kinds of comparison, with no case left out of either:
  - TOLERANCE: for every (g, c), |got - want| <= 2 n_g 2^-53 A[g][c], n_g the number of terms Gaussian g receives and A the sum
    of their magnitudes, both from the reference; any order of n_g binary64 adds lies within (n_g - 1) 2^-53 A of the exact sum,
    and so does the reference's own: the factor 2.  A row with n_g = 0 keeps the bits it held.
  - EXACT: a mask that counts one or two pixels gives every Gaussian at most two terms, and a binary64 add is commutative: out and
    out_weight equal the reference bit for bit.
Outputs are views into larger device buffers with guard words, offset so that they are 8-byte aligned and nothing more; values
are 4-byte aligned and nothing more, the mask starts at an odd address.  Renderers start in exp mode 2 (conftest); every test
runs on both depth-order paths."""
import os
import re

import numpy as np
import pytest
import torch  # at collection, before the package loads its library: both must bind the same HIP runtime

import lift_reference as lref
import limit_scenes as ls
from helpers import assert_images_identical, compare_stages, oracle_frame
from test_gpu_blend_chunk_loop import _grazing_scene, _saturated_quadrant, _tile_list

pytestmark = pytest.mark.gpu


def _source_constant(header, pattern):
    """An integer constant read from the kernels' own sources: the channel counts and list lengths below bracket the values the
    library is BUILT with, not copies of them."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "3dgs.cpp_amd", "csrc", header)
    with open(path) as f:
        found = re.findall(pattern, f.read(), re.M)
    assert len(found) == 1, (header, pattern, found)
    return int(found[0])


G = _source_constant("gs_kernels.h", r"\bkLiftGroup = (\d+)")             # channels per launch
SMALL = _source_constant("gs_kernels.h", r"\bkLiftGroupSmall = (\d+)")     # a last group of at most SMALL runs a kernel of SMALL
CHUNK = _source_constant("gs_device.h", r"^#define WAVE (\d+)")            # gs_lift.hip stages WAVE entries per chunk
assert 1 < SMALL < G - 1 and CHUNK == 64
SCENES = {"A": (600, 72, 40), "T": (1500, 64, 64)}    # synth_records(n, seed=5, kind) at width x height; 72 x 40 = 4.5 x 2.5 tiles
CAMERAS = [{}, dict(position=(0.3, -0.2, 0.5)), dict(position=(-0.25, 0.1, 0.3))]
GUARD, SENTINEL = 37, -7777.25                        # guard words on either side of a view (odd: an output is 8-byte aligned only)
U53, U24 = 2.0 ** -53, 2.0 ** -24
_cache = {}


def _values(h, w, channels, seed=23):
    """Seeded pixel rows with negatives, an all-zero channel (1) and a channel of ones (2: its lift is the weight)."""
    v = np.random.default_rng(seed).standard_normal((h, w, channels)).astype(np.float32)
    if channels > 1:
        v[..., 1] = 0.0
    if channels > 2:
        v[..., 2] = 1.0
    return v


def _freeze(want):
    for a in want.values():
        a.setflags(write=False)
    return want


def _records(pkg, kind):
    return pkg.synth.synth_records(SCENES[kind][0], seed=5, kind=kind)


def _frame(pkg, oracle, kind, cam=0):
    key = (kind, cam)
    if key not in _cache:
        _, w, h = SCENES[kind]
        _cache[key] = oracle_frame(oracle, _records(pkg, kind), w, h, oracle.default_camera(**CAMERAS[cam]))
    return _cache[key]


def _reference(pkg, oracle, kind, cam=0, channels=5):
    """(verts, oracle stages, values, reference lift) of a synthetic scene seen by CAMERAS[cam]: computed once, never changed."""
    key = (kind, cam, channels)
    if key not in _cache:
        _, w, h = SCENES[kind]
        verts, _, ref = _frame(pkg, oracle, kind, cam)
        vals = _values(h, w, channels)
        vals.setflags(write=False)
        _cache[key] = (verts, ref, vals, _freeze(lref.lift(oracle, ref, w, h, vals)))
    return _cache[key]


def _uniforms(pkg, kind, cam=0):
    _, w, h = SCENES[kind]
    return pkg.camera_uniforms(pkg.make_camera(**CAMERAS[cam]), w, h)


def _open(pkg, kind):
    gs = pkg.Scene.from_records(_records(pkg, kind), device=0)
    return gs, pkg.Renderer(gs)


def _offset_view(array, dtype, lead):
    """`array` on the device as a view `lead` elements into a larger buffer: aligned to its element and nothing more."""
    a = np.array(array, order="C")       # (a copy: the cached arrays are read-only)
    buf = torch.zeros(a.size + 2 * lead, dtype=dtype, device="cuda")
    view = buf[lead:lead + a.size].view(a.shape)
    view.copy_(torch.as_tensor(a).to(dtype))
    assert view.is_contiguous() and view.data_ptr() % (2 * view.element_size()) != 0
    return view


def _values_tensor(vals):
    return None if vals is None else _offset_view(vals, torch.float32, 1)


def _mask_tensor(mask, dtype=torch.uint8):
    return None if mask is None else _offset_view(np.asarray(mask) != 0 if dtype == torch.bool else mask, dtype, 1)


class Sums:
    """out (n, channels) and weight (n,) as float64 views into larger flat device buffers: `preload` in the views, a sentinel
    in the guard words around them."""

    def __init__(self, n, channels, preload=0.0, only=("out", "weight")):
        self.buf, self.t, self.preload = {}, {}, float(preload)
        for name in only:
            shape = (n, channels) if name == "out" else (n,)
            numel = int(np.prod(shape))
            self.buf[name] = torch.full((numel + 2 * GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
            self.t[name] = self.buf[name][GUARD:GUARD + numel].view(shape)
            self.t[name].fill_(self.preload)
            assert self.t[name].is_contiguous() and self.t[name].data_ptr() % 8 == 0 and self.t[name].data_ptr() % 16 != 0

    def get(self, name):
        return self.t[name].cpu().numpy()

    def guards_intact(self):
        for name, b in self.buf.items():
            g = torch.cat([b[:GUARD], b[-GUARD:]]).cpu().numpy()
            assert (g == SENTINEL).all(), f"{name}: a guard word was written"


def _want(want, name, channels):
    """(sum, terms, magnitude) of the reference for an output, as arrays of the output's shape."""
    if name == "out":
        return want["out"][:, :channels], np.broadcast_to(want["terms"][:, None], (len(want["terms"]), channels)), want["A"][:, :channels]
    return want["weight"], want["terms"], want["abs_weight"]


def _assert_close(sums, want, label, times=1):
    """Every element within the bound of the definition, `times` calls after the preload; untouched rows keep their bits."""
    sums.guards_intact()
    worst = 0.0
    for name in sums.t:
        got = sums.get(name)
        total, terms, mag = _want(want, name, got.shape[1] if name == "out" else 0)
        assert got.shape == total.shape, (label, name, got.shape, total.shape)
        n = times * terms + (1 if sums.preload != 0.0 else 0)          # what the element held is one more term of the sum
        bound = 2.0 * n * U53 * (times * mag + abs(sums.preload))
        err = np.abs(got - (sums.preload + times * total))
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        bad = np.argwhere(~(err <= bound))
        assert len(bad) == 0, (f"{label}: {name} is outside the bound at {len(bad)} place(s), first {tuple(bad[0])}: "
                               f"{got[tuple(bad[0])]!r} against {(sums.preload + times * total)[tuple(bad[0])]!r}, bound {bound[tuple(bad[0])]:.3g}")
        untouched = terms == 0
        assert (got[untouched].view(np.uint64) == np.float64(sums.preload).view(np.uint64)).all(), f"{label}: {name}: a row without terms changed"
    print(f"{label}: worst error / bound = {worst:.3g}")


def _assert_bits(sums, want, label):
    sums.guards_intact()
    assert sums.preload == 0.0
    for name in sums.t:
        got = sums.get(name)
        total, _, _ = _want(want, name, got.shape[1] if name == "out" else 0)
        bad = np.argwhere(got.view(np.uint64) != np.ascontiguousarray(total).view(np.uint64))
        assert len(bad) == 0, f"{label}: {name} differs at {len(bad)} place(s), first {tuple(bad[0])}: {got[tuple(bad[0])]!r} != {total[tuple(bad[0])]!r}"


def _run(rend, vals, want, n, label, mask=None, only=("out", "weight"), preload=0.0, check=_assert_close, mask_dtype=torch.uint8):
    channels = 0 if vals is None else vals.shape[2]
    only = tuple(o for o in only if not (o == "out" and vals is None))
    sums = Sums(n, channels, preload, only)
    got = rend.lift_pixels(_values_tensor(vals), mask=_mask_tensor(mask, mask_dtype), **sums.t)
    assert sorted(got) == sorted(sums.t)
    check(sums, want, label)
    return sums


# ------------------------------------------------------------------------------------------------ 1. whole frame
@pytest.mark.parametrize("kind", sorted(SCENES))
def test_a_whole_frame_is_within_the_bound_and_the_pass_reads_only(pkg, oracle, gpu, kind):
    n, w, h = SCENES[kind]
    verts, ref, vals, want = _reference(pkg, oracle, kind)
    assert (want["terms"] > 2).sum() > 300 and want["terms"].max() > 256    # sums that meet in every layer: DPP, LDS, device
    gs, rend = _open(pkg, kind)
    try:
        u = _uniforms(pkg, kind)
        before, _ = rend.render_host(u)
        assert_images_identical(before, ref["image"], label=f"kind {kind}")
        sums = _run(rend, vals, want, n, f"kind {kind}")
        # channel 2 of the values is 1: its lift is the weight, term for term (both within the weight's bound of the exact sum)
        assert (np.abs(sums.get("out")[:, 2] - sums.get("weight")) <= 2.0 * want["terms"] * U53 * want["abs_weight"]).all()
        rend.lift_pixels(_values_tensor(vals), **sums.t)                   # a second call into the same arrays: twice the sums
        _assert_close(sums, want, f"kind {kind}, second call into the same arrays", times=2)
        _run(rend, vals, want, n, f"kind {kind}, arrays preloaded with 1.0", preload=1.0)
        compare_stages(pkg, rend, u, ref)                   # the taps of the frame the pass walked are intact
        after, _ = rend.render_host(u)
        assert np.array_equal(after.view(np.uint32), before.view(np.uint32)), "a frame rendered after the pass differs"
        compare_stages(pkg, rend, u, ref)
    finally:
        rend.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ 2. at most two terms: exact
PAIRS = {"one pixel": [(20, 12)],
         "two lanes of one wave": [(3, 5), (4, 5)],                 # one 8 x 8 quadrant: the DPP sum
         "two lanes in two rows of 16": [(3, 1), (3, 2)],           # lanes 11 and 19: the sum across the wave's rows
         "two waves of one tile": [(7, 5), (8, 5)],                 # two quadrants of tile 0: the LDS slot
         "two tiles": [(15, 5), (16, 5)],                           # the device atomic
         "last row of the partial tiles": [(35, 39), (36, 39)],     # 72 x 40: tiles of rows 32 .. 39 only
         "last row, two partial tiles": [(47, 39), (48, 39)],
         "last column and corner": [(71, 38), (71, 39)]}            # tiles of columns 64 .. 71 only


@pytest.mark.parametrize("name", list(PAIRS))
def test_one_or_two_counted_pixels_give_the_reference_bit_for_bit(pkg, oracle, gpu, name):
    kind = "A"
    n, w, h = SCENES[kind]
    _, ref, vals, whole = _reference(pkg, oracle, kind)
    mask = np.zeros((h, w), np.uint8)
    for x, y in PAIRS[name]:
        assert whole["blended"][y, x] >= 3, (name, x, y)
        mask[y, x] = 200
    want = lref.lift(oracle, ref, w, h, vals, mask)
    assert want["terms"].max() == len(PAIRS[name]) and want["terms"].sum() == sum(whole["blended"][y, x] for x, y in PAIRS[name])
    if len(PAIRS[name]) == 2:
        assert (want["terms"] == 2).sum() >= 3, f"{name}: the two pixels share too few blended Gaussians"
    gs, rend = _open(pkg, kind)
    try:
        rend.render_host(_uniforms(pkg, kind))
        _run(rend, vals, want, n, name, mask=mask, check=_assert_bits)
        _run(rend, np.ascontiguousarray(vals[..., :3]), want, n, f"{name}, 3 channels", mask=mask, check=_assert_bits)   # the kernel of four
        full = np.ascontiguousarray(_reference(pkg, oracle, kind, channels=2 * G + 5)[2])
        wide = lref.lift(oracle, ref, w, h, full, mask)                # whole groups and a short one
        _run(rend, full, wide, n, f"{name}, {2 * G + 5} channels", mask=mask, check=_assert_bits)
    finally:
        rend.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ 3. list lengths around the chunks
def _limit_frame(pkg, oracle, rec, w, h):
    _, u_ref, ref = oracle_frame(oracle, rec, w, h)
    gs = pkg.Scene.from_records(rec, device=0)
    rend = pkg.Renderer(gs)
    u = pkg.camera_uniforms(pkg.make_camera(), w, h)
    assert u.tobytes() == u_ref.tobytes()
    return gs, rend, u, ref


@pytest.mark.parametrize("k", [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1])
def test_lists_that_end_around_one_and_two_chunks(pkg, oracle, gpu, k):
    sc = ls.blend_chunk(k)
    gs, rend, u, ref = _limit_frame(pkg, oracle, sc.records, sc.width, sc.height)
    try:
        assert len(_tile_list(ref, sc.width, (2, 1))) == k
        vals = _values(sc.height, sc.width, 5)
        want = lref.lift(oracle, ref, sc.width, sc.height, vals)
        assert (want["terms"] != 0).sum() == len(sc.records)    # no pixel stops early: every entry of both lists is blended somewhere
        rend.render_host(u)
        _run(rend, vals, want, len(sc.records), f"list of {k}")
    finally:
        rend.close()
        gs.close()


def test_nan_values_at_uncounted_pixels_and_in_tiles_with_empty_lists_reach_no_output(pkg, oracle, gpu):
    sc = ls.blend_chunk(CHUNK + 1)
    w, h = sc.width, sc.height
    gs, rend, u, ref = _limit_frame(pkg, oracle, sc.records, w, h)
    try:
        b = ref["boundaries"].astype(np.int64).reshape(-1, 2)
        tx = (w + 15) // 16
        empty = np.zeros((h, w), bool)
        for t in np.nonzero(b[:, 1] == b[:, 0])[0]:
            empty[16 * (t // tx):16 * (t // tx) + 16, 16 * (t % tx):16 * (t % tx) + 16] = True
        assert empty.sum() >= 10 * 256
        mask = np.ones((h, w), np.uint8)
        listed = np.argwhere(~empty)
        mask[listed[::3, 0], listed[::3, 1]] = 0                    # a third of the pixels whose tile has a list: not counted
        vals = _values(h, w, G + 1)
        want = lref.lift(oracle, ref, w, h, vals, mask)
        assert (want["terms"] > 0).sum() > CHUNK and np.isfinite(want["out"]).all()
        poisoned = vals.copy()
        poisoned[empty] = np.nan                                    # counted, but there is no entry to blend
        poisoned[mask == 0] = np.nan                                # not counted: never read
        rend.render_host(u)
        sums = _run(rend, poisoned, want, len(sc.records), "NaN values", mask=mask)
        assert np.isfinite(sums.get("out")).all() and np.isfinite(sums.get("weight")).all()
    finally:
        rend.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ 4. saturation, grazing inputs
@pytest.mark.parametrize("quadrant", [0, 3])
@pytest.mark.parametrize("chunk", [1, 2])
def test_a_quadrant_that_saturates_mid_list_while_the_rest_walk_on(pkg, oracle, gpu, chunk, quadrant):
    """More than five chunks; one 8 x 8 block of pixels has saturated by the end of `chunk`, the other three quadrants walk the
    whole list: the wave that is done stays for the barriers and the flush and adds nothing more.  Then through a mask that
    counts that block alone: entries behind its last break get nothing."""
    rec, w, h = _saturated_quadrant(chunk, quadrant)
    gs, rend, u, ref = _limit_frame(pkg, oracle, rec, w, h)
    try:
        ids = _tile_list(ref, w, (1, 1))
        assert len(ids) > 5 * CHUNK
        vals = _values(h, w, 5)
        want = lref.lift(oracle, ref, w, h, vals)
        rend.render_host(u)
        _run(rend, vals, want, len(rec), f"quadrant {quadrant} saturates in chunk {chunk}")
        mask = np.zeros((h, w), np.uint8)
        y0, x0 = 16 + 8 * (quadrant >> 1), 16 + 8 * (quadrant & 1)
        mask[y0:y0 + 8, x0:x0 + 8] = 1
        want_q = lref.lift(oracle, ref, w, h, vals, mask)
        behind = ids[CHUNK * (chunk + 1):]
        assert (want_q["terms"][behind] == 0).all() and (want["terms"][behind] > 0).any()
        assert (want_q["terms"][ids[:CHUNK * chunk]] > 0).any()
        _run(rend, vals, want_q, len(rec), f"quadrant {quadrant} alone", mask=mask)
    finally:
        rend.close()
        gs.close()


def test_grazing_splats_and_cancelling_needles(pkg, oracle, gpu):
    """Alpha within 1e-6 .. 1e-1 of 1/255 on either side at a quadrant's edge and corner pixels, and 45-degree needles whose
    `power` terms cancel: where a cull or a reordered product would flip which pixels a Gaussian is lifted from."""
    rec, w, h, n_graze, n_needle, _ = _grazing_scene()
    gs, rend, u, ref = _limit_frame(pkg, oracle, rec, w, h)
    try:
        vals = _values(h, w, 5)
        want = lref.lift(oracle, ref, w, h, vals)
        assert (want["terms"][:n_graze] != 0).sum() > n_graze // 4 and (want["terms"][n_graze:n_graze + n_needle] != 0).sum() > n_needle // 2
        rend.render_host(u)
        _run(rend, vals, want, len(rec), "grazing splats")
    finally:
        rend.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ 5. channel groups, masks
def test_channel_counts_and_single_outputs(pkg, oracle, gpu):
    kind = "A"
    n, w, h = SCENES[kind]
    _, ref, vals, want = _reference(pkg, oracle, kind, channels=2 * G + 5)   # (channel sums are independent: a prefix of the
    gs, rend = _open(pkg, kind)                                              #  channels lifts to the same prefix of the reference)
    try:
        rend.render_host(_uniforms(pkg, kind))
        assert (G, SMALL) == (16, 4)                              # (the issue's cases 1, 3, G - 1 .. 2 G + 5, and every path's edge)
        for channels in (1, 3, SMALL, SMALL + 1, G - 1, G, G + 1, G + SMALL, 2 * G + 5):  # (a last group of 1 .. SMALL runs the small kernel)
            # (out is dense: a write past a Gaussian's row lands in the next row or the guard words, a read past a pixel's row
            #  brings the next pixel's values in; either is outside the bound)
            _run(rend, np.ascontiguousarray(vals[..., :channels]), want, n, f"{channels} channels")
        _run(rend, None, want, n, "no channels: the weights alone")
        _run(rend, np.ascontiguousarray(vals[..., :G + 1]), want, n, "out alone", only=("out",))
        # sums allocated by the wrapper
        got = rend.lift_pixels(_values_tensor(np.ascontiguousarray(vals[..., :3])), out=True, weight=True)
        assert got["out"].dtype == torch.float64 and tuple(got["out"].shape) == (n, 3) and tuple(got["weight"].shape) == (n,)
        assert (np.abs(got["out"].cpu().numpy() - want["out"][:, :3]) <= 2.0 * want["terms"][:, None] * U53 * want["A"][:, :3]).all()
        assert (np.abs(got["weight"].cpu().numpy() - want["weight"]) <= 2.0 * want["terms"] * U53 * want["abs_weight"]).all()
        assert rend.lift_pixels(None) == {}                       # nothing asked for: a no-op after the drain
        # channels == 0 with out given: that output is not touched (the C entry point; the wrapper does not build this)
        import ctypes as C
        out_only, weight_only = Sums(n, 3, only=("out",)), Sums(n, 0, only=("weight",))
        l = pkg.binding.PixelLift(channels=0, out=out_only.t["out"].data_ptr(), out_weight=weight_only.t["weight"].data_ptr())
        assert pkg.binding.lib().gs_lift_pixels(rend._h, C.byref(l)) == 0
        rend.synchronize()
        out_only.guards_intact()
        assert (out_only.get("out") == 0).all()
        _assert_close(weight_only, want, "channels == 0 through the C entry point")
    finally:
        rend.close()
        gs.close()


def test_masks(pkg, oracle, gpu):
    kind = "A"
    n, w, h = SCENES[kind]
    _, ref, vals, whole = _reference(pkg, oracle, kind)
    gs, rend = _open(pkg, kind)
    try:
        rend.render_host(_uniforms(pkg, kind))
        random = (np.random.default_rng(7).random((h, w)) < 0.4).astype(np.uint8) * 3     # any nonzero value counts
        quadrant = np.zeros((h, w), np.uint8)
        quadrant[24:32, 40:48] = 1                                                        # one wave of one tile
        ragged = np.zeros((h, w), np.uint8)
        ragged[33:, 60:] = 1                                                              # inside the partial tiles of the last row and column
        got = {}
        for name, mask, dtype in (("random", random, torch.uint8), ("one quadrant", quadrant, torch.uint8),
                                  ("ragged corner", ragged, torch.uint8), ("random as bool", random, torch.bool),
                                  ("complement", random == 0, torch.bool)):
            want = lref.lift(oracle, ref, w, h, vals, mask)
            assert want["terms"].sum() > 0
            got[name] = _run(rend, vals, want, n, f"mask: {name}", mask=mask, mask_dtype=dtype)
        # a mask and its complement sum to the unmasked result, within its bound
        for name in ("out", "weight"):
            total, terms, mag = _want(whole, name, 5)
            both = got["random"].get(name) + got["complement"].get(name)
            assert (np.abs(both - total) <= 2.0 * (terms + 1) * U53 * mag).all(), name
        # an all-zero mask: the arrays keep the bits they held
        _run(rend, vals, lref.lift(oracle, ref, w, h, vals, np.zeros((h, w), np.uint8)), n, "mask: all zero", mask=np.zeros((h, w), np.uint8),
             preload=77.5)
    finally:
        rend.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ 6. the blend's switches
@pytest.mark.parametrize("kind", sorted(SCENES))
def test_the_pass_does_not_depend_on_how_the_frame_was_blended(pkg, oracle, gpu, kind):
    n, w, h = SCENES[kind]
    _, _, vals, want = _reference(pkg, oracle, kind)
    gs, rend = _open(pkg, kind)
    try:
        u = _uniforms(pkg, kind)
        settings = [("exp mode 3", lambda: rend.set_exp_mode(3)), ("contraction on", lambda: rend.set_blend_contraction(True)),
                    ("lockstep 0", lambda: rend.set_blend_lockstep(0)), ("lockstep 1", lambda: rend.set_blend_lockstep(1)),
                    ("exp mode 0, contracted, lockstep 1", lambda: rend.set_exp_mode(0))]
        for label, apply in settings:                        # (cumulative: each frame is blended with one more switch moved)
            apply()
            rend.render_host(u)
            _run(rend, vals, want, n, f"kind {kind}, {label}")
    finally:
        rend.close()
        gs.close()


def test_the_antialiased_mode_is_followed_through_the_records(pkg, oracle, gpu):
    """With set_antialiased(True) the records carry opacity' and its cut: the pass equals the reference run on the scene S' that
    holds the frame's opacity' (the recipe of test_gpu_contributions)."""
    kind = "T"
    n, w, h = SCENES[kind]
    verts, _, vals, plain = _reference(pkg, oracle, kind)
    gs, rend = _open(pkg, kind)
    try:
        u = _uniforms(pkg, kind)
        rend.set_antialiased(True)
        img, _ = rend.render_host(u)
        vis = rend.stage("tiles") != 0
        prime = verts.copy()
        prime["scale_opacity"][vis, 3] = rend.stage("conic_opacity").reshape(-1, 4)[vis, 3]
        ref = oracle.stages(prime, u.view(oracle.UNIFORMS_DT))
        assert_images_identical(img, ref["image"], label="antialiased")
        want = lref.lift(oracle, ref, w, h, vals)
        assert not np.array_equal(want["weight"], plain["weight"])
        _run(rend, vals, want, n, "antialiased")
    finally:
        rend.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ 7. which frame, which ids
@pytest.mark.parametrize("graph", [False, True], ids=["launches", "graph"])
def test_with_frames_in_flight_the_pass_lifts_the_last_one(pkg, oracle, gpu, graph):
    kind = "A"
    n, w, h = SCENES[kind]
    refs = [_reference(pkg, oracle, kind, cam) for cam in range(3)]
    assert not np.array_equal(refs[1][3]["terms"], refs[2][3]["terms"])
    gs, rend = _open(pkg, kind)
    try:
        rend.set_graph_mode(graph)
        rend.set_frames_in_flight(3)
        for round_ in range(2):                              # (the second round replays the captured graphs)
            order = [0, 1, 2] if round_ == 0 else [2, 0, 1]
            targets = [torch.zeros((h, w, 4), dtype=torch.float32, device="cuda") for _ in order]
            for cam, t in zip(order, targets):
                rend.render(_uniforms(pkg, kind, cam), t.data_ptr(), 0)
            _run(rend, refs[order[-1]][2], refs[order[-1]][3], n, f"graph {graph}, cameras {order}")
            for cam, t in zip(order, targets):
                assert np.array_equal(t.cpu().numpy().view(np.uint32), refs[cam][1]["image"].view(np.uint32))
    finally:
        rend.close()
        gs.close()


def test_a_scene_read_in_spatial_order_lifts_to_scene_ids(pkg, oracle, gpu, monkeypatch):
    kind = "T"
    n, w, h = SCENES[kind]
    _, _, vals, want = _reference(pkg, oracle, kind)
    monkeypatch.setenv("GS_SPATIAL_MIN", "1")                # the scene gets its copy in spatial order at 1 500 Gaussians
    gs, rend = _open(pkg, kind)
    try:
        assert not np.array_equal(ls.morton_order(_records(pkg, kind)[:, :3]), np.arange(n))
        rend.render_host(_uniforms(pkg, kind))
        _run(rend, vals, want, n, "spatial order")
    finally:
        rend.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_before_any_frame_the_call_is_refused(pkg, gpu):
    gs, rend = _open(pkg, "A")
    try:
        with pytest.raises(pkg.binding.GsError) as e:
            rend.lift_pixels(None)
        assert e.value.code == -1 and "no frame" in str(e.value)
        with pytest.raises(pkg.binding.GsError) as e:
            rend.lift_pixels(None, weight=True)
        assert e.value.code == -1 and "no frame" in str(e.value)
    finally:
        rend.close()
        gs.close()


def test_misaligned_pointers_are_refused_and_nothing_is_written(pkg, gpu):
    import ctypes as C
    kind = "A"
    n, w, h = SCENES[kind]
    gs, rend = _open(pkg, kind)
    try:
        rend.render_host(_uniforms(pkg, kind))
        big = torch.zeros(3 * n + 8, dtype=torch.float64, device="cuda")
        vals = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        L = pkg.binding.lib()
        for member, offset in (("out", 4), ("out_weight", 4), ("values", 2)):
            l = pkg.binding.PixelLift(values=vals.data_ptr(), channels=3, out=big.data_ptr(), out_weight=big.data_ptr())
            setattr(l, member, getattr(l, member) + offset)
            assert L.gs_lift_pixels(rend._h, C.byref(l)) == -1, member
        assert (big == 0).all()
    finally:
        rend.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ 9. the adjoint of feature_maps
def test_the_lift_is_the_transpose_of_feature_maps_on_the_device(pkg, oracle, gpu):
    """<feature_maps(f), v> = <f, lift_pixels(v)> within 2 (m_max + 3) 2^-24 sum |f w v| (tests/test_lift_api.py derives the
    bound), m_max and the magnitudes from the reference; and through differentiable_feature_maps the gradient of <out, v> is
    lift_pixels(v) rounded to float32."""
    kind = "A"
    n, w, h = SCENES[kind]
    _, ref, vals, want = _reference(pkg, oracle, kind)
    f = np.random.default_rng(31).standard_normal((n, 5)).astype(np.float32)
    gs, rend = _open(pkg, kind)
    try:
        rend.render_host(_uniforms(pkg, kind))
        ft, vt = torch.as_tensor(f).cuda(), torch.as_tensor(np.array(vals)).cuda()
        fwd = rend.feature_maps(features=ft, out=True)["out"]
        lifted = rend.lift_pixels(vt, out=True)["out"]
        lhs = float((fwd.double() * vt.double()).sum())
        rhs = float((ft.double() * lifted).sum())
        bound = 2 * (int(want["blended"].max()) + 3) * U24 * float((np.abs(f.astype(np.float64)) * want["A"]).sum())
        print(f"<Bf, v> = {lhs!r}, <f, B'v> = {rhs!r}, difference {abs(lhs - rhs):.3g}, bound {bound:.3g}")
        assert abs(lhs - rhs) <= bound
        fg = ft.clone().requires_grad_(True)
        out = rend.differentiable_feature_maps(fg)
        assert torch.equal(out.detach(), fwd)
        (grad,) = torch.autograd.grad((out * vt).sum(), fg)
        assert grad.dtype == torch.float32 and tuple(grad.shape) == (n, 5) and grad.is_cuda
        # The gradient is lift_pixels(v) rounded to float32 -- of the backward's OWN call.  Equality with the separate call above
        # cannot be asserted: the order of the binary64 adds is open, two calls need not give the same bits, and a last-bit
        # difference can cross a binary32 rounding boundary.  What the definition fixes is asserted: the gradient is one binary32
        # rounding (half an ulp) away from a value within lift_pixels' summation bound of this call's.
        g64, l64 = grad.double().cpu().numpy(), lifted.cpu().numpy()
        half_ulp = np.abs(l64) * U24
        assert (np.abs(g64 - l64) <= half_ulp + 2.0 * want["terms"][:, None] * U53 * want["A"]).all()
        assert (g64[want["terms"] == 0] == 0).all()
        out = rend.differentiable_feature_maps(fg)
        rend.render_host(_uniforms(pkg, kind, 1))           # another frame: the backward of the old forward is refused
        with pytest.raises(RuntimeError, match="frame"):
            torch.autograd.grad((out * vt).sum(), fg)
    finally:
        rend.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ 10. the caller's stream
def _queue_filler(passes=64):
    """Several milliseconds of work queued on torch's current stream (elementwise passes over 256 MiB); returns at once."""
    big = torch.ones(64 << 20, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for _ in range(passes):
        big.mul_(1.0000001)
    return big


def _within(got, want, name, channels, label):
    total, terms, mag = _want(want, name, channels)
    bad = np.argwhere(~(np.abs(got - total) <= 2.0 * terms * U53 * mag))
    assert len(bad) == 0, f"{label}: {name} is outside the bound at {len(bad)} place(s), first {tuple(bad[0])}: {got[tuple(bad[0])]!r} against {total[tuple(bad[0])]!r}"


def test_producers_still_queued_on_torchs_stream_are_complete_before_the_pass(pkg, oracle, gpu):
    """The pass runs on the renderer's own non-blocking stream.  values are written, and the sums zeroed, by kernels queued on
    torch's stream BEHIND milliseconds of other work, immediately before the call: the pass must read the final values and its
    sums must not be wiped by a late fill."""
    kind = "A"
    n, w, h = SCENES[kind]
    _, ref, vals, want = _reference(pkg, oracle, kind)
    gs, rend = _open(pkg, kind)
    try:
        rend.render_host(_uniforms(pkg, kind))
        final = torch.as_tensor(np.array(vals)).cuda()
        values = torch.full_like(final, float("nan"))
        out = torch.full((n, 5), 123.0, dtype=torch.float64, device="cuda")
        keep = _queue_filler()
        values.copy_(final)                                  # the producer of values, behind the filler
        out.zero_()                                          # the caller's own zeroing, behind both
        got = rend.lift_pixels(values, out=out, weight=True)  # (weight=True: the wrapper's zeros, behind all three)
        _within(out.cpu().numpy(), want, "out", 5, "values and zeros queued behind a filler")
        _within(got["weight"].cpu().numpy(), want, "weight", 0, "values and zeros queued behind a filler")
        values.fill_(float("nan"))
        torch.cuda.synchronize()
        keep = _queue_filler()
        values.copy_(final)
        got = rend.lift_pixels(values, out=True)
        _within(got["out"].cpu().numpy(), want, "out", 5, "out=True behind a filler")
        del keep
    finally:
        rend.close()
        gs.close()


def test_a_backward_and_a_forward_behind_queued_work_see_complete_tensors(pkg, oracle, gpu):
    """differentiable_feature_maps in a loop: the features are written (an optimizer step) and the incoming gradient is produced
    by kernels queued on torch's stream behind other work; forward and backward must see them complete."""
    kind = "A"
    n, w, h = SCENES[kind]
    _, ref, vals, want = _reference(pkg, oracle, kind)
    f = np.random.default_rng(31).standard_normal((n, 5)).astype(np.float32)
    gs, rend = _open(pkg, kind)
    try:
        rend.render_host(_uniforms(pkg, kind))
        ft, vt = torch.as_tensor(f).cuda(), torch.as_tensor(np.array(vals)).cuda()
        fwd = rend.feature_maps(features=ft, out=True)["out"]
        lifted = rend.lift_pixels(vt, out=True)["out"].cpu().numpy()
        fg = torch.full_like(ft, float("nan")).requires_grad_(True)
        torch.cuda.synchronize()
        keep = _queue_filler()
        fg.data.copy_(ft)                                    # the step that writes the features, behind the filler
        out = rend.differentiable_feature_maps(fg)
        assert torch.equal(out.detach(), fwd), "the forward read features that were not complete"
        keep = _queue_filler()
        (grad,) = torch.autograd.grad((out * vt).sum(), fg)  # grad of out = vt, produced by a kernel behind the filler
        g64 = grad.double().cpu().numpy()
        assert np.isfinite(g64).all()
        assert (np.abs(g64 - lifted) <= np.abs(lifted) * U24 + 2.0 * want["terms"][:, None] * U53 * want["A"]).all(), \
            "the backward lifted a gradient that was not complete, or its sums were wiped"
        assert (g64[want["terms"] > 0] != 0).any()
        del keep
    finally:
        rend.close()
        gs.close()
