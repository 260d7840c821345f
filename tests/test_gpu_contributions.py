"""gs_accumulate_contributions on the device (gs_contrib.hip) against its definition restated in numpy
(tests/contribution_reference.py, pinned to the oracle's image by tests/test_contributions_api.py).  Everything the pass
computes is an integer defined by the reference's binary32 arithmetic: every comparison here is EXACT equality -- weight as
uint64, pixels and top_id as uint32 -- with no tolerance and no case left out.  Renderers start in exp mode 2 (conftest); every
test runs on both depth-order paths."""
import numpy as np
import pytest
import torch  # at collection, before the package loads its library: both must bind the same HIP runtime

import contribution_reference as cref
import limit_scenes as ls
from helpers import assert_images_identical, compare_stages, oracle_frame
from test_gpu_blend_chunk_loop import _grazing_scene, _saturated_quadrant, _tile_list

pytestmark = pytest.mark.gpu

CHUNK = 64                                            # gs_contrib.hip: entries staged per chunk
SCENES = {"A": (600, 72, 40), "T": (1500, 64, 64)}    # synth_records(n, seed=5, kind) at width x height; 72 x 40 = 4.5 x 2.5 tiles
CAMERAS = [{}, dict(position=(0.3, -0.2, 0.5)), dict(position=(-0.25, 0.1, 0.3))]
_cache = {}


def _records(pkg, kind):
    return pkg.synth.synth_records(SCENES[kind][0], seed=5, kind=kind)


def _reference(pkg, oracle, kind, cam=0):
    """(verts, oracle stages, reference contributions) of a synthetic scene seen by CAMERAS[cam]: computed once, never changed."""
    key = (kind, cam)
    if key not in _cache:
        _, w, h = SCENES[kind]
        verts, _, ref = oracle_frame(oracle, _records(pkg, kind), w, h, oracle.default_camera(**CAMERAS[cam]))
        want = cref.contributions(oracle, ref, w, h)
        for a in want.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[key] = (verts, ref, want)
    return _cache[key]


def _uniforms(pkg, kind, cam=0):
    _, w, h = SCENES[kind]
    return pkg.camera_uniforms(pkg.make_camera(**CAMERAS[cam]), w, h)


class Arrays:
    """The three outputs as torch tensors on the device, preloaded; read back as the unsigned integers the C ABI defines."""

    def __init__(self, n, h, w, weight0=0, pixels0=0, only=("weight", "pixels", "top_id")):
        self.t = {}
        if "weight" in only:
            self.t["weight"] = torch.full((n,), int(weight0), dtype=torch.int64, device="cuda")
        if "pixels" in only:
            self.t["pixels"] = torch.full((n,), int(np.uint32(pixels0).view(np.int32)), dtype=torch.int32, device="cuda")
        if "top_id" in only:
            self.t["top_id"] = torch.full((h, w), 12345, dtype=torch.int32, device="cuda")

    def get(self, name):
        a = self.t[name].cpu().numpy()
        return a.view(np.uint64 if name == "weight" else np.uint32)


def _mask_tensor(mask, dtype=None):
    return None if mask is None else torch.as_tensor(np.ascontiguousarray(mask), dtype=dtype or torch.uint8).cuda().contiguous()


def _assert_equal(arrays, want, label, weight0=0, pixels0=0):
    for name in arrays.t:
        w = want[name]
        if name == "weight":
            w = w + np.uint64(weight0)
        if name == "pixels":
            w = w + np.uint32(pixels0)      # (modulo 2^32, as the device adds)
        got = arrays.get(name)
        bad = np.argwhere(got != w)
        assert len(bad) == 0, f"{label}: {name} differs at {len(bad)} place(s), first {tuple(bad[0])}: {got[tuple(bad[0])]} != {w[tuple(bad[0])]}"


def _open(pkg, kind):
    gs = pkg.Scene.from_records(_records(pkg, kind), device=0)
    return gs, pkg.Renderer(gs)


# ------------------------------------------------------------------------------------------------ 1. whole frame
@pytest.mark.parametrize("kind", sorted(SCENES))
def test_a_whole_frame_equals_the_reference_and_the_pass_reads_only(pkg, oracle, gpu, kind):
    n, w, h = SCENES[kind]
    verts, ref, want = _reference(pkg, oracle, kind)
    assert (want["pixels"] != 0).sum() > 300
    gs, rend = _open(pkg, kind)
    try:
        u = _uniforms(pkg, kind)
        before, _ = rend.render_host(u)
        assert_images_identical(before, ref["image"], label=f"kind {kind}")
        out = Arrays(n, h, w)
        rend.contributions(**out.t)
        _assert_equal(out, want, f"kind {kind}")
        again = Arrays(n, h, w)
        rend.contributions(**again.t)                       # integer sums: two runs give the same bits
        _assert_equal(again, want, f"kind {kind}, second call")
        compare_stages(pkg, rend, u, ref)                   # the taps of the frame the pass walked are intact
        after, _ = rend.render_host(u)
        assert np.array_equal(after.view(np.uint32), before.view(np.uint32)), "a frame rendered after the pass differs"
        compare_stages(pkg, rend, u, ref)
    finally:
        rend.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ 2. list lengths around the chunks
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
        want = cref.contributions(oracle, ref, sc.width, sc.height)
        assert (want["pixels"] != 0).sum() == len(sc.records)    # no pixel stops early: every entry of both lists is blended somewhere
        rend.render_host(u)
        out = Arrays(len(sc.records), sc.height, sc.width)
        rend.contributions(**out.t)
        _assert_equal(out, want, f"list of {k}")
    finally:
        rend.close()
        gs.close()


@pytest.mark.parametrize("quadrant", [0, 3])
@pytest.mark.parametrize("chunk", [1, 2])
def test_a_quadrant_that_saturates_mid_list_while_the_rest_walk_on(pkg, oracle, gpu, chunk, quadrant):
    """More than five chunks; one 8 x 8 block of pixels has saturated by the end of `chunk`, the other three quadrants walk the
    whole list.  Through a mask that counts that block alone: entries behind its last break get nothing from it."""
    rec, w, h = _saturated_quadrant(chunk, quadrant)
    gs, rend, u, ref = _limit_frame(pkg, oracle, rec, w, h)
    try:
        ids = _tile_list(ref, w, (1, 1))
        assert len(ids) > 5 * CHUNK
        want = cref.contributions(oracle, ref, w, h)
        rend.render_host(u)
        out = Arrays(len(rec), h, w)
        rend.contributions(**out.t)
        _assert_equal(out, want, f"quadrant {quadrant} saturates in chunk {chunk}")
        mask = np.zeros((h, w), np.uint8)
        y0, x0 = 16 + 8 * (quadrant >> 1), 16 + 8 * (quadrant & 1)
        mask[y0:y0 + 8, x0:x0 + 8] = 1
        want_q = cref.contributions(oracle, ref, w, h, mask)
        behind = ids[CHUNK * (chunk + 1):]
        assert (want_q["pixels"][behind] == 0).all() and (want["pixels"][behind] > 0).any()
        assert (want_q["pixels"][ids[:CHUNK * chunk]] > 0).any()
        out_q = Arrays(len(rec), h, w)
        rend.contributions(mask=_mask_tensor(mask), **out_q.t)
        _assert_equal(out_q, want_q, f"quadrant {quadrant} alone")
        assert (out_q.get("pixels")[behind] == 0).all() and (out_q.get("weight")[behind] == 0).all()
    finally:
        rend.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ 3. grazing and cancelling inputs
def test_grazing_splats_and_cancelling_needles(pkg, oracle, gpu):
    """Alpha within 1e-6 .. 1e-1 of 1/255 on either side at a quadrant's edge and corner pixels, and 45-degree needles whose
    `power` terms cancel: where a cull or a reordered product would flip a count."""
    rec, w, h, n_graze, n_needle, _ = _grazing_scene()
    gs, rend, u, ref = _limit_frame(pkg, oracle, rec, w, h)
    try:
        want = cref.contributions(oracle, ref, w, h)
        assert (want["pixels"][:n_graze] != 0).sum() > n_graze // 4 and (want["pixels"][n_graze:n_graze + n_needle] != 0).sum() > n_needle // 2
        rend.render_host(u)
        out = Arrays(len(rec), h, w)
        rend.contributions(**out.t)
        _assert_equal(out, want, "grazing splats")
    finally:
        rend.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ 4. the mask
def test_masks(pkg, oracle, gpu):
    kind = "A"
    n, w, h = SCENES[kind]
    _, ref, whole = _reference(pkg, oracle, kind)
    gs, rend = _open(pkg, kind)
    try:
        rend.render_host(_uniforms(pkg, kind))
        rect = np.zeros((h, w), np.uint8)
        rect[5:29, 11:43] = 7                                # aligned to neither tiles nor 8 x 8 blocks; any nonzero value counts
        single = np.zeros((h, w), np.uint8)
        ys, xs = np.nonzero(whole["top_id"] != cref.NONE)
        single[ys[len(ys) // 2], xs[len(xs) // 2]] = 1       # one pixel, one that blends something
        ragged = np.zeros((h, w), np.uint8)
        ragged[33:, 60:] = 1                                 # inside the partial tiles of the last row and column
        got = {}
        for name, mask, dtype in (("rectangle", rect, None), ("single pixel", single, None), ("ragged corner", ragged, None),
                                  ("rectangle as bool", rect != 0, torch.bool), ("complement", rect == 0, torch.bool)):
            want = cref.contributions(oracle, ref, w, h, mask)
            assert want["blended"] > 0
            out = Arrays(n, h, w)
            rend.contributions(mask=_mask_tensor(mask, dtype), **out.t)
            _assert_equal(out, want, f"mask: {name}")
            got[name] = out
        assert int(got["single pixel"].get("pixels").sum()) == int((got["single pixel"].get("pixels") != 0).sum()) > 0
        assert (got["single pixel"].get("top_id") != cref.NONE).sum() == 1
        # a mask and its complement sum to the unmasked result
        for name in ("weight", "pixels"):
            np.testing.assert_array_equal(got["rectangle"].get(name) + got["complement"].get(name), whole[name])
        np.testing.assert_array_equal(np.where(rect != 0, got["rectangle"].get("top_id"), got["complement"].get("top_id")), whole["top_id"])
        # an all-zero mask: the sums stay what they were, top_id is all "nothing"
        out = Arrays(n, h, w, weight0=77, pixels0=5)
        rend.contributions(mask=_mask_tensor(np.zeros((h, w), np.uint8)), **out.t)
        assert (out.get("weight") == 77).all() and (out.get("pixels") == 5).all() and (out.get("top_id") == cref.NONE).all()
    finally:
        rend.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ 5. accumulation
def test_accumulation_over_views_preloaded_arrays_and_single_outputs(pkg, oracle, gpu):
    kind = "A"
    n, w, h = SCENES[kind]
    wants = [_reference(pkg, oracle, kind, cam)[2] for cam in (0, 1)]
    assert not np.array_equal(wants[0]["pixels"], wants[1]["pixels"])
    gs, rend = _open(pkg, kind)
    try:
        both = Arrays(n, h, w)
        for cam in (0, 1):
            rend.render_host(_uniforms(pkg, kind, cam))
            rend.contributions(**both.t)
        total = dict(weight=wants[0]["weight"] + wants[1]["weight"], pixels=wants[0]["pixels"] + wants[1]["pixels"],
                     top_id=wants[1]["top_id"])             # top_id is overwritten: the last view's
        _assert_equal(both, total, "two cameras")
        # the carry into the high word of weight; pixels across its sign bit as an int32 tensor
        w0, p0 = 2 ** 32 - 1, 2 ** 31 - 1
        pre = Arrays(n, h, w, weight0=w0, pixels0=p0)
        rend.contributions(**pre.t)
        _assert_equal(pre, wants[1], "preloaded", weight0=w0, pixels0=p0)
        assert (pre.get("weight") >> np.uint64(32) != 0).sum() == (wants[1]["pixels"] != 0).sum() > 300
        for name in ("weight", "pixels", "top_id"):
            one = Arrays(n, h, w, only=(name,))
            rend.contributions(**one.t)
            _assert_equal(one, wants[1], f"{name} alone")
        rend.contributions()                                 # all three null: a no-op after the drain
    finally:
        rend.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ 6. the blend's switches
@pytest.mark.parametrize("kind", sorted(SCENES))
def test_the_pass_does_not_depend_on_how_the_frame_was_blended(pkg, oracle, gpu, kind):
    n, w, h = SCENES[kind]
    _, _, want = _reference(pkg, oracle, kind)
    gs, rend = _open(pkg, kind)
    try:
        u = _uniforms(pkg, kind)
        settings = [("exp mode 3", lambda: rend.set_exp_mode(3)), ("contraction on", lambda: rend.set_blend_contraction(True)),
                    ("lockstep 0", lambda: rend.set_blend_lockstep(0)), ("lockstep 1", lambda: rend.set_blend_lockstep(1)),
                    ("exp mode 0, contracted, lockstep 1", lambda: rend.set_exp_mode(0))]
        for label, apply in settings:                        # (cumulative: each frame is blended with one more switch moved)
            apply()
            rend.render_host(u)
            out = Arrays(n, h, w)
            rend.contributions(**out.t)
            _assert_equal(out, want, f"kind {kind}, {label}")
    finally:
        rend.close()
        gs.close()


def test_the_antialiased_mode_is_followed_through_the_records(pkg, oracle, gpu):
    """With set_antialiased(True) the records carry opacity' and its cut: the pass equals the reference run on the scene S' that
    holds the frame's opacity' (the recipe of test_the_quadrant_test_with_the_antialiased_opacity)."""
    kind = "T"
    n, w, h = SCENES[kind]
    verts, _, plain = _reference(pkg, oracle, kind)
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
        want = cref.contributions(oracle, ref, w, h)
        assert not np.array_equal(want["weight"], plain["weight"])
        out = Arrays(n, h, w)
        rend.contributions(**out.t)
        _assert_equal(out, want, "antialiased")
    finally:
        rend.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ 7. which frame
@pytest.mark.parametrize("graph", [False, True], ids=["launches", "graph"])
def test_with_frames_in_flight_the_pass_reports_the_last_one(pkg, oracle, gpu, graph):
    kind = "A"
    n, w, h = SCENES[kind]
    wants = [_reference(pkg, oracle, kind, cam)[2] for cam in range(3)]
    gs, rend = _open(pkg, kind)
    try:
        rend.set_graph_mode(graph)
        rend.set_frames_in_flight(3)
        for round_ in range(2):                              # (the second round replays the captured graphs)
            order = [0, 1, 2] if round_ == 0 else [2, 0, 1]
            targets = [torch.zeros((h, w, 4), dtype=torch.float32, device="cuda") for _ in order]
            for cam, t in zip(order, targets):
                rend.render(_uniforms(pkg, kind, cam), t.data_ptr(), 0)
            out = Arrays(n, h, w)
            rend.contributions(**out.t)
            _assert_equal(out, wants[order[-1]], f"graph {graph}, cameras {order}")
            for cam, t in zip(order, targets):
                assert np.array_equal(t.cpu().numpy().view(np.uint32), _reference(pkg, oracle, kind, cam)[1]["image"].view(np.uint32))
    finally:
        rend.close()
        gs.close()


def test_a_frame_that_overflowed_is_rerun_by_the_drain(pkg, oracle, gpu, monkeypatch):
    kind = "A"
    n, w, h = SCENES[kind]
    _, ref, want = _reference(pkg, oracle, kind)
    monkeypatch.setenv("GS_INITIAL_CAPACITY", "256")
    assert len(ref["keys"]) > 256
    gs, rend = _open(pkg, kind)
    try:
        target = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        rend.render(_uniforms(pkg, kind), target.data_ptr(), 0)      # enqueued only: nobody has seen it overflow yet
        out = Arrays(n, h, w)
        rend.contributions(**out.t)
        _assert_equal(out, want, "first frame overflowed")
        assert rend.stats().retries >= 1
    finally:
        rend.close()
        gs.close()


def test_before_any_frame_the_call_is_refused(pkg, gpu):
    gs, rend = _open(pkg, "A")
    try:
        with pytest.raises(pkg.binding.GsError) as e:
            rend.contributions()
        assert e.value.code == -1 and "no frame" in str(e.value)
    finally:
        rend.close()
        gs.close()


def test_misaligned_pointers_are_refused(pkg, gpu):
    import ctypes as C
    kind = "A"
    n, w, h = SCENES[kind]
    gs, rend = _open(pkg, kind)
    try:
        rend.render_host(_uniforms(pkg, kind))
        big = torch.zeros(2 * n + 8, dtype=torch.int64, device="cuda")
        base = big.data_ptr()
        L = pkg.binding.lib()
        for member, offset in (("weight", 4), ("pixels", 2), ("top_id", 1)):
            c = pkg.binding.Contributions()
            setattr(c, member, base + offset)
            assert L.gs_accumulate_contributions(rend._h, C.byref(c)) == -1, member
        assert (big == 0).all()
    finally:
        rend.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ 8. ids
def test_a_scene_read_in_spatial_order_reports_scene_ids(pkg, oracle, gpu, monkeypatch):
    kind = "T"
    n, w, h = SCENES[kind]
    _, _, want = _reference(pkg, oracle, kind)
    monkeypatch.setenv("GS_SPATIAL_MIN", "1")                # the scene gets its copy in spatial order at 1 500 Gaussians
    gs, rend = _open(pkg, kind)
    try:
        assert not np.array_equal(ls.morton_order(_records(pkg, kind)[:, :3]), np.arange(n))
        rend.render_host(_uniforms(pkg, kind))
        out = Arrays(n, h, w)
        rend.contributions(**out.t)
        _assert_equal(out, want, "spatial order")
    finally:
        rend.close()
        gs.close()
