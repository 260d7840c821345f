"""gs_blend_features on the device (gs_features.hip) against its definition restated in numpy (tests/feature_reference.py,
pinned to the oracle's image by tests/test_feature_maps_api.py).  Each pixel adds its entries in list order on one lane, so
every output is defined bit for bit: every comparison here is EXACT equality of the binary32 patterns, with no tolerance and no
case left out.  Outputs are views into larger device buffers preloaded with a sentinel, at an offset that is 4-byte aligned and
nothing more; the guard words around each view must survive the call.  Renderers start in exp mode 2 (conftest); every test
runs on both depth-order paths."""
import numpy as np
import pytest
import torch  # at collection, before the package loads its library: both must bind the same HIP runtime

import feature_reference as fref
import limit_scenes as ls
from helpers import assert_images_identical, compare_stages, oracle_frame
from test_gpu_blend_chunk_loop import _grazing_scene, _saturated_quadrant, _tile_list

pytestmark = pytest.mark.gpu

G = 16                                                # gs_kernels.h: kFeatureGroup, channels per launch
CHUNK = 64                                            # gs_features.hip: entries staged per chunk
SCENES = {"A": (600, 72, 40), "T": (1500, 64, 64)}    # synth_records(n, seed=5, kind) at width x height; 72 x 40 = 4.5 x 2.5 tiles
CAMERAS = [{}, dict(position=(0.3, -0.2, 0.5)), dict(position=(-0.25, 0.1, 0.3))]
GUARD, SENTINEL = 37, -7777.25                        # guard words on either side of a view (odd: the view is 4-byte aligned only)
OUTPUTS = ("out", "alpha", "depth", "median_depth")
WANT_KEY = dict(out="features", alpha="alpha", depth="depth", median_depth="median")
_cache = {}


def _features(n, channels, seed=11):
    """Seeded rows with negatives, an all-zero channel (1) and a channel of ones (2)."""
    f = np.random.default_rng(seed).standard_normal((n, channels)).astype(np.float32)
    if channels > 1:
        f[:, 1] = 0.0
    if channels > 2:
        f[:, 2] = 1.0
    return f


def _freeze(want):
    for a in want.values():
        a.setflags(write=False)
    return want


def _records(pkg, kind):
    return pkg.synth.synth_records(SCENES[kind][0], seed=5, kind=kind)


def _reference(pkg, oracle, kind, cam=0, channels=5):
    """(verts, oracle stages, features, reference maps) of a synthetic scene seen by CAMERAS[cam]: computed once, never changed."""
    key = (kind, cam, channels)
    if key not in _cache:
        n, w, h = SCENES[kind]
        fkey = (kind, cam)
        if fkey not in _cache:
            _cache[fkey] = oracle_frame(oracle, _records(pkg, kind), w, h, oracle.default_camera(**CAMERAS[cam]))
        verts, _, ref = _cache[fkey]
        feats = _features(n, channels)
        feats.setflags(write=False)
        _cache[key] = (verts, ref, feats, _freeze(fref.feature_maps(oracle, ref, w, h, feats)))
    return _cache[key]


def _uniforms(pkg, kind, cam=0):
    _, w, h = SCENES[kind]
    return pkg.camera_uniforms(pkg.make_camera(**CAMERAS[cam]), w, h)


def _open(pkg, kind):
    gs = pkg.Scene.from_records(_records(pkg, kind), device=0)
    return gs, pkg.Renderer(gs)


class Maps:
    """The outputs as views into larger flat device buffers preloaded with a sentinel."""

    def __init__(self, h, w, channels, only=OUTPUTS):
        self.buf, self.t = {}, {}
        for name in only:
            shape = (h, w, channels) if name == "out" else (h, w)
            numel = int(np.prod(shape))
            self.buf[name] = torch.full((numel + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
            self.t[name] = self.buf[name][GUARD:GUARD + numel].view(shape)
            assert self.t[name].is_contiguous() and self.t[name].data_ptr() % 16 != 0

    def get(self, name):
        return self.t[name].cpu().numpy()

    def guards_intact(self):
        for name, b in self.buf.items():
            g = torch.cat([b[:GUARD], b[-GUARD:]]).cpu().numpy()
            assert (g == np.float32(SENTINEL)).all(), f"{name}: a guard word was written"


def _assert_equal(maps, want, label):
    maps.guards_intact()
    for name in maps.t:
        got, w = maps.get(name), want[WANT_KEY[name]]
        if name == "out":
            w = w[..., :got.shape[2]]
        assert got.shape == w.shape, (label, name, got.shape, w.shape)
        bad = np.argwhere(got.view(np.uint32) != np.ascontiguousarray(w).view(np.uint32))
        assert len(bad) == 0, f"{label}: {name} differs at {len(bad)} place(s), first {tuple(bad[0])}: {got[tuple(bad[0])]!r} != {w[tuple(bad[0])]!r}"


def _run(rend, feats, want, h, w, label, only=OUTPUTS):
    channels = 0 if feats is None else feats.shape[1]
    maps = Maps(h, w, channels, only)
    ft = None if feats is None else torch.as_tensor(np.array(feats, np.float32, order="C")).cuda()   # (a copy: the cached rows are read-only)
    got = rend.feature_maps(features=ft, **maps.t)
    assert sorted(got) == sorted(maps.t)
    _assert_equal(maps, want, label)
    return maps


# ------------------------------------------------------------------------------------------------ 1. whole frame
@pytest.mark.parametrize("kind", sorted(SCENES))
def test_a_whole_frame_equals_the_reference_and_the_pass_reads_only(pkg, oracle, gpu, kind):
    n, w, h = SCENES[kind]
    verts, ref, feats, want = _reference(pkg, oracle, kind)
    assert np.isfinite(want["median"]).sum() > 100 and (want["median"] == np.inf).sum() > 100 and (want["alpha"] > 0).sum() > w * h // 4
    gs, rend = _open(pkg, kind)
    try:
        u = _uniforms(pkg, kind)
        before, _ = rend.render_host(u)
        assert_images_identical(before, ref["image"], label=f"kind {kind}")
        _run(rend, feats, want, h, w, f"kind {kind}")
        _run(rend, feats, want, h, w, f"kind {kind}, second call")      # one lane per pixel, list order: the same bits
        # the records' own colours blend to the frame's image
        colours = np.concatenate([rend.stage("uv_rg").reshape(-1, 4)[:, 2:4], rend.stage("b").reshape(-1, 1)], axis=1)
        rgb = Maps(h, w, 3, only=("out",))
        rend.feature_maps(features=torch.as_tensor(np.ascontiguousarray(colours, np.float32)).cuda(), **rgb.t)
        rgb.guards_intact()
        assert np.array_equal(rgb.get("out").view(np.uint32), np.ascontiguousarray(before[..., :3]).view(np.uint32)), \
            "the records' colours do not blend to the image"
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
        feats = _features(len(sc.records), 5)
        want = fref.feature_maps(oracle, ref, sc.width, sc.height, feats)
        rend.render_host(u)
        _run(rend, feats, want, sc.height, sc.width, f"list of {k}")
    finally:
        rend.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ 3. saturation, grazing inputs
@pytest.mark.parametrize("quadrant", [0, 3])
@pytest.mark.parametrize("chunk", [1, 2])
def test_a_quadrant_that_saturates_mid_list_while_the_rest_walk_on(pkg, oracle, gpu, chunk, quadrant):
    """More than five chunks; one 8 x 8 block of pixels has saturated by the end of `chunk`, the other three quadrants walk the
    whole list: the wave that is done stays for the barriers and adds nothing more."""
    rec, w, h = _saturated_quadrant(chunk, quadrant)
    gs, rend, u, ref = _limit_frame(pkg, oracle, rec, w, h)
    try:
        assert len(_tile_list(ref, w, (1, 1))) > 5 * CHUNK
        feats = _features(len(rec), 5)
        want = fref.feature_maps(oracle, ref, w, h, feats)
        y0, x0 = 16 + 8 * (quadrant >> 1), 16 + 8 * (quadrant & 1)
        assert (want["T"][y0:y0 + 8, x0:x0 + 8] < 0.01).all() and want["T"][16:32, 16:32].max() > 0.1
        rend.render_host(u)
        _run(rend, feats, want, h, w, f"quadrant {quadrant} saturates in chunk {chunk}")
    finally:
        rend.close()
        gs.close()


def test_grazing_splats_and_cancelling_needles(pkg, oracle, gpu):
    """Alpha within 1e-6 .. 1e-1 of 1/255 on either side at a quadrant's edge and corner pixels, and 45-degree needles whose
    `power` terms cancel: where a cull or a reordered product would flip what a pixel adds."""
    rec, w, h, n_graze, n_needle, _ = _grazing_scene()
    gs, rend, u, ref = _limit_frame(pkg, oracle, rec, w, h)
    try:
        feats = _features(len(rec), 5)
        want = fref.feature_maps(oracle, ref, w, h, feats)
        assert (want["alpha"] > 0).sum() > 100
        rend.render_host(u)
        _run(rend, feats, want, h, w, "grazing splats")
    finally:
        rend.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ 4. channel groups, single outputs
def test_channel_groups_and_single_outputs(pkg, oracle, gpu):
    kind = "A"
    n, w, h = SCENES[kind]
    _, ref, feats, want = _reference(pkg, oracle, kind, channels=256)   # (channel sums are independent: a prefix of the channels
    gs, rend = _open(pkg, kind)                                         #  blends to the same prefix of the reference)
    try:
        rend.render_host(_uniforms(pkg, kind))
        for channels in (1, G - 1, G, G + 1, 2 * G + 1, 256, 2, 3, 4, 5, G + 4, G + 5):   # (1 .. 4: kernels of their own size)
            _run(rend, feats[:, :channels], want, h, w, f"{channels} channels")
        _run(rend, None, want, h, w, "no channels, alpha alone", only=("alpha",))
        _run(rend, None, want, h, w, "median depth alone", only=("median_depth",))
        _run(rend, None, want, h, w, "depth alone", only=("depth",))
        _run(rend, feats[:, :G + 1], want, h, w, "out alone", only=("out",))
        _run(rend, feats[:, :3], want, h, w, "out and median", only=("out", "median_depth"))
        # outputs allocated by the wrapper
        got = rend.feature_maps(features=torch.as_tensor(np.array(feats[:, :5], np.float32, order="C")).cuda(), out=True, alpha=True, depth=True,
                                median_depth=True)
        for name in OUTPUTS:
            assert np.array_equal(got[name].cpu().numpy().view(np.uint32),
                                  np.ascontiguousarray(want[WANT_KEY[name]][..., :5] if name == "out" else want[WANT_KEY[name]]).view(np.uint32))
    finally:
        rend.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ 5. rows nobody blends
def test_nan_rows_of_gaussians_in_no_list_reach_no_output(pkg, oracle, gpu):
    kind = "A"
    n, w, h = SCENES[kind]
    _, ref, feats, want = _reference(pkg, oracle, kind)
    for k in ("features", "alpha", "depth"):
        assert np.isfinite(want[k]).all(), k
    assert not np.isnan(want["median"]).any()
    unlisted = np.setdiff1d(np.arange(n), ref["sorted_payload"])
    assert len(unlisted) > 10
    poisoned = feats.copy()
    poisoned[unlisted] = np.nan
    gs, rend = _open(pkg, kind)
    try:
        rend.render_host(_uniforms(pkg, kind))
        maps = _run(rend, poisoned, want, h, w, "NaN rows")
        for name in OUTPUTS:
            assert not np.isnan(maps.get(name)).any(), name
    finally:
        rend.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ 6. the blend's switches
@pytest.mark.parametrize("kind", sorted(SCENES))
def test_the_pass_does_not_depend_on_how_the_frame_was_blended(pkg, oracle, gpu, kind):
    n, w, h = SCENES[kind]
    _, _, feats, want = _reference(pkg, oracle, kind)
    gs, rend = _open(pkg, kind)
    try:
        u = _uniforms(pkg, kind)
        settings = [("exp mode 3", lambda: rend.set_exp_mode(3)), ("contraction on", lambda: rend.set_blend_contraction(True)),
                    ("lockstep 0", lambda: rend.set_blend_lockstep(0)), ("lockstep 1", lambda: rend.set_blend_lockstep(1))]
        for label, apply in settings:                        # (cumulative: each frame is blended with one more switch moved)
            apply()
            rend.render_host(u)
            _run(rend, feats, want, h, w, f"kind {kind}, {label}")
    finally:
        rend.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ 7. antialiased
def test_the_antialiased_mode_is_followed_through_the_records(pkg, oracle, gpu):
    """With set_antialiased(True) the records carry opacity' and its cut: the pass equals the reference run on the scene S' that
    holds the frame's opacity' (the recipe of test_gpu_contributions)."""
    kind = "T"
    n, w, h = SCENES[kind]
    verts, _, feats, plain = _reference(pkg, oracle, kind)
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
        want = fref.feature_maps(oracle, ref, w, h, feats)
        assert not np.array_equal(want["alpha"], plain["alpha"])
        _run(rend, feats, want, h, w, "antialiased")
    finally:
        rend.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ 8. which frame
@pytest.mark.parametrize("graph", [False, True], ids=["launches", "graph"])
def test_with_frames_in_flight_the_pass_reports_the_last_one(pkg, oracle, gpu, graph):
    kind = "A"
    n, w, h = SCENES[kind]
    refs = [_reference(pkg, oracle, kind, cam) for cam in range(3)]
    gs, rend = _open(pkg, kind)
    try:
        rend.set_graph_mode(graph)
        rend.set_frames_in_flight(3)
        for round_ in range(2):                              # (the second round replays the captured graphs)
            order = [0, 1, 2] if round_ == 0 else [2, 0, 1]
            targets = [torch.zeros((h, w, 4), dtype=torch.float32, device="cuda") for _ in order]
            for cam, t in zip(order, targets):
                rend.render(_uniforms(pkg, kind, cam), t.data_ptr(), 0)
            _run(rend, refs[order[-1]][2], refs[order[-1]][3], h, w, f"graph {graph}, cameras {order}")
            for cam, t in zip(order, targets):
                assert np.array_equal(t.cpu().numpy().view(np.uint32), refs[cam][1]["image"].view(np.uint32))
    finally:
        rend.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ 9. an overflowed frame
def test_a_frame_that_overflowed_is_rerun_by_the_drain(pkg, oracle, gpu, monkeypatch):
    kind = "A"
    n, w, h = SCENES[kind]
    _, ref, feats, want = _reference(pkg, oracle, kind)
    monkeypatch.setenv("GS_INITIAL_CAPACITY", "256")
    assert len(ref["keys"]) > 256
    gs, rend = _open(pkg, kind)
    try:
        target = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        rend.render(_uniforms(pkg, kind), target.data_ptr(), 0)      # enqueued only: nobody has seen it overflow yet
        _run(rend, feats, want, h, w, "first frame overflowed")
        assert rend.stats().retries >= 1
    finally:
        rend.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ 10. ids
def test_a_scene_read_in_spatial_order_takes_features_by_scene_id(pkg, oracle, gpu, monkeypatch):
    kind = "T"
    n, w, h = SCENES[kind]
    _, _, feats, want = _reference(pkg, oracle, kind)
    monkeypatch.setenv("GS_SPATIAL_MIN", "1")                # the scene gets its copy in spatial order at 1 500 Gaussians
    gs, rend = _open(pkg, kind)
    try:
        assert not np.array_equal(ls.morton_order(_records(pkg, kind)[:, :3]), np.arange(n))
        rend.render_host(_uniforms(pkg, kind))
        _run(rend, feats, want, h, w, "spatial order")
    finally:
        rend.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ 11. refusals and no-ops
def test_before_any_frame_the_call_is_refused(pkg, gpu):
    gs, rend = _open(pkg, "A")
    try:
        with pytest.raises(pkg.binding.GsError) as e:
            rend.feature_maps()
        assert e.value.code == -1 and "no frame" in str(e.value)
        with pytest.raises(pkg.binding.GsError) as e:
            rend.feature_maps(alpha=True)
        assert e.value.code == -1 and "no frame" in str(e.value)
    finally:
        rend.close()
        gs.close()


def test_without_outputs_nothing_is_written(pkg, gpu):
    kind = "A"
    n, w, h = SCENES[kind]
    gs, rend = _open(pkg, kind)
    try:
        rend.render_host(_uniforms(pkg, kind))
        assert rend.feature_maps() == {}
        # channels == 0 with out_features given: that output is not touched (the C entry point; the wrapper does not build this)
        import ctypes as C
        maps = Maps(h, w, 3, only=("out",))
        m = pkg.binding.FeatureMaps(channels=0, out_features=maps.t["out"].data_ptr())
        assert pkg.binding.lib().gs_blend_features(rend._h, C.byref(m)) == 0
        rend.synchronize()
        assert (maps.buf["out"] == SENTINEL).all()
    finally:
        rend.close()
        gs.close()
