"""What a renderer answers after a gs_render that returned an error (the contract: include/gs3d_hip.h at gs_render).  Every case
is ONE renderer that lives through good frames, a refusal or a failure, and good frames again; frames are compared with the
oracle bit for bit in exp mode 2 (conftest), oracle frames cached per scene, pose and size.

A REFUSED call changes nothing (test_a_refused_call_changes_nothing).  The four refusals -- width 0, 1 048 576 x 1 (a tile box
beyond 16 bits), 16400 x 64 (beyond the binning), null uniforms -- through gs_render and gs_render_host, after a frame of each
form (three-kernel level 1 over the planes, dense lists, one-pass level 1 whose plane taps are rebuilt from the records, the
global path with its depth_order tap, a slab frame), with one buffer set, with three, and under graph replay.  "Unchanged" is a
self-comparison of the same renderer across the call: every stage tap (the raw lists and ranges and the frame's own, culled
or not, too), level1_fused(), tile_cull() and listed_instances(), the contributions
(weight, pixels, top id) and the feature maps (5 channels, alpha, both depths) bit for bit, the stats field for field.  The lift
is not bit-reproducible by its definition: with non-negative values both results for a Gaussian with n terms lie within
(n - 1) 2^-53 S of the exact sum S of its terms (gs_lift.hip's header), so they differ by at most
2 (pixels[g] - 1) 2^-53 out[g] (1 + 2^-40), pixels[g] from the contributions pass, out[g] the smaller of the two -- derived, not
measured.  All arrays sit inside sentinel guards.  Then the same good frame again equals the oracle (a replay, in graph mode,
and the frame after it), and a frame followed AT ONCE by the refusal still gives the oracle's taps (the planes of a dense-list
or one-pass frame are rebuilt after the refusal, from the frame's size).  Every frame before the refused 16400 x 64 one has
fewer tiles than it, so the old code's re-allocation of `ranges` for the refused frame would have been reached.

A call that FAILS WHILE RETIRING queued frames leaves the renderer WITHOUT a last frame (test_after_a_failed_frame_*): the
unrefinable frame of limit_scenes (4112 x 256, bins of 16 x 16 tiles, 16385 candidates: "a bin holds more candidates ...") and a
run of 66 equal depths in a slab ("... depths are too crowded ..."), both under set_sort_path(2), each with a second camera pose
of the same scene whose fullest bin stays <= 4096 (re-measured from the oracle's stages here).  (a) a good frame, the failing
one through render_host; (b) two frames in flight, both sets warmed at both sizes, the failing pose queued at one size and the
good pose at another tile grid: the SECOND call raises; (c) three in flight, good - failing - good, synchronize() raises.
After each: error -5 with the right message, every tap and every pass raises "no frame rendered yet" and writes nothing,
stats() still describes the last frame that retired (all fields but retries and instance_capacity; in (c) that frame retired
inside the failing call, so its time spans are not known from before and are left out), and after set_sort_path(0) the failing
pose renders right -- image, taps, and the three passes against their references.

Not covered, and why: the run-away guard ("instance buffers overflowed repeatedly": nine re-runs in a row, each grow step sized
from the failing frame's own counts) and the two 2^30 limits (more than 2^30 tile instances or level-1 candidates) throw from
the same place in rerun_queued, behind the same forget_last_frame(), but cannot be reached at small shapes: the first needs
buffers that keep overflowing after being sized to fit, the others a gigabyte-scale frame."""
import numpy as np
import pytest
import torch  # at collection, before the package loads its library: both must bind the same HIP runtime

import contribution_reference as cref
import feature_reference as fref
import lift_reference as lref
import limit_scenes as ls
from helpers import assert_images_identical, compare_stages, oracle_frame
from test_gpu_feature_maps import Maps, _assert_equal as _assert_maps_equal, _features
from test_gpu_lift import Sums, _assert_close as _assert_lift_close, _values_tensor

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 37, -7777                           # guard words around the integer arrays of the contributions
CHANNELS, LIFT_CHANNELS = 5, 2
NO_FRAME = "no frame rendered yet"
ALL_TAPS = ("tiles", "depth", "radius", "aabb", "conic_opacity", "uv_rg", "b", "alpha_cut", "sorted_tile", "sorted_gid", "ranges",
            "lists_raw", "ranges_raw", "lists_culled", "ranges_culled")   # (the _culled pair of an unculled frame: its own lists)
_frames = {}


def _oracle(oracle, scene, width, height, position=(0.0, 0.0, 0.0)):
    """(verts, uniforms, stages) of `scene` seen from `position` at width x height: computed once, read only."""
    key = (scene.name, width, height, tuple(position))
    if key not in _frames:
        _frames[key] = oracle_frame(oracle, scene.records, width, height, oracle.default_camera(position=position))
    return _frames[key]


def _uniforms(pkg, u_ref, width, height, position=(0.0, 0.0, 0.0)):
    u = pkg.camera_uniforms(pkg.make_camera(position=position), width, height)
    assert u.tobytes() == u_ref.tobytes()
    return u


def _tile_count(width, height):
    return ls.tiles_across(width) * ls.tiles_across(height)


def _nonneg_values(h, w):
    """Seeded non-negative pixel rows; channel 1 is all ones (its lift is the weight)."""
    v = np.abs(np.random.default_rng(29).standard_normal((h, w, LIFT_CHANNELS))).astype(np.float32)
    v[..., 1] = 1.0
    return v


# ------------------------------------------------------------------------------------------------ the arrays of the passes
class Counts:
    """weight, pixels and top_id as views into larger flat device buffers: zeros (12345 for top_id) in the views, a sentinel in
    the guard words around them."""

    def __init__(self, n, h, w):
        self.buf, self.t = {}, {}
        for name, dtype, shape, fill in (("weight", torch.int64, (n,), 0), ("pixels", torch.int32, (n,), 0), ("top_id", torch.int32, (h, w), 12345)):
            numel = int(np.prod(shape))
            self.buf[name] = torch.full((numel + 2 * GUARD,), SENTINEL, dtype=dtype, device="cuda")
            self.t[name] = self.buf[name][GUARD:GUARD + numel].view(shape)
            self.t[name].fill_(fill)
            assert self.t[name].is_contiguous()
        torch.cuda.synchronize()                       # the passes run on the renderer's own, non-blocking stream

    def get(self, name):
        return self.t[name].cpu().numpy().view(np.uint64 if name == "weight" else np.uint32)

    def guards_intact(self):
        for name, b in self.buf.items():
            g = torch.cat([b[:GUARD], b[-GUARD:]]).cpu().numpy()
            assert (g == SENTINEL).all(), f"{name}: a guard word was written"


def _run_passes(rend, n, h, w, feats, vals):
    """The three passes over the renderer's last frame, into fresh guarded arrays: (Counts, Maps, Sums), guards checked."""
    counts = Counts(n, h, w)
    rend.contributions(**counts.t)
    counts.guards_intact()
    maps = Maps(h, w, feats.shape[1])
    ft = torch.as_tensor(np.array(feats, np.float32, order="C")).cuda()
    torch.cuda.synchronize()
    rend.feature_maps(features=ft, **maps.t)
    maps.guards_intact()
    sums = Sums(n, vals.shape[2])
    rend.lift_pixels(_values_tensor(vals), **sums.t)
    sums.guards_intact()
    return counts, maps, sums


def _snapshot(rend, u, n, feats, vals):
    """Everything the renderer answers about its last frame: stats, every tap, the results of the three passes."""
    h, w = int(u["height"][0]), int(u["width"][0])
    st = rend.stats().as_dict()
    names = ALL_TAPS + (("depth_order",) if st["sort_path"] == 1 else ())
    taps = {name: rend.stage(name, u).copy() for name in names}
    counts, maps, sums = _run_passes(rend, n, h, w, feats, vals)
    exact = {name: counts.get(name) for name in counts.t}
    exact.update({f"map {name}": maps.get(name) for name in maps.t})
    lift = {name: sums.get(name) for name in sums.t}
    getters = dict(level1_fused=rend.level1_fused(), tile_cull=rend.tile_cull(), listed_instances=rend.listed_instances())
    return dict(stats=st, getters=getters, taps=taps, exact=exact, lift=lift)


def _assert_unchanged(before, after, label):
    assert after["stats"] == before["stats"], f"{label}: stats changed: {before['stats']} -> {after['stats']}"
    assert after["getters"] == before["getters"], f"{label}: getters changed: {before['getters']} -> {after['getters']}"
    assert sorted(after["taps"]) == sorted(before["taps"])
    for kind in ("taps", "exact"):
        for name, a in before[kind].items():
            b = after[kind][name]
            assert a.shape == b.shape and a.dtype == b.dtype, (label, name)
            if a.tobytes() != b.tobytes():
                bad = np.nonzero(np.frombuffer(a.tobytes(), np.uint8) != np.frombuffer(b.tobytes(), np.uint8))[0]
                raise AssertionError(f"{label}: {name} changed in {len(bad)} byte(s), first at element {bad[0] // a.itemsize}")
    pixels = before["exact"]["pixels"].astype(np.float64)
    for name, a in before["lift"].items():
        b = after["lift"][name]
        assert (a >= 0).all() and (b >= 0).all(), (label, name)
        terms = pixels if a.ndim == 1 else pixels[:, None]
        bound = 2.0 * np.maximum(terms - 1.0, 0.0) * 2.0 ** -53 * np.minimum(a, b) * (1.0 + 2.0 ** -40)
        err = np.abs(a - b)
        bad = np.argwhere(~(err <= bound))
        print(f"{label}: lift {name}: worst |d| / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3g}")
        assert len(bad) == 0, (f"{label}: lift {name} moved beyond the bound at {len(bad)} place(s), first {tuple(bad[0])}: "
                               f"{a[tuple(bad[0])]!r} -> {b[tuple(bad[0])]!r}, bound {bound[tuple(bad[0])]:.3g}")


# ------------------------------------------------------------------------------------------------ refusals
REFUSED_FRAME = (16400, 64)
REFUSALS = {"width 0": "empty framebuffer", "1048576 x 1": "tile box is 16-bit", "16400 x 64": "resolution too large for the tile binning",
            "null uniforms": "null argument"}
# the frame before the refusal: (scene, environment, gs_set_level1_fused or None, gs_set_sort_path)
BIG = "1000000000"
FORMS = {"planes": (lambda: ls.level1_count(1025, 300, w=320, h=200), {"GS_L1_DENSE_MIN": BIG}, 0, 0),
         "dense_lists": (lambda: ls.level1_count(1025, 300, w=320, h=200), {"GS_L1_DENSE_MIN": "0"}, None, 0),
         "one_pass": (lambda: ls.level1_count(1025, 300, w=320, h=200), {"GS_L1_DENSE_MIN": BIG}, 1, 0),
         "global": (lambda: ls.level1_count(1025, 300, w=320, h=200), {"GS_L1_DENSE_MIN": BIG}, 0, 1),
         "slab": (lambda: ls.level2_size(16385, shift=2), {}, None, 0)}
MODES = ("one set", "three sets", "graph")


def _refuse(pkg, rend, u, which):
    """The refused call through both entry points: GS_ERR_INVALID with the refusal's own message."""
    lib, msg = pkg.binding.lib(), REFUSALS[which]
    if which == "null uniforms":
        for fn in (lib.gs_render, lib.gs_render_host):
            assert fn(rend._h, None, None, None) == -1 and msg in lib.gs_last_error().decode()
        return
    if which == "width 0":
        bad = u.copy()
        bad["width"] = 0
    else:
        size = (1048576, 1) if which == "1048576 x 1" else REFUSED_FRAME
        bad = pkg.camera_uniforms(pkg.make_camera(), *size)
    for call in (lambda: rend.render(bad), lambda: rend.render_host(bad)):
        with pytest.raises(pkg.GsError) as e:
            call()
        assert e.value.code == -1 and msg in str(e.value), f"{which}: {e.value}"


def _device_frames(rend, u, count):
    """`count` frames of `u` enqueued into device targets of their own, then synchronised: the images."""
    h, w = int(u["height"][0]), int(u["width"][0])
    targets = [torch.zeros((h, w, 4), dtype=torch.float32, device="cuda") for _ in range(count)]
    torch.cuda.synchronize()                           # (the frames run on the renderer's own, non-blocking streams)
    for t in targets:
        rend.render(u, t.data_ptr(), 0)
    rend.synchronize()
    return [t.cpu().numpy() for t in targets]


def _good_frames(rend, u, mode):
    if mode == "one set":
        return [rend.render_host(u)[0]]
    return _device_frames(rend, u, 3 if mode == "three sets" else 1)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("form", list(FORMS))
def test_a_refused_call_changes_nothing(pkg, oracle, gpu, monkeypatch, form, mode):
    build, env, fused, sort_path = FORMS[form]
    scene = build()
    monkeypatch.delenv("GS_SORT_PATH", raising=False)
    for k, v in {**scene.env, **env}.items():
        monkeypatch.setenv(k, v)
    w, h = scene.width, scene.height
    verts, u_ref, ref = _oracle(oracle, scene, w, h)
    got = ls.measure(scene, ref)
    for key, want in scene.expect.items():
        assert got[key] == want, f"{scene.name} missed its edge ({scene.pins}): {key} is {got[key]}, not {want}"
    # `ranges` used to be re-allocated for the refused 16400 x 64 frame (1025 x 4 tiles) when it had more tiles than every frame
    # before it: these frames stay below that, and below 3075
    assert _tile_count(w, h) < min(3075, _tile_count(*REFUSED_FRAME))
    u = _uniforms(pkg, u_ref, w, h)
    n = len(scene.records)
    feats, vals = _features(n, CHANNELS), _nonneg_values(h, w)
    gs = pkg.Scene.from_records(scene.records, device=0)
    rend = pkg.Renderer(gs)
    try:
        rend.set_sort_path(sort_path)
        if fused is not None:
            rend.set_level1_fused(fused)
        if mode == "three sets":
            rend.set_frames_in_flight(3)
        rend.set_graph_mode(mode == "graph")
        for k, which in enumerate(REFUSALS):
            label = f"{form}, {mode}, refused: {which}"
            for img in _good_frames(rend, u, mode):            # (graph mode: from the second round on, a replay)
                assert_images_identical(img, ref["image"], label=f"{label}: the frame before")
            if k == 0:
                compare_stages(pkg, rend, u, ref)
                st = rend.stats()
                assert rend.level1_fused() == (form == "one_pass"), f"{label}: not the form of level 1 the case is named for"
                assert st.sort_path == (1 if form == "global" else 2) and (st.sort_level == ls.SLAB_LEVEL) == (form == "slab")
            before = _snapshot(rend, u, n, feats, vals)
            _refuse(pkg, rend, u, which)
            after = _snapshot(rend, u, n, feats, vals)
            _assert_unchanged(before, after, label)
            assert rend.level1_fused() == (form == "one_pass")
            # the same frame again, the refusal at once behind it (in three-set mode: while frames are queued): the oracle's taps
            if mode == "three sets":
                targets = [torch.zeros((h, w, 4), dtype=torch.float32, device="cuda") for _ in range(3)]
                torch.cuda.synchronize()
                for j, t in enumerate(targets):
                    rend.render(u, t.data_ptr(), 0)
                    if j == 1:
                        _refuse(pkg, rend, u, which)
                rend.synchronize()
                again = [t.cpu().numpy() for t in targets]
            else:
                again = _good_frames(rend, u, mode)
            _refuse(pkg, rend, u, which)
            for img in again:
                assert_images_identical(img, ref["image"], label=f"{label}: the frame after")
            compare_stages(pkg, rend, u, ref)
            if mode == "graph":                                 # ... and the frame after it, which is a replay
                assert_images_identical(_good_frames(rend, u, mode)[0], ref["image"], label=f"{label}: the replay after")
    finally:
        rend.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ failures
BIN_TOO_FULL = "a bin holds more candidates than the bin-local sort can order"    # gs_renderer.cpp: DepthPolicy::kBinTooFull
TOO_CROWDED = "a bin's depths are too crowded for the bin-local order"            # ... kDepthsTooCrowded
# (scene, the pose whose fullest bin stays <= 4096, another tile grid, predict(forced=True), the message)
FAILURES = {"bin too full": (lambda: ls.build_unrefinable(16385), (0.3, 0.0, 0.0), (4112, 240), "bin too full", BIN_TOO_FULL),
            "depths too crowded": (lambda: ls.equal_run(66, "straddle", slab=True), (0.0, 0.0, -1.8), (128, 112), "error", TOO_CROWDED)}
_failure_refs = {}


class Failure:
    """The failing frame of a scene and its good pose, with the oracle's frames; the references of the three passes for the
    failing pose are computed when first asked for, once."""

    def __init__(self, pkg, oracle, monkeypatch, name):
        build, self.good_at, self.other_size, verdict, self.message = FAILURES[name]
        self.name, self.scene = name, build()
        sc = self.scene
        monkeypatch.delenv("GS_SORT_PATH", raising=False)
        for k, v in sc.env.items():
            monkeypatch.setenv(k, v)
        assert ls.predict(sc, forced=True) == verdict
        self.n, self.size = len(sc.records), (sc.width, sc.height)
        _, u_ref, self.ref_fail = _oracle(oracle, sc, *self.size)
        got = ls.measure(sc, self.ref_fail)
        for key, want in sc.expect.items():
            assert got[key] == want, f"{sc.name} missed its edge ({sc.pins}): {key} is {got[key]}, not {want}"
        self.u_fail = _uniforms(pkg, u_ref, *self.size)
        self.u_good, self.ref_good = {}, {}
        for size in (self.size, self.other_size):
            assert size == self.size or _tile_count(*size) != _tile_count(*self.size)
            _, u_ref, ref = _oracle(oracle, sc, *size, position=self.good_at)
            (fullest,) = ls.measure(sc, ref)["fullest_bin"].values()        # (at the one bin size the scene runs with)
            assert 0 < fullest <= ls.LEVEL_LIMITS[0], f"{sc.name} from {self.good_at} at {size}: fullest bin {fullest}"
            assert (ref["image"][..., :3] != 0).any()
            self.u_good[size], self.ref_good[size] = _uniforms(pkg, u_ref, *size, position=self.good_at), ref
        self.oracle = oracle

    def references(self):
        if self.name not in _failure_refs:
            (w, h), ref = self.size, self.ref_fail
            feats, vals = _features(self.n, CHANNELS), _nonneg_values(h, w)
            want = dict(feats=feats, vals=vals, counts=cref.contributions(self.oracle, ref, w, h),
                        maps=fref.feature_maps(self.oracle, ref, w, h, feats), lift=lref.lift(self.oracle, ref, w, h, vals))
            for group in want.values():
                for a in (group.values() if isinstance(group, dict) else [group]):
                    if isinstance(a, np.ndarray):
                        a.setflags(write=False)
            _failure_refs[self.name] = want
        return _failure_refs[self.name]

    def open(self, pkg, in_flight):
        gs = pkg.Scene.from_records(self.scene.records, device=0)
        rend = pkg.Renderer(gs)
        rend.set_sort_path(2)
        if in_flight > 1:
            rend.set_frames_in_flight(in_flight)
        return gs, rend

    def target(self, size=None):
        w, h = size or self.size
        t = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()                       # (the frames run on the renderer's own, non-blocking streams)
        return t

    def assert_raised(self, pkg, e, label):
        print(f"{label}: raised {e.value}")
        assert e.value.code == -5 and self.message in str(e.value), f"{label}: the error of another failure: {e.value}"

    def assert_no_last_frame(self, pkg, rend, label):
        """Every tap and every pass refuses with the code and message of a renderer that has not rendered yet, and writes nothing;
        so does listed_instances(), no frame's lists are culled, and level1_fused() still answers (for the frame that failed)."""
        (w, h), n = self.size, self.n
        with pytest.raises(pkg.GsError) as e:
            rend.listed_instances()
        assert e.value.code == -1 and NO_FRAME in str(e.value), f"{label}: listed_instances: {e.value}"
        assert rend.tile_cull()[1] is False, f"{label}: a renderer without a last frame reports culled lists"
        assert rend.level1_fused() in (True, False)
        for name in pkg.binding.STAGES:
            with pytest.raises(pkg.GsError) as e:
                rend.stage(name, self.u_fail)
            assert e.value.code == -1 and NO_FRAME in str(e.value), f"{label}: tap {name}: {e.value}"
        counts, maps, sums = Counts(n, h, w), Maps(h, w, CHANNELS), Sums(n, LIFT_CHANNELS)
        ft = torch.as_tensor(_features(n, CHANNELS)).cuda()
        torch.cuda.synchronize()
        calls = dict(contributions=lambda: rend.contributions(**counts.t), feature_maps=lambda: rend.feature_maps(features=ft, **maps.t),
                     lift_pixels=lambda: rend.lift_pixels(_values_tensor(_nonneg_values(h, w)), **sums.t))
        for name, call in calls.items():
            with pytest.raises(pkg.GsError) as e:
                call()
            assert e.value.code == -1 and NO_FRAME in str(e.value), f"{label}: {name}: {e.value}"
        for arrays in (counts, maps, sums):
            arrays.guards_intact()
        assert (counts.get("weight") == 0).all() and (counts.get("pixels") == 0).all() and (counts.t["top_id"] == 12345).all()
        assert all((b == -7777.25).all() for b in maps.buf.values()), f"{label}: a refused feature_maps wrote a map"
        assert all((sums.get(k) == 0).all() for k in sums.t), f"{label}: a refused lift_pixels added to a sum"

    def assert_stats_kept(self, rend, retired, label, spans=True):
        now = rend.stats().as_dict()
        keys = [k for k in retired if k not in ("retries", "instance_capacity") and (spans or not k.startswith("ms_"))]
        assert {k: now[k] for k in keys} == {k: retired[k] for k in keys}, f"{label}: stats {now}, after the last retired frame {retired}"

    def assert_renders_on(self, pkg, rend, label):
        """gs_set_sort_path(0): the failing pose is right -- image, taps, and the three passes against their references."""
        (w, h), want = self.size, self.references()
        rend.set_sort_path(0)
        img, _ = rend.render_host(self.u_fail)
        assert_images_identical(img, self.ref_fail["image"], label=f"{label}: the failing pose in automatic mode")
        compare_stages(pkg, rend, self.u_fail, self.ref_fail)
        counts, maps, sums = _run_passes(rend, self.n, h, w, want["feats"], want["vals"])
        for name in counts.t:
            bad = np.argwhere(counts.get(name) != want["counts"][name])
            assert len(bad) == 0, f"{label}: contributions: {name} differs at {len(bad)} place(s), first {tuple(bad[0])}"
        _assert_maps_equal(maps, want["maps"], f"{label}: feature maps")
        _assert_lift_close(sums, want["lift"], f"{label}: lift")


@pytest.mark.parametrize("name", list(FAILURES))
def test_after_a_failed_frame_the_renderer_has_no_last_frame(pkg, oracle, gpu, monkeypatch, name):
    """(a): one frame at a time.  The failing frame ran on the set of the good frame before it."""
    f = Failure(pkg, oracle, monkeypatch, name)
    gs, rend = f.open(pkg, 1)
    try:
        img, _ = rend.render_host(f.u_good[f.size])
        assert_images_identical(img, f.ref_good[f.size]["image"], label=f"{name}: the good pose")
        compare_stages(pkg, rend, f.u_good[f.size], f.ref_good[f.size])
        retired = rend.stats().as_dict()
        with pytest.raises(pkg.GsError) as e:
            rend.render_host(f.u_fail)
        f.assert_raised(pkg, e, name)
        f.assert_no_last_frame(pkg, rend, name)
        f.assert_stats_kept(rend, retired, name)
        f.assert_renders_on(pkg, rend, name)
    finally:
        rend.close()
        gs.close()


@pytest.mark.parametrize("name", list(FAILURES))
def test_after_a_frame_that_fails_inside_the_next_call(pkg, oracle, gpu, monkeypatch, name):
    """(b): two frames in flight, both sets warm at both sizes, so the second call waits for nothing but the new tile grid -- and
    retires the failing frame there.  The frame of that call was never enqueued; it is not the last frame."""
    f = Failure(pkg, oracle, monkeypatch, name)
    gs, rend = f.open(pkg, 2)
    try:
        warm = [(size, f.target(size)) for size in (f.size, f.other_size) for _ in range(2)]
        for size, t in warm:
            rend.render(f.u_good[size], t.data_ptr(), 0)
        rend.synchronize()
        for size, t in warm:
            assert_images_identical(t.cpu().numpy(), f.ref_good[size]["image"], label=f"{name}: the good pose at {size}")
        retired = rend.stats().as_dict()
        t_fail, t_good = f.target(), f.target(f.other_size)
        rend.render(f.u_fail, t_fail.data_ptr(), 0)              # queued: nobody has seen it fail yet
        with pytest.raises(pkg.GsError) as e:
            rend.render(f.u_good[f.other_size], t_good.data_ptr(), 0)
        f.assert_raised(pkg, e, name)
        f.assert_no_last_frame(pkg, rend, name)
        f.assert_stats_kept(rend, retired, name)
        f.assert_renders_on(pkg, rend, name)
    finally:
        rend.close()
        gs.close()


@pytest.mark.parametrize("name", list(FAILURES))
def test_after_a_frame_that_fails_between_two_good_ones(pkg, oracle, gpu, monkeypatch, name):
    """(c): three in flight, good - failing - good on warm sets; synchronize() raises.  The first good frame retired inside that
    call (the stats are its counts: the pose's, as before; its time spans are its own), the other two were dropped.  In automatic
    mode the same three poses then render right into their targets."""
    f = Failure(pkg, oracle, monkeypatch, name)
    gs, rend = f.open(pkg, 3)
    try:
        good, ref_good = f.u_good[f.size], f.ref_good[f.size]
        for img in _device_frames(rend, good, 3):
            assert_images_identical(img, ref_good["image"], label=f"{name}: the good pose")
        retired = rend.stats().as_dict()
        poses = [(good, ref_good), (f.u_fail, f.ref_fail), (good, ref_good)]
        targets = [f.target() for _ in poses]
        for (u, _), t in zip(poses, targets):
            rend.render(u, t.data_ptr(), 0)
        with pytest.raises(pkg.GsError) as e:
            rend.synchronize()
        f.assert_raised(pkg, e, name)
        f.assert_no_last_frame(pkg, rend, name)
        f.assert_stats_kept(rend, retired, name, spans=False)
        rend.set_sort_path(0)
        for t in targets:
            t.zero_()
        torch.cuda.synchronize()
        for (u, _), t in zip(poses, targets):
            rend.render(u, t.data_ptr(), 0)
        rend.synchronize()
        for k, ((_, ref), t) in enumerate(zip(poses, targets)):
            assert_images_identical(t.cpu().numpy(), ref["image"], label=f"{name}: pose {k} of three in automatic mode")
        compare_stages(pkg, rend, good, ref_good)
        f.assert_renders_on(pkg, rend, name)
    finally:
        rend.close()
        gs.close()
