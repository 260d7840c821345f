"""gs_project_backward on the device (gs_project_backward.hip) against its definition restated in numpy
(tests/project_backward_reference.py, pinned to torch.autograd and given teeth by tests/test_project_backward_api.py), and
Renderer.differentiable_render over both backward passes.  The sums are binary64 and the association is unspecified, so every
comparison is the bound that module derives, with no element of any of the six outputs left out:
    |got - (preload + times * want)| <= 2 times ((660 + times) A + |preload|) 2^-53;    an element with A = 0 keeps its bits.
Outputs are views into larger device buffers with guard words, preloaded with a pattern (a -0.0 among it), offset so that they are
8-byte aligned and nothing more; so are the inputs.  Frames are at most 1152 x 128, scenes at most some 4 200 Gaussians."""
import ctypes as C

import numpy as np
import pytest
import torch  # at collection, before the package loads its library: both must bind the same HIP runtime

import backward_reference as bref
import limit_scenes as ls
import project_backward_reference as pref
import project_backward_scenes as psc
from helpers import oracle_frame
from test_gpu_blend_backward import SCENES, _grads
from test_gpu_lift import GUARD, SENTINEL, _offset_view

pytestmark = pytest.mark.gpu

NAMES = tuple(pref.OUTPUTS)           # means, log_scales, quats, opacity_logits, sh_dc, sh_rest
INS = tuple(pref.INPUTS)              # colour, opacity, conic, uv
PATTERN = np.array([1.5, -0.0, -2.25, 0.0078125, -640.0, 0.0, 3.0e-9])
_cache = {}


def _shapes(n, k):
    return dict(means=(n, 3), log_scales=(n, 3), quats=(n, 4), opacity_logits=(n,), sh_dc=(n, 3), sh_rest=(n, k, 3))


class Arrays:
    """The six outputs as float64 views into larger flat device buffers: a pattern in the views, a sentinel in the guard words."""

    def __init__(self, n, k=15, only=NAMES):
        self.buf, self.t, self.pre = {}, {}, {}
        for i, name in enumerate(only):
            shape = _shapes(n, k)[name]
            numel = int(np.prod(shape))
            if numel == 0:
                continue
            pre = PATTERN[(np.arange(numel) * 5 + i) % len(PATTERN)]
            self.buf[name] = torch.full((numel + 2 * GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
            self.t[name] = self.buf[name][GUARD:GUARD + numel].view(shape)
            self.t[name].copy_(torch.as_tensor(pre.reshape(shape)))
            self.pre[name] = pre.reshape(shape)
            assert self.t[name].is_contiguous() and self.t[name].data_ptr() % 8 == 0 and self.t[name].data_ptr() % 16 != 0

    def get(self, name):
        return self.t[name].cpu().numpy()

    def guards_intact(self):
        for name, b in self.buf.items():
            g = torch.cat([b[:GUARD], b[-GUARD:]]).cpu().numpy()
            assert (g == SENTINEL).all(), f"{name}: a guard word was written"


def _assert_close(arr, want, label, times=1, skip_rows=None):
    """Every element of every output within the bound, `times` calls after the preload; an element no gradient reaches -- every
    element of a culled Gaussian among them -- keeps its bits."""
    arr.guards_intact()
    for name in arr.t:
        got, total, pre = arr.get(name), want[name], arr.pre[name]
        assert got.shape == total.shape, (label, name, got.shape, total.shape)
        keep = np.ones(len(got), bool)
        if skip_rows is not None:
            keep[skip_rows] = False
        lim = pref.bound(want, name, pre, times)
        err = np.abs(got - (pre + times * total))
        ratio = err[keep] / np.maximum(lim[keep], 1e-300)
        print(f"{label}: {name}: worst error / bound = {float(ratio.max()) if ratio.size else 0.0:.3g}")
        bad = np.argwhere(~(err <= lim) & keep.reshape((-1,) + (1,) * (got.ndim - 1)))
        assert len(bad) == 0, (f"{label}: {name} is outside the bound at {len(bad)} place(s), first {tuple(bad[0])}: "
                               f"{got[tuple(bad[0])]!r} against {(pre + times * total)[tuple(bad[0])]!r}, bound {lim[tuple(bad[0])]:.3g}")
        untouched = (want["A"][name] == 0) & keep.reshape((-1,) + (1,) * (got.ndim - 1))
        assert (got[untouched].view(np.uint64) == pre[untouched].view(np.uint64)).all(), f"{label}: {name}: an element no gradient reaches changed"
        assert (want["A"][name][~want["visible"]] == 0).all()


def _inputs(g):
    return {name: (None if g.get(name) is None else _offset_view(g[name], torch.float64, 1)) for name in INS}


def _want(verts, u, ref, g, antialiased=False, sh16=False, k=15):
    return pref.backward(*pref.unpack_vertices(verts, sh16=sh16), u, ref["tiles"] != 0, ref["attr"]["color_radii"][:, 0] > 0,
                         colour=g.get("colour"), opacity_grad=g.get("opacity"), conic=g.get("conic"), uv=g.get("uv"),
                         antialiased=antialiased, sh_rest_coeffs=k)


def _oracle(oracle, key, rec, w, h, sh16=False):
    """(vertices, uniforms, stages) of the oracle's frame, on coefficients rounded to binary16 where the scene is read from that
    storage: computed once per key, never changed."""
    key = (key, sh16)
    if key not in _cache:
        verts, u, ref = oracle_frame(oracle, rec, w, h)
        if sh16:
            verts["sh"] = verts["sh"].astype(np.float16).astype(np.float32)
            ref = oracle.stages(verts, u)
        _cache[key] = (verts, u, ref)
    return _cache[key]


def _open(pkg, rec, w, h, sh16=False, antialiased=False):
    gs = pkg.Scene.from_records(rec, device=0)
    if sh16:
        gs.quantize_sh()
    rend = pkg.Renderer(gs)
    rend.set_antialiased(antialiased)
    return gs, rend, pkg.camera_uniforms(pkg.make_camera(), w, h)


def _run(rend, g, want, n, label, k=15, only=NAMES, times=1):
    arr = Arrays(n, k, only)
    for _ in range(times):
        out = rend.project_backward(**_inputs(g), out=dict(arr.t))
        assert sorted(out) == sorted(arr.t)
    _assert_close(arr, want, label, times)
    return arr


# ------------------------------------------------------------------------------------------------ 1. the whole chain
@pytest.mark.parametrize("kind,sh16,antialiased", [("A", False, False), ("A", True, True), ("T", False, True), ("T", True, False)])
def test_render_blend_backward_project_backward_on_small_frames(pkg, oracle, gpu, _sort_path, kind, sh16, antialiased):
    n, w, h = SCENES[kind]
    rec = pkg.synth.synth_records(n, seed=5, kind=kind)
    verts, u_ref, ref = _oracle(oracle, ("synth", kind), rec, w, h, sh16)
    gs, rend, u = _open(pkg, rec, w, h, sh16, antialiased)
    try:
        assert u.tobytes() == u_ref.tobytes()
        rend.render_host(u)
        assert np.array_equal(rend.stage("tiles"), ref["tiles"])
        G, ga = _grads(h, w)
        d = rend.blend_backward(torch.as_tensor(G).cuda(), torch.as_tensor(ga).cuda(), colour=True, opacity=True, conic=True, uv=True)
        g = {name: d[name].cpu().numpy() for name in INS}
        want = _want(verts, u, ref, g, antialiased, sh16)
        assert want["visible"].sum() > n // 4 and all(np.abs(want[name]).max() > 0 for name in NAMES)
        label = f"kind {kind}, {'binary16' if sh16 else 'fp32'} SH, {'antialiased' if antialiased else 'reference mode'}"
        arr = Arrays(n)
        rend.project_backward(**d, out=dict(arr.t))
        _assert_close(arr, want, label)
        rend.project_backward(**d, out=dict(arr.t))
        _assert_close(arr, want, label + ", a second call into the same arrays", times=2)
        fresh = rend.project_backward(**d)                     # zeros allocated by the wrapper, all six, degree 3
        for name in NAMES:
            assert fresh[name].dtype == torch.float64 and tuple(fresh[name].shape) == want[name].shape
            assert (np.abs(fresh[name].cpu().numpy() - want[name]) <= pref.bound(want, name)).all(), name
        rend.set_sort_path(2)                                  # the forced bin-local path: other lists, the same records and visibility
        rend.render_host(u)
        assert rend.stats().sort_path == 2
        _run(rend, g, want, n, label + ", sort path 2")
    finally:
        rend.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ 2. lane patterns
LEVEL1_FORMS = {"planes": ("1000000000", 0), "dense_lists": ("0", None), "one_pass": ("1000000000", 1)}   # test_gpu_limits.py


@pytest.mark.parametrize("level1", list(LEVEL1_FORMS))
@pytest.mark.parametrize("order", ["scene", "spatial"])
@pytest.mark.parametrize("tail", ls.WAVE_TAILS)
def test_every_count_of_visible_lanes_per_wave_in_scene_and_in_spatial_order(pkg, oracle, gpu, monkeypatch, tail, order, level1):
    """limit_scenes.wave_patterns: every count and placement of visible lanes, the ragged wave of 37, all three cull exits in every
    wave; in spatial order lane j's Gaussian has another scene id, and everything lands by that id.  Each form of level 1 leaves
    the frame's visibility in another place (the planes, the dense lists, the one-pass bits): the pass reads the tap's answer."""
    scene = ls.wave_patterns(order, tail)
    verts, u_ref, ref = _oracle(oracle, scene.name, scene.records, scene.width, scene.height)
    n = len(scene.records)
    assert (ref["tiles"] != 0).sum() == scene.expect["visible"]
    dense_min, switch = LEVEL1_FORMS[level1]
    monkeypatch.delenv("GS_SORT_PATH", raising=False)
    for k, v in {**scene.env, "GS_L1_DENSE_MIN": dense_min}.items():
        monkeypatch.setenv(k, v)
    g = psc.random_gradients(n, seed=11)
    if (scene.name, "want") not in _cache:
        _cache[(scene.name, "want")] = _want(verts, u_ref, ref, g)
    want = _cache[(scene.name, "want")]
    gs, rend, u = _open(pkg, scene.records, scene.width, scene.height)
    try:
        if switch is not None:
            rend.set_level1_fused(switch)
        rend.render_host(u)
        assert rend.level1_fused() == (level1 == "one_pass")
        _run(rend, g, want, n, f"{scene.name}, {level1}")
        assert np.array_equal(rend.stage("tiles"), ref["tiles"])
    finally:
        rend.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ 3. sizes
def _small_scene(n, visible=True):
    w = h = 64
    rng = np.random.default_rng(100 + n)
    bits = ls._spread_bits(n, span=4096)
    rec = ls._splats(bits, None, None, w, h, pixel=(rng.uniform(4.0, 60.0, n), rng.uniform(4.0, 60.0, n)))
    tz = bits.view(np.float32).astype(np.float64)
    rec[:, 55:58] = np.log(tz * 0.01)[:, None] + 0.5 * rng.standard_normal((n, 3))
    rec[:, 58:62] = rng.standard_normal((n, 4))
    rec[:, 9:54] = 0.3 * rng.standard_normal((n, 45))
    if not visible:
        rec[:, 2] = 2.0                                        # behind the camera
    return rec, w, h


@pytest.mark.parametrize("n,visible", [(1, True), (63, True), (64, True), (65, True), (257, True), (64, False)])
def test_sizes_around_one_wave_all_visible_and_a_wave_with_none(pkg, oracle, gpu, n, visible):
    rec, w, h = _small_scene(n, visible)
    verts, u_ref, ref = _oracle(oracle, ("small", n, visible), rec, w, h)
    assert (ref["tiles"] != 0).sum() == (n if visible else 0)
    g = psc.random_gradients(n, seed=13)
    want = _want(verts, u_ref, ref, g)
    gs, rend, u = _open(pkg, rec, w, h)
    try:
        rend.render_host(u)
        arr = _run(rend, g, want, n, f"{n} Gaussians, {'all' if visible else 'none'} visible")
        if not visible:                                        # nothing at all is written
            for name in NAMES:
                assert np.array_equal(arr.get(name).view(np.uint64), arr.pre[name].view(np.uint64)), name
    finally:
        rend.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ 4. branches
@pytest.mark.parametrize("antialiased", [False, True], ids=["reference mode", "antialiased"])
def test_the_clamps_either_side_a_red_channel_at_zero_and_a_needle_without_area(pkg, oracle, gpu, antialiased):
    """project_backward_scenes.branch_records; that each Gaussian stands on the intended side of its branch, by which margin, is
    asserted on the reference in tests/test_project_backward_api.py and again here on the device's record."""
    rec, (w, h) = psc.branch_records(), psc.BRANCH_FRAME
    verts, u_ref, ref = _oracle(oracle, "branch", rec, w, h)
    n = len(rec)
    g = psc.random_gradients(n, seed=17)
    want = _want(verts, u_ref, ref, g, antialiased)
    assert want["binds"][list(psc.BRANCH_BEYOND_X), 0].all() and want["binds"][list(psc.BRANCH_BEYOND_Y), 1].all()
    assert want["binds"].sum() == 4 and want["visible"].all()
    gs, rend, u = _open(pkg, rec, w, h, antialiased=antialiased)
    try:
        rend.render_host(u)
        assert (rend.stage("tiles") != 0).all()
        assert rend.stage("uv_rg").reshape(-1, 4)[psc.BRANCH_RED_OFF, 2] == 0 and rend.stage("uv_rg").reshape(-1, 4)[psc.BRANCH_RED_ON, 2] > 0.5
        if antialiased:
            assert rend.stage("conic_opacity").reshape(-1, 4)[psc.BRANCH_NEEDLE, 3] == 0 and want["det_raw"][psc.BRANCH_NEEDLE] == 0
        arr = _run(rend, g, want, n, f"branches, {'antialiased' if antialiased else 'reference mode'}")
        off = psc.BRANCH_RED_OFF                               # its r row stays untouched; g and b flow
        assert np.array_equal(arr.get("sh_dc")[off, 0:1].view(np.uint64), arr.pre["sh_dc"][off, 0:1].view(np.uint64))
        assert np.array_equal(arr.get("sh_rest")[off, :, 0].view(np.uint64), np.ascontiguousarray(arr.pre["sh_rest"][off, :, 0]).view(np.uint64))
        assert (arr.get("sh_dc")[off, 1:] != arr.pre["sh_dc"][off, 1:]).all()
        if antialiased:                                        # comp is the constant 0: the opacity's gradient goes nowhere
            needle = psc.BRANCH_NEEDLE
            assert arr.get("opacity_logits")[needle:needle + 1].view(np.uint64) == arr.pre["opacity_logits"][needle:needle + 1].view(np.uint64)
    finally:
        rend.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ 5. NULLs, K, NaN, the frame
def test_each_input_null_in_turn_each_output_null_in_turn_and_every_k(pkg, oracle, gpu):
    kind = "A"
    n, w, h = SCENES[kind]
    rec = pkg.synth.synth_records(n, seed=5, kind=kind)
    verts, u_ref, ref = _oracle(oracle, ("synth", kind), rec, w, h)
    g = psc.random_gradients(n, seed=19)
    gs, rend, u = _open(pkg, rec, w, h)
    try:
        rend.render_host(u)
        full = _want(verts, u, ref, g)
        for left_out in INS:                                   # a NULL input is an array of zeros
            part = dict(g, **{left_out: None})
            want = _want(verts, u, ref, part)
            _run(rend, part, want, n, f"input {left_out} NULL")
            zeros = dict(g, **{left_out: np.zeros_like(g[left_out])})
            _run(rend, zeros, want, n, f"input {left_out} of zeros")
        for left_out in NAMES:                                 # a NULL output is skipped: the others are what they were
            _run(rend, g, full, n, f"without output {left_out}", only=tuple(k for k in NAMES if k != left_out))
        for k in (0, 3, 8, 15):
            _run(rend, g, _want(verts, u, ref, g, k=k), n, f"sh_rest_coeffs {k}", k=k)
        # all six NULL: success, nothing is launched; through the wrapper: an empty dict comes back
        assert rend.project_backward(**_inputs(g), out={}) == {}
        assert pkg.binding.lib().gs_project_backward(rend._h, C.byref(pkg.binding.ProjectGrads())) == 0
    finally:
        rend.close()
        gs.close()


def test_a_nan_in_one_gaussians_d_conic_reaches_that_gaussians_rows_only(pkg, oracle, gpu):
    kind = "A"
    n, w, h = SCENES[kind]
    rec = pkg.synth.synth_records(n, seed=5, kind=kind)
    verts, u_ref, ref = _oracle(oracle, ("synth", kind), rec, w, h)
    g = psc.random_gradients(n, seed=19)
    want = _want(verts, u_ref, ref, g)
    v = int(np.nonzero(want["visible"])[0][7])
    poisoned = {name: a.copy() for name, a in g.items()}
    poisoned["conic"][v, 1] = np.nan
    gs, rend, u = _open(pkg, rec, w, h)
    try:
        rend.render_host(u)
        arr = Arrays(n)
        rend.project_backward(**_inputs(poisoned), out=dict(arr.t))
        _assert_close(arr, want, "a NaN in one d_conic", skip_rows=[v])
        for name in ("means", "log_scales", "quats"):
            assert np.isnan(arr.get(name)[v]).all(), name
        for name in ("opacity_logits", "sh_dc", "sh_rest"):    # not downstream of the conic
            assert np.isfinite(arr.get(name)[v]).all(), name
        for name in NAMES:
            assert np.isfinite(np.delete(arr.get(name), v, axis=0)).all(), name
    finally:
        rend.close()
        gs.close()


def test_the_pass_answers_for_the_frame_not_for_a_setter_made_after_it(pkg, oracle, gpu):
    kind = "T"
    n, w, h = SCENES[kind]
    rec = pkg.synth.synth_records(n, seed=5, kind=kind)
    verts, u_ref, ref = _oracle(oracle, ("synth", kind), rec, w, h)
    g = psc.random_gradients(n, seed=23)
    on, off = _want(verts, u_ref, ref, g, antialiased=True), _want(verts, u_ref, ref, g, antialiased=False)
    assert (np.abs(on["log_scales"] - off["log_scales"]) > 1000.0 * pref.bound(on, "log_scales")).any()
    gs, rend, u = _open(pkg, rec, w, h, antialiased=True)
    try:
        rend.render_host(u)
        rend.set_antialiased(False)
        _run(rend, g, on, n, "an antialiased frame, the mode switched off after it")
        rend.render_host(u)
        rend.set_antialiased(True)
        _run(rend, g, off, n, "a reference-mode frame, the mode switched on after it")
    finally:
        rend.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ 6. refusals on the device
def test_before_any_frame_a_misaligned_pointer_and_a_bad_k_are_refused_and_nothing_is_written(pkg, gpu):
    kind = "A"
    n, w, h = SCENES[kind]
    gs, rend, u = _open(pkg, pkg.synth.synth_records(n, seed=5, kind=kind), w, h)
    try:
        big = torch.zeros(59 * n + 8, dtype=torch.float64, device="cuda")    # the six outputs, one behind the other
        ones = torch.ones(3 * n + 8, dtype=torch.float64, device="cuda")
        L, PG = pkg.binding.lib(), pkg.binding.ProjectGrads
        at = lambda rows: big.data_ptr() + 8 * rows * n  # noqa: E731

        def struct(**over):
            s = PG(d_colour=ones.data_ptr(), d_opacity=ones.data_ptr(), d_conic=ones.data_ptr(), d_uv=ones.data_ptr(), d_means=at(0),
                   d_log_scales=at(3), d_quats=at(6), d_opacity_logits=at(10), d_sh_dc=at(11), d_sh_rest=at(14), sh_rest_coeffs=15)
            for k, v in over.items():
                setattr(s, k, v)
            return s
        with pytest.raises(pkg.binding.GsError) as e:
            rend.project_backward()
        assert e.value.code == -1 and "no frame" in str(e.value)
        assert L.gs_project_backward(rend._h, C.byref(struct())) == -1 and b"no frame" in L.gs_last_error()
        assert L.gs_project_backward(rend._h, C.byref(PG())) == -1          # nothing asked for: still no frame to answer from
        rend.render_host(u)
        for member, _ in PG._fields_[:-1]:
            assert L.gs_project_backward(rend._h, C.byref(struct(**{member: big.data_ptr() + 4}))) == -1, member
            assert b"aligned" in L.gs_last_error()
        for k in (1, 7, 16, 45):
            assert L.gs_project_backward(rend._h, C.byref(struct(sh_rest_coeffs=k))) == -1, k
        assert L.gs_project_backward(rend._h, C.byref(struct(d_sh_rest=None))) == -1
        assert (big == 0).all()
        assert L.gs_project_backward(rend._h, C.byref(struct())) == 0       # ... and the same structure, in order, is taken
        assert (big != 0).any()
    finally:
        rend.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ 7. differentiable_render
RENDER_SCENE = (200, 64, 48)


def _parameters(rec, requires_grad=()):
    n = len(rec)
    p = dict(means=rec[:, 0:3], log_scales=rec[:, 55:58], quats=rec[:, 58:62], opacity_logits=rec[:, 54], sh_dc=rec[:, 6:9],
             sh_rest=rec[:, 9:54].reshape(n, 3, 15).transpose(0, 2, 1))
    return {k: torch.tensor(np.ascontiguousarray(v, np.float32), device="cuda", requires_grad=k in requires_grad) for k, v in p.items()}


def test_differentiable_render_is_the_two_passes_rounded_to_float32(pkg, oracle, gpu):
    n, w, h = RENDER_SCENE
    rec = pkg.synth.synth_records(n, seed=9, kind="A")
    params = _parameters(rec, requires_grad=NAMES)
    gs = pkg.Scene.from_tensors(**{k: v.detach() for k, v in params.items()})
    rend = pkg.Renderer(gs)
    try:
        u = pkg.camera_uniforms(pkg.make_camera(), w, h)
        weights = torch.as_tensor(_grads(h, w, seed=29)[0]).cuda()
        rgb = rend.differentiable_render(u, **params)
        assert tuple(rgb.shape) == (h, w, 3) and rgb.dtype == torch.float32
        host, _ = rend.render_host(u)                          # the same frame once more ...
        assert np.array_equal(rgb.detach().cpu().numpy().view(np.uint32), host[..., :3].view(np.uint32))
        with pytest.raises(RuntimeError, match="rendered frame"):   # ... so a backward of the first is refused
            (weights * rgb).sum().backward()
        assert all(v.grad is None for v in params.values())

        rgb = rend.differentiable_render(u, **params)
        (weights * rgb).sum().backward()
        d = rend.blend_backward(weights, colour=True, opacity=True, conic=True, uv=True)
        manual = rend.project_backward(**d)
        # two runs of blend_backward differ by the order of their atomic adds: each within its bound of the exact sums, and that
        # difference, propagated through the projection by the magnitudes of its partials (the reference's A on |difference|)
        verts = gs.download_vertices()
        _, u_ref, ref = oracle_frame(oracle, gs.download_records(), w, h)
        assert np.array_equal(rend.stage("tiles"), ref["tiles"])
        blend = bref.backward(oracle, ref, w, h, weights.cpu().numpy())
        g = {name: d[name].cpu().numpy() for name in INS}
        want = _want(verts, u, ref, g)
        spread = _want(verts, u, ref, {name: bref.bound(blend, name) for name in INS})["A"]
        for name in NAMES:
            got, man = params[name].grad, manual[name].cpu().numpy()
            assert got.dtype == torch.float32 and tuple(got.shape) == tuple(params[name].shape)
            got = got.cpu().numpy().astype(np.float64)
            assert (np.abs(man - want[name]) <= pref.bound(want, name)).all(), name
            tol = np.abs(man) * 2.0 ** -24 + 2.0 ** -149 + spread[name] + pref.bound(want, name)
            err = np.abs(got - man)
            print(f"{name}: worst |float32 gradient - manual| / allowed = {float((err / tol).max()):.3g}, largest gradient {np.abs(man).max():.3g}")
            assert (err <= tol).all(), name
            assert np.abs(man).max() > 0
        rgb2, alpha = rend.differentiable_render(u, **params, want_alpha=True)
        assert tuple(alpha.shape) == (h, w) and np.array_equal(rgb2.detach().cpu().numpy(), rgb.detach().cpu().numpy())
        assert np.array_equal(alpha.detach().cpu().numpy(), rend.feature_maps(alpha=True)["alpha"].cpu().numpy())
    finally:
        rend.close()
        gs.close()


def test_five_adam_steps_on_sh_dc_and_opacity_logits_lower_the_loss_every_time(pkg, gpu):
    n, w, h = RENDER_SCENE
    rec = pkg.synth.synth_records(n, seed=9, kind="A")
    rng = np.random.default_rng(31)
    target_rec = rec.copy()
    target_rec[:, 6:9] += 0.3 * rng.standard_normal((n, 3)).astype(np.float32)
    target_rec[:, 54] += 0.5 * rng.standard_normal(n).astype(np.float32)
    params = _parameters(rec, requires_grad=("sh_dc", "opacity_logits"))
    gs = pkg.Scene.from_tensors(**{k: v.detach() for k, v in params.items()})
    rend = pkg.Renderer(gs)
    try:
        u = pkg.camera_uniforms(pkg.make_camera(), w, h)
        with torch.no_grad():
            target = rend.differentiable_render(u, **_parameters(target_rec)).clone()
        opt = torch.optim.Adam([params["sh_dc"], params["opacity_logits"]], lr=0.01)
        losses = []
        for _ in range(6):
            opt.zero_grad()
            loss = ((rend.differentiable_render(u, **params) - target) ** 2).sum()
            losses.append(loss.item())
            loss.backward()
            opt.step()
        print("losses:", " ".join(f"{v:.6g}" for v in losses))
        assert losses[0] > 0 and all(b < a for a, b in zip(losses, losses[1:])), losses
    finally:
        rend.close()
        gs.close()
