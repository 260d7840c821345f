"""gs_camera_backward on the device (gs_camera_backward.hip) against its definition restated in numpy
(tests/camera_backward_reference.py, pinned to torch.autograd by tests/test_camera_backward_api.py), and
Renderer.differentiable_render_posed over the whole chain.  The inputs are the sums of a real blend_backward of a random grad_rgb /
grad_alpha; the 27 sums are compared within the bound that module derives,
    |got - (x + want)| <= (2 K_PATH + n_visible + C_SUM) 2^-53 S + 2^-53 |x|;     an element with S = 0 keeps its bits,
row 3 of d_view_mat and row 2 of d_proj_mat among them.  Outputs are views into larger device buffers with guard words, preloaded
with a pattern, 8-byte aligned and nothing more.  Frames are 64 x 48 to 160 x 96."""
import ctypes as C

import numpy as np
import pytest
import torch  # at collection, before the package loads its library: both must bind the same HIP runtime

import backward_cameras as bc
import camera_backward_reference as cref
import composed_pose_reference as cpose
import project_backward_reference as pref
import project_backward_scenes as psc
from composed_reference import RENDER_SCENE
from helpers import oracle_frame
from test_gpu_blend_backward import _grads
from test_gpu_lift import GUARD, SENTINEL
from test_gpu_project_backward import SCENES, _small_scene

pytestmark = pytest.mark.gpu

NAMES = tuple(cref.OUTPUTS)
INS = tuple(pref.INPUTS)
BINDING = {("A", "C1"): (9, 10), ("T", "C2"): (48, 35), ("T", "C1"): (27, 13), ("A", "C2"): (43, 70)}   # Gaussians whose x / y clamp binds
PATTERN = np.array([1.5, -0.0, -2.25, 0.0078125, -640.0, 0.0, 3.0e-9])
_cache = {}


class Arrays:
    """The three outputs as float64 views into larger device buffers: a pattern in the views, a sentinel in the guard words."""

    def __init__(self, only=NAMES, zeros=False):
        self.buf, self.t, self.pre = {}, {}, {}
        for i, name in enumerate(only):
            size = cref.OUTPUTS[name]
            pre = np.zeros(size) if zeros else PATTERN[(np.arange(size) * 5 + i) % len(PATTERN)]
            self.buf[name] = torch.full((size + 2 * GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
            self.t[name] = self.buf[name][GUARD:GUARD + size]
            self.t[name].copy_(torch.as_tensor(pre))
            self.pre[name] = pre.copy()
            assert self.t[name].data_ptr() % 8 == 0 and self.t[name].data_ptr() % 16 != 0

    def kwargs(self):
        return {name: self.t.get(name) for name in NAMES}

    def get(self, name):
        return self.t[name].cpu().numpy()

    def guards_intact(self):
        for name, b in self.buf.items():
            g = torch.cat([b[:GUARD], b[-GUARD:]]).cpu().numpy()
            assert (g == SENTINEL).all(), f"{name}: a guard word was written"


def _assert_close(arr, want, label, times=1):
    arr.guards_intact()
    for name in arr.t:
        got, pre = arr.get(name), arr.pre[name]
        lim = cref.bound(want, name, pre, times)
        err = np.abs(got - (pre + times * want[name]))
        print(f"{label}: {name}: worst error / bound = {float((err / np.maximum(lim, 1e-300)).max()):.3g}, largest |sum| {np.abs(want[name]).max():.3g}")
        bad = np.nonzero(~(err <= lim))[0]
        assert len(bad) == 0, f"{label}: {name}[{bad[0]}] = {got[bad[0]]!r} against {(pre + times * want[name])[bad[0]]!r}, bound {lim[bad[0]]:.3g}"
        untouched = want["A"][name] == 0
        assert np.array_equal(got[untouched].view(np.uint64), pre[untouched].view(np.uint64)), f"{label}: {name}: an element no gradient reaches changed"
        assert untouched[list(cref.UNTOUCHED[name])].all()


def _oracle(oracle, key, rec, w, h, cam="default", sh16=False):
    key = (key, cam, sh16)
    if key not in _cache:
        verts, u, ref = oracle_frame(oracle, rec, w, h, bc.camera(oracle, cam))
        if sh16:
            verts["sh"] = verts["sh"].astype(np.float16).astype(np.float32)
            ref = oracle.stages(verts, u)
        _cache[key] = (verts, u, ref)
    return _cache[key]


def _open(pkg, rec, w, h, cam="default", sh16=False, antialiased=False):
    gs = pkg.Scene.from_records(rec, device=0)
    if sh16:
        gs.quantize_sh()
    rend = pkg.Renderer(gs)
    rend.set_antialiased(antialiased)
    return gs, rend, pkg.camera_uniforms(bc.camera(pkg, cam), w, h)


def _blend(rend, h, w, seed=41):
    """The four sums of a real blend_backward of a random grad_rgb / grad_alpha: (device tensors, numpy copies)."""
    G, ga = _grads(h, w, seed=seed)
    d = rend.blend_backward(torch.as_tensor(G).cuda(), torch.as_tensor(ga).cuda(), colour=True, opacity=True, conic=True, uv=True)
    return d, {name: d[name].cpu().numpy() for name in INS}


def _want(verts, u, ref, g, antialiased=False, sh16=False):
    fields = pref.unpack_vertices(verts, sh16=sh16)
    return cref.backward(*fields, u, ref["tiles"] != 0, ref["attr"]["color_radii"][:, 0] > 0, colour=g["colour"], opacity_grad=g["opacity"],
                         conic=g["conic"], uv=g["uv"], antialiased=antialiased)


# ------------------------------------------------------------------------------------------------ 1. frames, cameras, storage, modes
@pytest.mark.parametrize("kind,cam,sh16,antialiased", [("A", "default", False, False), ("A", "C1", True, True), ("T", "C2", False, True),
                                                       ("T", "C1", True, False), ("A", "C2", False, False)])
def test_render_blend_backward_camera_backward_on_small_frames(pkg, oracle, gpu, _sort_path, kind, cam, sh16, antialiased):
    n, w, h = SCENES[kind]
    rec = pkg.synth.synth_records(n, seed=5, kind=kind)
    verts, u_ref, ref = _oracle(oracle, ("synth", kind), rec, w, h, cam, sh16)
    gs, rend, u = _open(pkg, rec, w, h, cam, sh16, antialiased)
    try:
        assert u.tobytes() == u_ref.tobytes()
        rend.render_host(u)
        assert np.array_equal(rend.stage("tiles"), ref["tiles"])
        d, g = _blend(rend, h, w)
        want = _want(verts, u, ref, g, antialiased, sh16)
        if cam in bc.MOVED:                                    # both clamps bind, the view is asymmetric, the camera off the origin
            bc.assert_conditions(u, want["visible"], want["binds"], f"{kind}, {cam}")
            assert tuple(want["binds"].sum(axis=0)) == BINDING[kind, cam], want["binds"].sum(axis=0)
        assert want["n_visible"] > n // 4 and all(np.abs(want[name]).max() > 0 for name in NAMES)
        label = f"kind {kind}, {cam}, {'binary16' if sh16 else 'fp32'} SH, {'antialiased' if antialiased else 'reference mode'}"
        arr = Arrays()
        out = rend.camera_backward(**d, **arr.kwargs())
        assert sorted(out) == sorted(NAMES)
        _assert_close(arr, want, label)                        # pre-filled: the ADD shows; rows 3 / 2 keep the pattern
        first = {name: arr.get(name).copy() for name in NAMES}
        rend.camera_backward(**d, **arr.kwargs())
        _assert_close(arr, want, label + ", a second call into the same arrays", times=2)
        a, b = Arrays(zeros=True), Arrays(zeros=True)          # two calls on the same frame with the same inputs: the same bits
        rend.camera_backward(**d, **a.kwargs())
        rend.camera_backward(**d, **b.kwargs())
        for name in NAMES:
            assert np.array_equal(a.get(name).view(np.uint64), b.get(name).view(np.uint64)), name
            assert np.array_equal((a.get(name) + PATTERN[(np.arange(len(first[name])) * 5 + NAMES.index(name)) % len(PATTERN)]).view(np.uint64)
                                  [want["A"][name] > 0], first[name].view(np.uint64)[want["A"][name] > 0]), name   # one add per element
        fresh = rend.camera_backward(**d)                      # zeros allocated by the wrapper
        for name in NAMES:
            assert fresh[name].dtype == torch.float64 and np.array_equal(fresh[name].cpu().numpy().view(np.uint64), a.get(name).view(np.uint64))
        for only in (("view_mat",), ("proj_mat",), ("camera_position",), ("view_mat", "camera_position")):   # NULL-output subsets
            part = Arrays(only=only, zeros=True)
            assert sorted(rend.camera_backward(**d, **part.kwargs())) == sorted(only)
            part.guards_intact()
            for name in only:
                assert np.array_equal(part.get(name).view(np.uint64), a.get(name).view(np.uint64)), (only, name)
        assert rend.camera_backward(**d, view_mat=None, proj_mat=None, camera_position=None) == {}
        assert pkg.binding.lib().gs_camera_backward(rend._h, C.byref(pkg.binding.CameraGrads())) == 0
    finally:
        rend.close()
        gs.close()


def test_a_scene_read_through_its_copy_in_spatial_order(pkg, oracle, gpu, monkeypatch):
    monkeypatch.setenv("GS_SPATIAL_MIN", "1")                  # the scene gets its copy in spatial order at 1 500 Gaussians
    n, w, h = SCENES["T"]
    rec = pkg.synth.synth_records(n, seed=5, kind="T")
    verts, u_ref, ref = _oracle(oracle, ("synth", "T"), rec, w, h, "C1")
    gs, rend, u = _open(pkg, rec, w, h, "C1")
    try:
        rend.render_host(u)
        assert np.array_equal(rend.stage("tiles"), ref["tiles"])
        d, g = _blend(rend, h, w)
        arr = Arrays()
        rend.camera_backward(**d, **arr.kwargs())
        _assert_close(arr, _want(verts, u, ref, g), "spatial order, T, C1")
    finally:
        rend.close()
        gs.close()


TEETH = {"clamp_not_binding": 1000.0, "no_a_term": 100.0, "no_column_3": 10.0}


@pytest.mark.parametrize("cam", bc.MOVED)
def test_one_well_conditioned_gaussian_whose_clamp_binds_where_the_bound_is_its_own(pkg, oracle, gpu, cam):
    """On a whole scene the bound is the worst-conditioned splats'.  Here the scene is ONE Gaussian of scene A: of those whose
    clamp binds under the camera, the one whose term is best conditioned; the inputs are seeded random gradients (an isolated
    splat at the frame's edge gets none from a blend).  The device stays within the bound, and it misses the reference with the
    clamp treated as not binding, without the A = J V term or without column 3 by more than TEETH bounds -- figures a tenth or
    less of how far those mutated references lie from the true one (7e298 -- an element whose true term is an exact zero --,
    205 and 27 bounds under C1; more under C2), which is all a device within one bound of the true one can differ from them."""
    n, w, h = SCENES["A"]
    full = pkg.synth.synth_records(n, seed=5, kind="A")
    g_full = psc.random_gradients(n)
    verts, u_ref, ref = _oracle(oracle, ("synth", "A"), full, w, h, cam)
    probe = _want(verts, u_ref, ref, g_full, antialiased=True)
    ids = np.nonzero(probe["visible"])[0]
    ratio = probe["term_A"]["view_mat"].max(axis=1) / np.maximum(np.abs(probe["terms"]["view_mat"]).max(axis=1), 1e-300)
    binding = probe["binds"][ids].any(axis=1)
    keep = ids[binding][np.argsort(ratio[binding])[:1]]
    rec, g = np.ascontiguousarray(full[keep]), {k: np.ascontiguousarray(v[keep]) for k, v in g_full.items()}
    verts, u_ref, ref = _oracle(oracle, ("binding one", cam), rec, w, h, cam)
    assert (ref["tiles"] != 0).all()
    gs, rend, u = _open(pkg, rec, w, h, cam, antialiased=True)
    try:
        rend.render_host(u)
        assert np.array_equal(rend.stage("tiles"), ref["tiles"])
        want = _want(verts, u, ref, g, antialiased=True)
        assert want["binds"].any() and all(np.abs(want[name]).max() > 0 for name in NAMES)
        arr = Arrays(zeros=True)
        rend.camera_backward(**{k: torch.as_tensor(v).cuda() for k, v in g.items()}, **arr.kwargs())
        _assert_close(arr, want, f"one binding Gaussian, {cam}")
        fields = pref.unpack_vertices(verts)
        for mutation, bounds in TEETH.items():
            bent = cref.backward(*fields, u, ref["tiles"] != 0, ref["attr"]["color_radii"][:, 0] > 0, colour=g["colour"], opacity_grad=g["opacity"],
                                 conic=g["conic"], uv=g["uv"], antialiased=True, mutate=mutation)
            miss = np.abs(arr.get("view_mat") - bent["view_mat"]) / np.maximum(cref.bound(want, "view_mat"), 1e-300)
            print(f"{cam}: {mutation}: the device misses the mutated reference by up to {float(miss.max()):.3g} bounds")
            assert miss.max() > bounds, mutation
    finally:
        rend.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ 2. sizes and lane patterns
def _sized(n, keep):
    """_small_scene(n) with only the Gaussians `keep` left in view (None: all); the others stand behind the camera."""
    rec, w, h = _small_scene(n)
    if keep is not None:
        hidden = np.ones(n, bool)
        hidden[list(keep)] = False
        rec[hidden, 2] = 2.0
    return rec, w, h


SIZES = {"1": (1, None), "63": (63, None), "64": (64, None), "65": (65, None), "last lane of the last wave only": (256 + 128, (256 + 127,)),
         "one per workgroup": (3 * 256 + 5, (3, 256 + 200, 2 * 256 + 64, 3 * 256 + 4)), "none": (64, ())}


@pytest.mark.parametrize("case", list(SIZES))
def test_sizes_around_one_wave_single_lanes_and_a_scene_with_every_gaussian_culled(pkg, oracle, gpu, case):
    n, keep = SIZES[case]
    rec, w, h = _sized(n, keep)
    verts, u_ref, ref = _oracle(oracle, ("sized", case), rec, w, h)
    assert (ref["tiles"] != 0).sum() == (n if keep is None else len(keep))
    gs, rend, u = _open(pkg, rec, w, h)
    try:
        rend.render_host(u)
        assert np.array_equal(rend.stage("tiles"), ref["tiles"])
        d, g = _blend(rend, h, w)
        if keep == ():                                         # nothing blended: give the pass inputs all the same
            g = {k: np.random.default_rng(3).standard_normal(v.shape) for k, v in g.items()}
            d = {k: torch.as_tensor(v).cuda() for k, v in g.items()}
        want = _want(verts, u, ref, g)
        arr = Arrays()
        rend.camera_backward(**d, **arr.kwargs())
        _assert_close(arr, want, case)
        if keep == ():                                         # every Gaussian culled: outputs bit-unchanged
            for name in NAMES:
                assert np.array_equal(arr.get(name).view(np.uint64), arr.pre[name].view(np.uint64)), name
        else:
            assert all(np.abs(want[name]).max() > 0 for name in NAMES)
    finally:
        rend.close()
        gs.close()


def test_one_gaussian_more_than_the_launch_has_lanes_is_reached_by_the_stride(pkg, oracle, gpu):
    """GS_CAMERA_BACKWARD_LANES lanes are launched at most (include/gs3d_hip.h); Gaussian LANES is lane 0's second one.  All but
    200 Gaussians stand behind the camera, so the frame stays cheap; the oracle sees the 200 alone (a Gaussian's visibility and
    record do not depend on the others), and the device's tiles tap is asserted to agree with it on the whole scene."""
    lanes = pkg.binding.CAMERA_BACKWARD_LANES
    n = lanes + 1
    small, w, h = _small_scene(200)
    keep = np.concatenate([np.arange(199), [lanes]])
    rec = np.repeat(small[:1], n, axis=0)
    rec[:, 2] = 2.0                                            # behind the camera
    rec[keep] = small
    assert n > lanes and keep[-1] == lanes                     # the wrap: slot `lanes` belongs to no lane's first round
    verts, u_ref, ref = _oracle(oracle, "stride", small, w, h)
    assert (ref["tiles"] != 0).all()
    gs, rend, u = _open(pkg, rec, w, h)
    try:
        rend.render_host(u)
        tiles = rend.stage("tiles")
        assert np.array_equal(np.nonzero(tiles)[0], keep) and np.array_equal(tiles[keep], ref["tiles"])
        d, g = _blend(rend, h, w)
        want = _want(verts, u, ref, {k: v[keep] for k, v in g.items()})
        arr = Arrays()
        rend.camera_backward(**d, **arr.kwargs())
        _assert_close(arr, want, f"{n} Gaussians")
        last = cref.backward(*pref.unpack_vertices(verts), u, np.arange(200) == 199, ref["attr"]["color_radii"][:, 0] > 0,
                             colour=g["colour"][keep], opacity_grad=g["opacity"][keep], conic=g["conic"][keep], uv=g["uv"][keep])
        without = {name: want[name] - last[name] for name in NAMES}   # the sums had the wrapped Gaussian been skipped
        assert any((np.abs(arr.get(name) - arr.pre[name] - without[name]) > cref.bound(want, name, arr.pre[name])).any() for name in NAMES)
    finally:
        rend.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ 3. NaN, the frame, refusals
def test_a_nan_in_a_culled_row_changes_nothing_and_one_in_a_visible_row_arrives(pkg, oracle, gpu):
    n, w, h = SCENES["A"]
    rec = pkg.synth.synth_records(n, seed=5, kind="A")
    verts, u_ref, ref = _oracle(oracle, ("synth", "A"), rec, w, h, "C1")
    gs, rend, u = _open(pkg, rec, w, h, "C1")
    try:
        rend.render_host(u)
        d, g = _blend(rend, h, w)
        vis = ref["tiles"] != 0
        clean = Arrays(zeros=True)
        rend.camera_backward(**d, **clean.kwargs())
        culled = {k: v.clone() for k, v in d.items()}
        for k in culled:
            culled[k][torch.as_tensor(~vis).cuda()] = float("nan")
        arr = Arrays(zeros=True)
        rend.camera_backward(**culled, **arr.kwargs())
        for name in NAMES:
            assert np.array_equal(arr.get(name).view(np.uint64), clean.get(name).view(np.uint64)), name
        v = int(np.nonzero(vis)[0][7])
        for member, reached in (("conic", ("view_mat",)), ("uv", ("proj_mat",)), ("colour", ("camera_position",))):
            poisoned = {k: t.clone() for k, t in d.items()}
            poisoned[member][v] = float("nan")
            arr = Arrays(zeros=True)
            rend.camera_backward(**poisoned, **arr.kwargs())
            for name in NAMES:
                got = arr.get(name)
                touched = np.ones(len(got), bool)
                touched[list(cref.UNTOUCHED[name])] = False
                if name in reached:
                    assert np.isnan(got[touched]).all() and (got[~touched] == 0).all(), (member, name)
                else:
                    assert np.array_equal(got.view(np.uint64), clean.get(name).view(np.uint64)), (member, name)
    finally:
        rend.close()
        gs.close()


def test_the_pass_answers_for_the_last_frame_its_camera_its_size_and_its_mode(pkg, oracle, gpu):
    n = SCENES["A"][0]
    rec = pkg.synth.synth_records(n, seed=5, kind="A")
    gs = pkg.Scene.from_records(rec, device=0)
    rend = pkg.Renderer(gs)
    try:
        with pytest.raises(pkg.binding.GsError) as e:
            rend.camera_backward()
        assert e.value.code == -1 and "no frame" in str(e.value)
        assert pkg.binding.lib().gs_camera_backward(rend._h, C.byref(pkg.binding.CameraGrads())) == -1   # nothing asked for: still no frame
        for cam, (w, h), aa in (("C1", (72, 40), True), ("C2", (160, 96), False)):
            verts, u_ref, ref = _oracle(oracle, ("synth", "A", w, h), rec, w, h, cam)
            rend.set_antialiased(aa)
            u = pkg.camera_uniforms(bc.camera(pkg, cam), w, h)
            rend.render_host(u)
            rend.set_antialiased(not aa)                       # a setter made after the frame does not count
            d, g = _blend(rend, h, w)
            arr = Arrays()
            rend.camera_backward(**d, **arr.kwargs())
            _assert_close(arr, _want(verts, u, ref, g, antialiased=aa), f"{cam} at {w} x {h}")
        big = torch.zeros(64, dtype=torch.float64, device="cuda")
        L, CG = pkg.binding.lib(), pkg.binding.CameraGrads
        for member, _ in CG._fields_:
            s = CG(d_view_mat=big.data_ptr(), d_proj_mat=big.data_ptr() + 128, d_camera_position=big.data_ptr() + 256)
            setattr(s, member, big.data_ptr() + 4)
            assert L.gs_camera_backward(rend._h, C.byref(s)) == -1 and b"aligned" in L.gs_last_error(), member
        assert (big == 0).all()
    finally:
        rend.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ 4. differentiable_render_posed
def _parameters(rec, requires_grad=()):
    n = len(rec)
    p = dict(means=rec[:, 0:3], log_scales=rec[:, 55:58], quats=rec[:, 58:62], opacity_logits=rec[:, 54], sh_dc=rec[:, 6:9],
             sh_rest=rec[:, 9:54].reshape(n, 3, 15).transpose(0, 2, 1))
    return {k: torch.tensor(np.ascontiguousarray(v, np.float32), device="cuda", requires_grad=k in requires_grad) for k, v in p.items()}


def test_the_pose_gradient_of_differentiable_render_posed_is_autograd_of_the_one_composed_function(pkg, oracle, gpu, monkeypatch):
    """The float32 pose gradient against torch.autograd of ONE float64 function from the pose to the loss
    (tests/composed_pose_reference.py).  The margin, computed here: the float32 rounding of the returned gradient, plus how far
    two evaluations within the references' bounds may lie apart -- the camera reference's bound and its magnitudes of the blend's
    bounds, carried to the pose by the absolute Jacobian of the uniforms -- taken twice, once for the device and once for the
    replay of the blend in binary64 that autograd differentiates."""
    n, w, h = RENDER_SCENE
    rec = pkg.synth.synth_records(n, seed=9, kind="A")
    gs = pkg.Scene.from_records(rec, device=0)
    rend = pkg.Renderer(gs)
    try:
        c1 = bc.CAMERAS["C1"]
        position = torch.tensor(c1["position"], dtype=torch.float32, requires_grad=True)
        rotation = torch.tensor(c1["rotation"], dtype=torch.float32, device="cuda", requires_grad=True)
        G, ga = _grads(h, w, seed=29)
        calls = []
        monkeypatch.setattr(rend, "project_backward", lambda *a, **k: calls.append(1))
        rgb, alpha = rend.differentiable_render_posed(w, h, position, rotation, fov=c1["fov"], want_alpha=True)
        cam = pkg.make_camera(position=position.detach().numpy(), rotation=rotation.detach().cpu().numpy(), fov=c1["fov"])
        u = pkg.camera_uniforms(cam, w, h)
        verts, u_ref, ref = oracle_frame(oracle, rec, w, h, cam.view(oracle.CAMERA_DT))
        assert u.tobytes() == u_ref.tobytes() and np.array_equal(rend.stage("tiles"), ref["tiles"])
        ((torch.as_tensor(G).cuda() * rgb).sum() + (torch.as_tensor(ga).cuda() * alpha).sum()).backward()
        assert not calls, "project_backward ran although no scene tensor asks for a gradient"
        assert position.grad.dtype == torch.float32 and position.grad.device.type == "cpu" and tuple(position.grad.shape) == (3,)
        assert rotation.grad.dtype == torch.float32 and rotation.grad.device.type == "cuda" and tuple(rotation.grad.shape) == (4,)
        got = np.concatenate([position.grad.numpy(), rotation.grad.cpu().numpy()]).astype(np.float64)
        dp, dq, margin, want = cpose.chained(oracle, verts, cam, u, ref, G, ga)
        ap, aq = cpose.composed_autograd(oracle, verts, cam, u, ref, G, ga)
        auto = np.concatenate([ap, aq])
        tol = np.abs(auto) * 2.0 ** -24 + 2.0 ** -149 + 2.0 * margin
        err = np.abs(got - auto)
        print("pose gradient", got, "autograd", auto, "chained references", np.concatenate([dp, dq]))
        print(f"worst |float32 gradient - autograd| / allowed = {float((err / tol).max()):.3g}; / |gradient| = {float((err / np.abs(auto)).max()):.3g}")
        assert (err <= tol).all() and np.abs(auto).min() > 0
        # a sanity figure beside the derived margin (which the worst-conditioned splats make wide): the binary32 walk against its
        # binary64 replay moves this scene's gradient by 1e-7 of its size on the CPU (tests/test_camera_backward_api.py)
        assert err.max() <= (2.0 ** -23 + 1e-5) * np.abs(auto).max()
        with pytest.raises(RuntimeError, match="rendered frame"):   # one backward per forward
            rgb2 = rend.differentiable_render_posed(w, h, position, rotation, fov=c1["fov"])
            rend.render_host(u)
            rgb2.sum().backward()
    finally:
        rend.close()
        gs.close()


def test_adam_on_the_pose_alone_finds_its_way_back_to_c1(pkg, gpu, monkeypatch):
    """The scene held, the target rendered at C1, the pose started composed_pose_reference.POSE_TWIST away; torch's Adam (lr
    POSE_LR = 5e-4) on float32 position and rotation through differentiable_render_posed, POSE_STEPS = 16 steps.  The float64 run
    of the same loop on the CPU references (composed_pose_reference.reference_descent, asserted by
    tests/test_camera_backward_api.py) falls at each of its first 10 steps and ends at 0.801 of the pose error it started with;
    the device loop is held to its first POSE_MONOTONE = 8 steps falling and to POSE_DEVICE_FACTOR = 0.82 of its start: the
    reference's factor plus a margin of 0.02 for float32 parameters (derived at those constants).
    No scene tensor requires a gradient: project_backward must not run (it is patched to count)."""
    n, w, h = RENDER_SCENE
    rec = pkg.synth.synth_records(n, seed=9, kind="A")
    gs = pkg.Scene.from_records(rec, device=0)
    rend = pkg.Renderer(gs)
    try:
        target_pose, start = cpose.descent_start(pkg)
        fov = bc.CAMERAS["C1"]["fov"]
        calls = []
        monkeypatch.setattr(rend, "project_backward", lambda *a, **k: calls.append(1))
        with torch.no_grad():
            target = rend.differentiable_render_posed(w, h, torch.tensor(target_pose[0]), torch.tensor(target_pose[1]), fov=fov).clone()
        position = torch.tensor(start[0], dtype=torch.float32, requires_grad=True)
        rotation = torch.tensor(start[1], dtype=torch.float32, requires_grad=True)
        opt = torch.optim.Adam([position, rotation], lr=cpose.POSE_LR)
        losses, errors = [], []
        for step in range(cpose.POSE_STEPS + 1):
            errors.append(cpose.pose_error((position.detach().numpy().astype(np.float64), rotation.detach().numpy().astype(np.float64)), target_pose))
            opt.zero_grad()
            loss = ((rend.differentiable_render_posed(w, h, position, rotation, fov=fov) - target) ** 2).sum()
            losses.append(loss.item())
            if step == cpose.POSE_STEPS:
                break
            loss.backward()
            opt.step()
        print("losses:", " ".join(f"{v:.6g}" for v in losses))
        print("pose errors:", " ".join(f"{v:.4g}" for v in errors))
        first = losses[:cpose.POSE_MONOTONE + 1]
        assert losses[0] > 0 and all(b < a for a, b in zip(first, first[1:])), losses
        assert errors[-1] < cpose.POSE_DEVICE_FACTOR * errors[0], errors
        assert not calls, "project_backward ran although no scene tensor requires a gradient"
    finally:
        rend.close()
        gs.close()
