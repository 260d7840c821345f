"""gs_camera_backward / gs_camera_uniforms_backward / Renderer.camera_backward without a GPU.  The yardstick the GPU tests compare
with (tests/camera_backward_reference.py) is pinned here: its sums are the gradients torch.autograd finds for an independent
float64 restatement of the record function F with the uniforms as leaves (tests/camera_record_torch.py) within the bound the
module derives, under the default camera and the moved, rotated cameras of tests/backward_cameras.py, antialiased on and off,
fp32 and binary16 SH; each single-term mutation of it fails that comparison on some camera.  Then the host half
(gs_camera_uniforms_backward) against torch.autograd of the real function behind gs_camera_uniforms and against central
differences of gs_camera_uniforms itself, the entry point's refusals, the structure's layout and the wrapper's tensor checks."""
import ctypes as C
import os

import numpy as np
import pytest

import backward_cameras as bc
import camera_backward_reference as cref
import camera_record_torch as crt
import project_backward_reference as pref
import project_backward_scenes as psc
from helpers import forbid_c, hand_made_renderer, oracle_frame
from test_project_backward_api import SCENES

INVALID = -1
_frames = {}


def frame(pkg, oracle, kind, cam, sh16=False):
    """(records, width, height, oracle vertices, uniforms, oracle stages): computed once, never changed."""
    key = (kind, cam, sh16)
    if key not in _frames:
        if kind == "branch":
            rec, (w, h) = psc.branch_records(), psc.BRANCH_FRAME
        else:
            n, w, h = SCENES[kind]
            rec = pkg.synth.synth_records(n, seed=5, kind=kind)
        verts, u, ref = oracle_frame(oracle, rec, w, h, bc.camera(oracle, cam))
        if sh16:
            verts["sh"] = verts["sh"].astype(np.float16).astype(np.float32)
            ref = oracle.stages(verts, u)
        _frames[key] = (rec, w, h, verts, u, ref)
    return _frames[key]


def reference(pkg, oracle, kind, cam, antialiased=False, sh16=False, mutate=None):
    key = ("want", kind, cam, antialiased, sh16, mutate)
    if key not in _frames:
        rec, w, h, verts, u, ref = frame(pkg, oracle, kind, cam, sh16)
        g = psc.random_gradients(len(rec))
        _frames[key] = cref.backward(*pref.unpack_vertices(verts, sh16=sh16), u, ref["tiles"] != 0, ref["attr"]["color_radii"][:, 0] > 0,
                                     colour=g["colour"], opacity_grad=g["opacity"], conic=g["conic"], uv=g["uv"], antialiased=antialiased,
                                     mutate=mutate)
    return _frames[key]


def autograd(pkg, oracle, kind, cam, antialiased=False, sh16=False):
    key = ("autograd", kind, cam, antialiased, sh16)
    if key not in _frames:
        rec, w, h, verts, u, ref = frame(pkg, oracle, kind, cam, sh16)
        g = psc.random_gradients(len(rec))
        view, proj, c = crt.leaves_of(u)
        f = crt.forward(verts, u, ref["tiles"] != 0, ref["attr"]["color_radii"][:, 0] > 0, antialiased, sh16, view, proj, c)
        crt.loss(f, g).backward()
        _frames[key] = crt.gradients(view, proj, c)
    return _frames[key]


def _worst(got, want):
    """{name: worst |got - want| / bound}; an element with S = 0 must be an exact zero on both sides."""
    worst = {}
    for name in cref.OUTPUTS:
        lim, err = cref.bound(want, name), np.abs(got[name] - want[name])
        assert ((lim > 0) | (err == 0)).all(), name
        worst[name] = float((err / np.maximum(lim, 1e-300)).max())
    return worst


# ------------------------------------------------------------------------------------------------ 1. autograd
CASES = [(kind, cam) for kind in ("A", "T") for cam in bc.CAMERAS] + [("branch", "default")]


@pytest.mark.parametrize("sh16", [False, True], ids=["fp32", "binary16"])
@pytest.mark.parametrize("antialiased", [False, True], ids=["reference mode", "antialiased"])
@pytest.mark.parametrize("kind,cam", CASES)
def test_the_sums_are_the_gradients_autograd_finds_with_the_uniforms_as_leaves(pkg, oracle, kind, cam, antialiased, sh16):
    rec, w, h, verts, u, ref = frame(pkg, oracle, kind, cam, sh16)
    want = reference(pkg, oracle, kind, cam, antialiased, sh16)
    if cam in bc.MOVED:     # the test must not pass on a frame where no clamp binds or the view is symmetric
        bc.assert_conditions(u, want["visible"], want["binds"], f"{kind}, {cam}")
    if kind == "branch":
        assert want["binds"].sum() == 4 and want["visible"].all()
    got = autograd(pkg, oracle, kind, cam, antialiased, sh16)
    print(f"counted roundings: {want['k']}, visible {want['n_visible']}")
    worst = _worst(got, want)
    for name in cref.OUTPUTS:
        print(f"{kind}, {cam}: {name}: worst error / bound = {worst[name]:.3g}, largest |sum| {np.abs(want[name]).max():.3g}")
        assert np.abs(want[name]).max() > 0, name
        assert worst[name] <= 1.0, (name, worst[name])
        for e in cref.UNTOUCHED[name]:          # row 3 of V and row 2 of P: F does not read them
            assert want[name][e] == 0 and want["A"][name][e] == 0 and got[name][e] == 0, (name, e)
    assert max(want["k"].values()) <= cref.K_PATH


def test_the_counted_path_constant_is_what_the_docstring_and_the_header_state(pkg, oracle):
    """K_PATH bounds the count on every call (asserted there); the largest the arithmetic counts is an antialiased frame's."""
    ks = {aa: reference(pkg, oracle, "T", "C1", antialiased=aa)["k"] for aa in (False, True)}
    print(ks)
    assert ks[True]["view_mat"] >= ks[False]["view_mat"]
    assert cref.K_PATH - 50 <= ks[True]["view_mat"] <= cref.K_PATH
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gs3d_hip.h")).read()
    body = header[header.index("The camera half of the backward"):header.index("} gs_camera_grads;")]
    assert f"{cref.K_PATH} * 2^-53" in body and f"(n_visible + {cref.C_SUM}) * 2^-53" in body


# ------------------------------------------------------------------------------------------------ 2. mutations
def _alone(pkg, oracle, kind, cam, i, mutate=None):
    """(reference, autograd) of the frame with Gaussian i as its ONLY visible one, antialiased: the sum is that Gaussian's term."""
    rec, w, h, verts, u, ref = frame(pkg, oracle, kind, cam)
    g = psc.random_gradients(len(rec))
    only = np.zeros(len(rec), bool)
    only[i] = True
    red = ref["attr"]["color_radii"][:, 0] > 0
    want = cref.backward(*pref.unpack_vertices(verts), u, only, red, colour=g["colour"], opacity_grad=g["opacity"], conic=g["conic"], uv=g["uv"],
                         antialiased=True, mutate=mutate)
    view, proj, c = crt.leaves_of(u)
    crt.loss(crt.forward(verts, u, only, red, True, False, view, proj, c), g).backward()
    return want, crt.gradients(view, proj, c)


@pytest.mark.parametrize("mutation", cref.MUTATIONS)
def test_each_mutation_of_the_reference_fails_against_autograd_on_some_camera(pkg, oracle, mutation):
    """A sum's bound is the SUM of its terms' magnitudes, so on a whole scene the few worst-conditioned Gaussians (a conic's
    gradient through a thin splat: magnitudes 1e17 times the term) set a bound no single-term slip can exceed.  The teeth are
    therefore shown where the bound is a term's own: frames in which ONE Gaussian is visible -- the four best-conditioned of
    scene A under each camera (for the clamp's mutation: of those whose clamp binds), where the unmutated reference still
    agrees with autograd within its bound and the mutated one misses it by more than a thousand bounds."""
    failed = {}
    for cam in bc.CAMERAS:
        full = reference(pkg, oracle, "A", cam, antialiased=True)
        ids = np.nonzero(full["visible"])[0]
        ratio = full["term_A"]["view_mat"].max(axis=1) / np.maximum(np.abs(full["terms"]["view_mat"]).max(axis=1), 1e-300)
        eligible = full["binds"][ids].any(axis=1) if mutation == "clamp_not_binding" else np.ones(len(ids), bool)
        if not eligible.any():
            continue
        worst = 0.0
        for i in ids[eligible][np.argsort(ratio[eligible])[:4]]:
            true, got = _alone(pkg, oracle, "A", cam, int(i))
            assert max(_worst(got, true).values()) <= 1.0
            bent, _ = _alone(pkg, oracle, "A", cam, int(i), mutate=mutation)
            worst = max(worst, max(float((np.abs(got[name] - bent[name]) / np.maximum(cref.bound(true, name), 1e-300)).max())
                                   for name in cref.OUTPUTS))
        failed[cam] = worst
        print(f"{mutation}: A, {cam}: worst error / bound = {worst:.3g}")
    assert max(failed.values()) > 1000.0, failed
    if mutation == "clamp_not_binding":      # only a camera under which a clamp binds can see it
        assert failed["C1"] > 1000.0 and failed["C2"] > 1000.0


# ------------------------------------------------------------------------------------------------ 3. the host half
POSES = {"C1": bc.CAMERAS["C1"], "C2": bc.CAMERAS["C2"],
         "non-unit quaternion": dict(position=(0.3, -0.2, 0.5), rotation=(1.1, 0.25, -0.3, 0.15), fov=50.0)}
SIZE = (160, 96)


def _pose_loss(pkg, name, gv, gp, gc, position=None, rotation=None):
    """(loss, position leaf, rotation leaf): sum(gv view) + sum(gp proj) + sum(gc camera_position) of crt.pose_uniforms at the
    camera's binary32 values (or at the given float64 ones), gv and gp laid out as the uniforms' matrices."""
    import torch
    cam = pkg.make_camera(**POSES[name])
    p = torch.tensor(np.asarray(cam["position"][0] if position is None else position, np.float64), requires_grad=True)
    q = torch.tensor(np.asarray(cam["rotation"][0] if rotation is None else rotation, np.float64), requires_grad=True)
    view, proj, c = crt.pose_uniforms(p, q, float(cam["fov"][0]), float(cam["near_plane"][0]), float(cam["far_plane"][0]), *SIZE)
    T = lambda a: torch.tensor(np.asarray(a, np.float64))  # noqa: E731
    return (T(gv).reshape(4, 4).T * view).sum() + (T(gp).reshape(4, 4).T * proj).sum() + (T(gc) * c).sum(), p, q


def _host_backward(pkg, cam, gv, gp, gc):
    dp, dq = np.zeros(3), np.zeros(4)
    L = pkg.binding.lib()
    assert L.gs_camera_uniforms_backward(pkg.binding._p(cam), C.c_uint32(SIZE[0]), C.c_uint32(SIZE[1]), pkg.binding._p(gv), pkg.binding._p(gp),
                                         pkg.binding._p(gc), pkg.binding._p(dp), pkg.binding._p(dq)) == 0, L.gs_last_error()
    return dp, dq


@pytest.mark.parametrize("name", list(POSES))
def test_the_host_half_is_autograd_of_the_real_function_behind_camera_uniforms(pkg, name):
    """The tolerance is the binary64 condition bound of g_M = -M^-T g M^-T: an inverse computed in binary64 by any stable method
    is within 8 u cond(M) |M^-1| of exact (n = 4, both the adjugate here and torch's LU); it enters g_M twice (16 u cond |M^-1|^2 G,
    G = |g_view| + |persp| |g_proj| in Frobenius / spectral norms), the two 4-term products and persp^T g_proj add 12 roundings
    of quantities no larger -- under 32 u cond |M^-1|^2 G a side, 64 for the two sides.  d_rotation sums 8 entries of g_M times
    at most 4 |q|_inf each (plus 8 roundings): 40 |q|_inf times that."""
    import torch
    rng = np.random.default_rng(5)
    gv, gp, gc = rng.standard_normal(16), rng.standard_normal(16), rng.standard_normal(3)
    cam = pkg.make_camera(**POSES[name])
    loss, p, q = _pose_loss(pkg, name, gv, gp, gc)
    loss.backward()
    dp, dq = _host_backward(pkg, cam, gv, gp, gc)
    via_wrapper = pkg.camera_pose_gradient(cam, *SIZE, dict(view_mat=gv, proj_mat=gp, camera_position=gc))
    assert np.array_equal(via_wrapper[0], dp) and np.array_equal(via_wrapper[1], dq)
    with torch.no_grad():
        view, proj, _ = crt.pose_uniforms(p, q, float(cam["fov"][0]), float(cam["near_plane"][0]), float(cam["far_plane"][0]), *SIZE)
    flip = np.array([1.0, -1.0, -1.0, 1.0])[:, None]
    Minv = view.numpy() * flip
    M = np.linalg.inv(Minv)
    persp = (proj.numpy() * np.array([1.0, -1.0, 1.0, 1.0])[:, None]) @ M
    ginv, cond = np.linalg.norm(Minv, 2), np.linalg.cond(M, 2)
    G = np.linalg.norm(gv) + np.linalg.norm(persp, 2) * np.linalg.norm(gp)
    tol_m = 64.0 * 2.0 ** -53 * cond * ginv ** 2 * G
    tol_p = tol_m + 2.0 ** -52 * np.abs(gc)
    tol_q = 40.0 * np.abs(q.detach().numpy()).max() * tol_m
    err_p, err_q = np.abs(dp - p.grad.numpy()), np.abs(dq - q.grad.numpy())
    print(f"{name}: |M^-1| {ginv:.3g}, cond {cond:.3g}; position error / tol {float((err_p / tol_p).max()):.3g}, rotation {float(err_q.max() / tol_q):.3g}")
    assert (err_p <= tol_p).all() and (err_q <= tol_q).all()
    assert np.abs(dp).min() > 1e-3 and np.abs(dq).min() > 1e-3
    if name == "non-unit quaternion":       # the raw quaternion's gradient has a radial part: nothing was normalised
        assert abs(float(np.dot(dq, q.detach().numpy()))) > 1e-3


@pytest.mark.parametrize("name", list(POSES))
def test_the_host_half_against_central_differences_of_the_real_camera_uniforms(pkg, name):
    """A sanity bound: gs_camera_uniforms is binary32.  STEP h = 2^-7: the difference quotient of a binary32 function carries its
    rounding error over 2 h, the truncation error falls with h^2 -- at 2^-7 both are some 1e-4 of the gradient's size, the minimum
    of their sum to within a factor of two.  The two parts are bounded apart.  ROUNDING: the same quotient of the float64
    function at the SAME two points differs only by the uniforms' binary32 errors -- an inverse by cofactors, a 4 x 4 product:
    under 64 ulp of max(1, |u|) per element, asserted below -- times |g|, over the points' distance.  TRUNCATION: Richardson --
    the float64 quotient at h is within 4/3 |q(h) - q(h/2)| of the derivative, doubled for slack in the estimate."""
    rng = np.random.default_rng(5)
    gv, gp, gc = rng.standard_normal(16), rng.standard_normal(16), rng.standard_normal(3)
    cam = pkg.make_camera(**POSES[name])
    dp, dq = _host_backward(pkg, cam, gv, gp, gc)
    analytic = np.concatenate([dp, dq])
    h = 2.0 ** -7

    def value32(c):
        u = pkg.camera_uniforms(c, *SIZE)[0]
        return float(np.dot(gv, u["view_mat"].astype(np.float64)) + np.dot(gp, u["proj_mat"].astype(np.float64))
                     + np.dot(gc, u["camera_position"][:3].astype(np.float64)))

    def value64(position, rotation):
        return float(_pose_loss(pkg, name, gv, gp, gc, position, rotation)[0].detach())

    for i in range(7):
        field, j = ("position", i) if i < 3 else ("rotation", i - 3)
        hi, lo = cam.copy(), cam.copy()
        hi[field][0, j] += np.float32(h)
        lo[field][0, j] -= np.float32(h)
        dist = float(hi[field][0, j]) - float(lo[field][0, j])
        fd32 = (value32(hi) - value32(lo)) / dist
        args = lambda c: (c["position"][0].astype(np.float64), c["rotation"][0].astype(np.float64))  # noqa: E731
        fd64 = (value64(*args(hi)) - value64(*args(lo))) / dist
        u_hi = pkg.camera_uniforms(hi, *SIZE)[0]
        scale = sum(float(np.dot(np.abs(g), np.maximum(1.0, np.abs(u_hi[k].astype(np.float64)[:len(g)]))))
                    for g, k in ((gv, "view_mat"), (gp, "proj_mat"), (gc, "camera_position")))
        rounding = 2.0 * 64.0 * 2.0 ** -24 * scale / dist
        half = cam.copy(), cam.copy()
        half[0][field][0, j] += np.float32(h / 2)
        half[1][field][0, j] -= np.float32(h / 2)
        fd64_half = (value64(*args(half[0])) - value64(*args(half[1]))) / (float(half[0][field][0, j]) - float(half[1][field][0, j]))
        truncation = 2.0 * (4.0 / 3.0) * abs(fd64 - fd64_half) + 2.0 ** -40 * abs(fd64)
        print(f"{name}: {field}[{j}]: analytic {analytic[i]:.6g}, float32 quotient {fd32:.6g}; rounding bound {rounding:.3g}, truncation bound {truncation:.3g}")
        assert abs(fd32 - fd64) <= rounding, (field, j)
        assert abs(fd64 - analytic[i]) <= truncation, (field, j)


def test_the_reference_pose_descent_falls_and_ends_at_the_factor_the_device_test_is_held_to(pkg, oracle):
    """The float64 loop the device's pose refinement (tests/test_gpu_camera_backward.py) takes its figures from."""
    import composed_pose_reference as cpose
    losses, errors = cpose.reference_descent(pkg, oracle)
    print("losses:", " ".join(f"{v:.6g}" for v in losses))
    print("pose errors:", " ".join(f"{v:.4g}" for v in errors))
    first = losses[:cpose.POSE_REFERENCE_MONOTONE + 1]
    assert len(losses) == cpose.POSE_STEPS + 1 and all(b < a for a, b in zip(first, first[1:])), losses
    assert abs(errors[-1] / errors[0] - cpose.POSE_REFERENCE_FACTOR) < 0.005, errors
    assert cpose.POSE_MONOTONE < cpose.POSE_REFERENCE_MONOTONE and cpose.POSE_DEVICE_FACTOR > cpose.POSE_REFERENCE_FACTOR


def test_the_chained_pose_references_are_autograd_of_the_one_composed_function(pkg, oracle):
    """Pose -> uniforms -> record -> image: the references chained against ONE float64 torch function.  The chained side walks
    the blend in binary32 as the definition does, autograd differentiates the binary64 replay of its decisions: the two differ
    by the walk's binary32 roundings, some 2^-24 of each pair's term -- far inside the chained margin, which is asserted, and
    within 1e-5 of the gradient's own size, which is printed and asserted as a sanity figure of this scene."""
    import composed_pose_reference as cpose
    from composed_reference import RENDER_SCENE
    from test_blend_backward_api import _grads
    n, w, h = RENDER_SCENE
    verts = oracle.activate_records(pkg.synth.synth_records(n, seed=9, kind="A"))
    for name in bc.MOVED:
        cam = bc.camera(oracle, name)
        u = oracle.camera_uniforms(cam, w, h)
        ref = oracle.stages(verts, u)
        G, ga = _grads(h, w, seed=29)
        dp, dq, margin, want = cpose.chained(oracle, verts, cam, u, ref, G, ga)
        ap, aq = cpose.composed_autograd(oracle, verts, cam, u, ref, G, ga)
        err = np.abs(np.concatenate([dp, dq]) - np.concatenate([ap, aq]))
        size = np.abs(np.concatenate([ap, aq])).max()
        print(f"{name}: worst error / margin = {float((err / margin).max()):.3g}; worst error / largest gradient = {float(err.max() / size):.3g}")
        assert (err <= margin).all() and err.max() <= 1e-5 * size and size > 1.0


# ------------------------------------------------------------------------------------------------ 4. the C entry points
IN_MEMBERS = ("d_colour", "d_opacity", "d_conic", "d_uv")
OUT_MEMBERS = ("d_view_mat", "d_proj_mat", "d_camera_position")


def _refused(pkg, rc, word):
    assert rc == INVALID
    msg = pkg.binding.lib().gs_last_error()
    assert msg and word in msg, msg


def test_invalid_arguments_are_refused_without_a_device(pkg):
    L, CG = pkg.binding.lib(), pkg.binding.CameraGrads
    fake = C.c_void_p(8)              # (r is not dereferenced before every member of g has been checked)
    _refused(pkg, L.gs_camera_backward(None, C.byref(CG())), b"null")
    _refused(pkg, L.gs_camera_backward(fake, None), b"null")
    _refused(pkg, L.gs_camera_backward(None, None), b"null")
    for member in IN_MEMBERS + OUT_MEMBERS:
        for offset in (4, 2, 1):
            g = CG(**{m: 8192 for m in IN_MEMBERS + OUT_MEMBERS})
            setattr(g, member, 8192 + offset)
            _refused(pkg, L.gs_camera_backward(fake, C.byref(g)), b"aligned")
    _refused(pkg, L.gs_camera_backward(fake, C.byref(CG(d_conic=4096 + 4))), b"aligned")   # nothing asked for: still refused
    cam, z16, z3, o3, o4 = pkg.make_camera(), np.zeros(16), np.zeros(3), np.zeros(3), np.zeros(4)
    p = pkg.binding._p
    good = [p(cam), C.c_uint32(64), C.c_uint32(48), p(z16), p(z16), p(z3), p(o3), p(o4)]
    assert L.gs_camera_uniforms_backward(*good) == 0
    for i in (0, 3, 4, 5, 6, 7):
        _refused(pkg, L.gs_camera_uniforms_backward(*[None if k == i else a for k, a in enumerate(good)]), b"null")
    for i in (1, 2):
        _refused(pkg, L.gs_camera_uniforms_backward(*[C.c_uint32(0) if k == i else a for k, a in enumerate(good)]), b"empty")


def test_the_structure_has_the_headers_layout(pkg):
    CG = pkg.binding.CameraGrads
    names = list(IN_MEMBERS + OUT_MEMBERS)
    assert [f[0] for f in CG._fields_] == names
    assert C.sizeof(CG) == 56 and [getattr(CG, k).offset for k in names] == [0, 8, 16, 24, 32, 40, 48]
    assert "gs_camera_backward" in pkg.binding.SYMBOLS and "gs_camera_uniforms_backward" in pkg.binding.SYMBOLS
    assert "gs_camera_backward.hip" in pkg.binding.KERNEL_SOURCES and "gs_project_chain.h" in pkg.binding.KERNEL_SOURCES
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gs3d_hip.h")).read()
    body = header[:header.index("} gs_camera_grads;")]
    body = body[body.rindex("typedef struct"):]
    order = [body.index(" " + m + ";") for m in names]
    assert order == sorted(order), "the header declares the members in another order"
    assert f"#define GS_CAMERA_BACKWARD_LANES {pkg.binding.CAMERA_BACKWARD_LANES}u" in header


def test_the_wrapper_checks_its_tensors_before_it_reaches_c(pkg, monkeypatch):
    from test_project_backward_api import _Fake

    forbid_c(pkg, monkeypatch)
    rend = hand_made_renderer(pkg, frame_hw=(40, 72))
    ins = dict(colour=_Fake((100, 3)), opacity=_Fake((100,)), conic=_Fake((100, 3)), uv=_Fake((100, 2)))
    outs = dict(view_mat=_Fake((16,)), proj_mat=_Fake((16,)), camera_position=_Fake((3,)))
    with pytest.raises(AssertionError, match="C library was reached"):   # everything in order: the call goes through to C
        rend.camera_backward(**ins, **outs)
    with pytest.raises(AssertionError, match="C library was reached"):
        rend.camera_backward(uv=ins["uv"], view_mat=outs["view_mat"], proj_mat=None, camera_position=None)
    bad = [("colour", _Fake((100, 3), "torch.float32"), TypeError), ("conic", _Fake((99, 3)), ValueError), ("uv", _Fake((100, 2), device="cpu"), ValueError),
           ("view_mat", _Fake((4, 4)), ValueError), ("proj_mat", _Fake((16,), "torch.float32"), TypeError), ("camera_position", _Fake((4,)), ValueError),
           ("view_mat", _Fake((16,), device="cuda:1"), ValueError), ("camera_position", _Fake((3,), contiguous=False), ValueError)]
    for name, tensor, error in bad:
        with pytest.raises(error, match=name):
            rend.camera_backward(**dict(ins, **dict(outs, **{name: tensor})))
    with pytest.raises(TypeError, match="unknown"):
        pkg.camera_pose_gradient(pkg.make_camera(), 64, 48, dict(view=np.zeros(16)))
    with pytest.raises(ValueError, match="proj_mat"):
        pkg.camera_pose_gradient(pkg.make_camera(), 64, 48, dict(proj_mat=np.zeros(12)))
