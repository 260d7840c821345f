"""gs_blend_backward, gs_project_backward and Renderer.differentiable_render on the device under a moved, rotated camera, and end
to end.  Every earlier device test of the backward looks through the default camera -- view matrix diag(1, -1, -1, 1), position
(0, 0, 0) -- under which a transposed view matrix, a view direction taken from p, a slip in the translation column, or uniforms
kept from another frame leave every bit unchanged (tests/test_backward_cameras_api.py asserts exactly that of the reference).
Here the cameras are C1 and C2 of tests/backward_cameras.py, the references are the ones pinned on the CPU by that file, and the
machinery is that of tests/test_gpu_project_backward.py and tests/test_gpu_blend_backward.py: outputs that are views into larger
buffers with guard words, preloaded patterns, 8-byte-only alignment, every element against the derived bound, elements no gradient
reaches keeping their bits.  Frames are at most 72 x 64, scenes at most 1500 Gaussians."""
import numpy as np
import pytest
import torch  # at collection, before the package loads its library: both must bind the same HIP runtime

import backward_cameras as bc
import backward_reference as bref
import composed_reference as comp
import project_backward_reference as pref
import project_backward_scenes as psc
from helpers import assert_images_identical
from test_backward_cameras_api import moved_branch_frame
from test_gpu_blend_backward import SCENES, Sums, _grads
from test_gpu_blend_backward import _assert_close as _assert_blend_close
from test_gpu_lift import _offset_view
from test_gpu_project_backward import INS, NAMES, Arrays, _assert_close, _parameters, _run, _want

pytestmark = pytest.mark.gpu
_cache = {}


def _oracle(pkg, oracle, kind, cam, size=None, sh16=False):
    """(records, vertices, uniforms, stages) of the oracle's reference-mode frame of a synthetic scene under camera `cam`, on
    coefficients rounded to binary16 where the scene is read from that storage: computed once per key, never changed."""
    n, w, h = SCENES[kind]
    w, h = size or (w, h)
    key = (kind, cam, w, h, sh16)
    if key not in _cache:
        rec = pkg.synth.synth_records(n, seed=5, kind=kind)
        verts = oracle.activate_records(rec)
        if sh16:
            verts["sh"] = verts["sh"].astype(np.float16).astype(np.float32)
        u = oracle.camera_uniforms(bc.camera(oracle, cam), w, h)
        _cache[key] = (rec, verts, u, oracle.stages(verts, u))
    return _cache[key]


def _uniforms(pkg, cam, w, h):
    return pkg.camera_uniforms(bc.camera(pkg, cam), w, h)


def _blend_reference(oracle, key, ref, w, h, G, ga):
    if key not in _cache:
        _cache[key] = bref.backward(oracle, ref, w, h, G, ga)
    return _cache[key]


def _frame_of_the_mode(oracle, rend, verts, u, plain, antialiased):
    """The oracle's frame the device's is compared with.  In an antialiased frame it is the plain frame of the scene whose opacities
    are the frame's compensated ones, read from the record tap (the contract tests/test_gpu_antialiased.py pins bit for bit)."""
    if not antialiased:
        return plain, b""
    vis = plain["tiles"] != 0
    op = rend.stage("conic_opacity").reshape(-1, 4)[:, 3]
    prime = verts.copy()
    prime["scale_opacity"][vis, 3] = op[vis]
    assert (op[vis] <= verts["scale_opacity"][vis, 3]).all() and (op[vis] < verts["scale_opacity"][vis, 3]).any()
    return oracle.stages(prime, u), op[vis].tobytes()


# ------------------------------------------------------------------------------------------------ a. the whole chain
@pytest.mark.parametrize("kind,sh16,antialiased", [("A", False, False), ("A", True, True), ("T", False, True), ("T", True, False)])
@pytest.mark.parametrize("cam", bc.MOVED)
def test_render_blend_backward_project_backward_under_a_moved_camera(pkg, oracle, gpu, _sort_path, cam, kind, sh16, antialiased):
    n, w, h = SCENES[kind]
    rec, verts, u_ref, plain = _oracle(pkg, oracle, kind, cam, sh16=sh16)
    gs = pkg.Scene.from_records(rec, device=0)
    if sh16:
        gs.quantize_sh()
    rend = pkg.Renderer(gs)
    rend.set_antialiased(antialiased)
    try:
        u = _uniforms(pkg, cam, w, h)
        assert u.tobytes() == u_ref.tobytes()
        rend.render_host(u)
        assert np.array_equal(rend.stage("tiles"), plain["tiles"])
        ref, tap = _frame_of_the_mode(oracle, rend, verts, u_ref, plain, antialiased)
        G, ga = _grads(h, w)
        label = f"{cam}, kind {kind}, {'binary16' if sh16 else 'fp32'} SH, {'antialiased' if antialiased else 'reference mode'}"
        blend = _blend_reference(oracle, ("blend", cam, kind, sh16, antialiased, tap), ref, w, h, G, ga)
        sums = Sums(n, preload=1.5)
        rend.blend_backward(_offset_view(G, torch.float32, 1), _offset_view(ga, torch.float32, 1), **sums.t)
        _assert_blend_close(sums, blend, label + ": blend_backward")
        d = Sums(n)                                            # from zeros: the sums the projection takes on, still 8-byte-aligned views
        rend.blend_backward(_offset_view(G, torch.float32, 1), _offset_view(ga, torch.float32, 1), **d.t)
        _assert_blend_close(d, blend, label + ": blend_backward from zeros")
        g = {name: d.get(name) for name in INS}
        want = _want(verts, u, ref, g, antialiased, sh16)
        bc.assert_conditions(u, want["visible"], want["binds"], label)
        assert all(np.abs(want[name]).max() > 0 for name in NAMES)
        arr = Arrays(n)
        rend.project_backward(**d.t, out=dict(arr.t))
        _assert_close(arr, want, label + ": project_backward")
        rend.project_backward(**d.t, out=dict(arr.t))
        _assert_close(arr, want, label + ": project_backward, a second call into the same arrays", times=2)
        d.guards_intact()
    finally:
        rend.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ b. branches
@pytest.mark.parametrize("antialiased", [False, True], ids=["reference mode", "antialiased"])
def test_the_branch_scene_moved_together_with_its_camera(pkg, oracle, gpu, antialiased):
    """project_backward_scenes.branch_records and the default camera, both moved by backward_cameras.BRANCH_MOVE: the clamps either
    side and red at zero under a view matrix whose rotation block is asymmetric.  The needle alone is left out: after the move its
    det_raw is a difference of rounding-sized products whose sign the association decides
    (tests/test_backward_cameras_api.py, where the margins of every other Gaussian are asserted)."""
    moved, cam, u_ref, _ = moved_branch_frame(pkg, oracle)
    w, h = psc.BRANCH_FRAME
    verts = moved[:psc.BRANCH_NEEDLE].copy()
    n = len(verts)
    if "branch" not in _cache:
        _cache["branch"] = oracle.stages(verts, u_ref)
    ref = _cache["branch"]
    g = psc.random_gradients(n, seed=17)
    want = _want(verts, u_ref, ref, g, antialiased)
    assert want["binds"][list(psc.BRANCH_BEYOND_X), 0].all() and want["binds"][list(psc.BRANCH_BEYOND_Y), 1].all()
    assert want["binds"].sum() == 4 and want["visible"].all()
    V = bc.view_block(u_ref)
    assert np.abs(V - V.T).max() > 0.1
    gs = pkg.Scene.from_vertices(verts, device=0)
    rend = pkg.Renderer(gs)
    rend.set_antialiased(antialiased)
    try:
        u = pkg.camera_uniforms(cam, w, h)
        assert u.tobytes() == u_ref.tobytes()
        rend.render_host(u)
        assert (rend.stage("tiles") != 0).all() and np.array_equal(rend.stage("tiles"), ref["tiles"])
        assert rend.stage("uv_rg").reshape(-1, 4)[psc.BRANCH_RED_OFF, 2] == 0 and rend.stage("uv_rg").reshape(-1, 4)[psc.BRANCH_RED_ON, 2] > 0.5
        arr = _run(rend, g, want, n, f"moved branches, {'antialiased' if antialiased else 'reference mode'}")
        off = psc.BRANCH_RED_OFF                               # its r row stays untouched; g and b flow
        assert np.array_equal(arr.get("sh_dc")[off, 0:1].view(np.uint64), arr.pre["sh_dc"][off, 0:1].view(np.uint64))
        assert np.array_equal(arr.get("sh_rest")[off, :, 0].view(np.uint64), np.ascontiguousarray(arr.pre["sh_rest"][off, :, 0]).view(np.uint64))
        assert (arr.get("sh_dc")[off, 1:] != arr.pre["sh_dc"][off, 1:]).all()
    finally:
        rend.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ c. its own frame
def _differ(a, b, name="means"):
    return (np.abs(a[name] - b[name]) > 1000.0 * pref.bound(a, name)).any()


def test_the_pass_answers_for_the_last_frames_camera_and_size(pkg, oracle, gpu):
    kind = "T"
    n, w, h = SCENES[kind]
    g = psc.random_gradients(n, seed=23)
    rec, verts, u_default, ref_default = _oracle(pkg, oracle, kind, "default")
    _, _, u1, ref1 = _oracle(pkg, oracle, kind, "C1")
    _, _, u2, ref2 = _oracle(pkg, oracle, kind, "C2", size=(72, 40))
    w_default, w1, w2 = _want(verts, u_default, ref_default, g), _want(verts, u1, ref1, g), _want(verts, u2, ref2, g)
    geometry = ("means", "log_scales", "quats")
    assert all(_differ(w1, w_default, name) for name in geometry) and all(_differ(w2, w1, name) for name in geometry)
    assert 4 * w2["visible"].sum() >= n and not np.array_equal(w1["visible"], w2["visible"])
    gs = pkg.Scene.from_records(rec, device=0)
    rend = pkg.Renderer(gs)
    try:
        rend.render_host(_uniforms(pkg, "default", w, h))
        rend.render_host(_uniforms(pkg, "C1", w, h))
        assert np.array_equal(rend.stage("tiles"), ref1["tiles"])
        _run(rend, g, w1, n, "the default camera, then C1: the backward of C1's frame")
        rend.render_host(_uniforms(pkg, "C1", w, h))
        rend.render_host(_uniforms(pkg, "C2", 72, 40))
        assert np.array_equal(rend.stage("tiles"), ref2["tiles"])
        _run(rend, g, w2, n, "C1 at 64 x 64, then C2 at 72 x 40: the backward of C2's frame")
    finally:
        rend.close()
        gs.close()


def test_two_renderers_on_one_scene_each_answer_for_their_own_frame(pkg, oracle, gpu):
    kind = "T"
    n, w, h = SCENES[kind]
    g = psc.random_gradients(n, seed=23)
    rec, verts, u1, ref1 = _oracle(pkg, oracle, kind, "C1")
    _, _, u2, ref2 = _oracle(pkg, oracle, kind, "C2")
    w1, w2 = _want(verts, u1, ref1, g), _want(verts, u2, ref2, g)
    assert all(_differ(w2, w1, name) for name in ("means", "log_scales", "quats"))
    G, ga = _grads(h, w)
    blend1 = _blend_reference(oracle, ("blend", "C1", kind, False, False, b""), ref1, w, h, G, ga)
    gs = pkg.Scene.from_records(rec, device=0)
    r1, r2 = pkg.Renderer(gs), pkg.Renderer(gs)
    try:
        r1.render_host(_uniforms(pkg, "C1", w, h))
        r2.render_host(_uniforms(pkg, "C2", w, h))
        assert np.array_equal(r1.stage("tiles"), ref1["tiles"]) and np.array_equal(r2.stage("tiles"), ref2["tiles"])
        _run(r1, g, w1, n, "two renderers: R1 (C1) after R2 rendered")
        sums = Sums(n, preload=-0.75)
        r1.blend_backward(_offset_view(G, torch.float32, 1), _offset_view(ga, torch.float32, 1), **sums.t)
        _assert_blend_close(sums, blend1, "two renderers: blend_backward on R1 between the two projections")
        _run(r2, g, w2, n, "two renderers: R2 (C2) after R1's passes")
        _run(r1, g, w1, n, "two renderers: R1 (C1) once more")
    finally:
        r1.close()
        r2.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ d. differentiable_render
def _as_oracle(oracle, verts):
    return np.ascontiguousarray(verts, np.float32).copy().view(oracle.VERTEX_DT).reshape(-1)


def _check_float32_gradients(grads, want, spread, label, names=NAMES):
    """|float32 gradient - reference| <= |reference| 2^-24 + 2^-149 + the projection's magnitudes of the blend's bounds + the
    projection's bound: the tolerance of test_differentiable_render_is_the_two_passes_rounded_to_float32, against the chained
    references instead of the same two passes called by hand."""
    for name in names:
        got = grads[name]
        assert got.dtype == torch.float32 and tuple(got.shape) == want[name].shape, name
        got = got.cpu().numpy().astype(np.float64)
        tol = np.abs(want[name]) * 2.0 ** -24 + 2.0 ** -149 + spread[name] + pref.bound(want, name)
        err = np.abs(got - want[name])
        print(f"{label}: {name}: worst error / bound = {float((err / tol).max()):.3g}, largest gradient {np.abs(want[name]).max():.3g}")
        assert (err <= tol).all(), (label, name, float((err / tol).max()))
        assert np.abs(want[name]).max() > 0


def test_differentiable_render_under_c1_against_the_chained_references_with_grad_alpha(pkg, oracle, gpu):
    n, w, h = comp.RENDER_SCENE
    rec = pkg.synth.synth_records(n, seed=9, kind="A")
    params = _parameters(rec, requires_grad=NAMES)
    gs = pkg.Scene.from_tensors(**{k: v.detach() for k, v in params.items()})
    rend = pkg.Renderer(gs)
    try:
        u1, u2 = _uniforms(pkg, "C1", w, h), _uniforms(pkg, "C2", w, h)
        G, ga = _grads(h, w, seed=29)
        W_rgb, W_alpha = torch.as_tensor(G).cuda(), torch.as_tensor(ga).cuda()
        rgb, alpha = rend.differentiable_render(u1, **params, want_alpha=True)
        assert tuple(rgb.shape) == (h, w, 3) and tuple(alpha.shape) == (h, w)
        # the reference: the oracle's frame of the scene as the device holds it, then the two yardsticks chained
        held = gs.download_vertices()
        verts = _as_oracle(oracle, held)
        ref = oracle.stages(verts, u1)
        assert np.array_equal(rend.stage("tiles"), ref["tiles"]) and 4 * (ref["tiles"] != 0).sum() >= n
        assert_images_identical(np.concatenate([rgb.detach().cpu().numpy(), np.ones((h, w, 1), np.float32)], axis=2), ref["image"], "C1")
        want, spread, blend = comp.composed(oracle, verts, u1, ref, G, ga)
        V = bc.view_block(u1)
        assert np.abs(V - V.T).max() > 0.1 and want["binds"].any()
        ((W_rgb * rgb).sum() + (W_alpha * alpha).sum()).backward()
        _check_float32_gradients({k: v.grad for k, v in params.items()}, want, spread, "C1, rgb and alpha")
        without_alpha, _, _ = comp.composed(oracle, verts, u1, ref, G, None)
        assert (np.abs(without_alpha["means"] - want["means"]) > 1000.0 * (pref.bound(want, "means") + spread["means"])).any()

        # sh_rest=None: five gradients, the scene keeps its bands
        five = {k: v.detach().clone().requires_grad_() for k, v in params.items() if k != "sh_rest"}
        rgb, alpha = rend.differentiable_render(u1, **five, want_alpha=True)
        assert np.array_equal(gs.download_vertices().view(np.uint32), held.view(np.uint32))
        ((W_rgb * rgb).sum() + (W_alpha * alpha).sum()).backward()
        _check_float32_gradients({k: v.grad for k, v in five.items()}, want, spread, "C1, sh_rest=None", names=tuple(five))

        # a frame of C2 in between, no backward; then C1 again: nothing of C2's frame may leak into the gradients
        fresh = {k: v.detach().clone().requires_grad_() for k, v in params.items()}
        with torch.no_grad():
            rend.differentiable_render(u2, **fresh, want_alpha=True)
        assert not np.array_equal(rend.stage("tiles"), ref["tiles"])
        rgb, alpha = rend.differentiable_render(u1, **fresh, want_alpha=True)
        ((W_rgb * rgb).sum() + (W_alpha * alpha).sum()).backward()
        _check_float32_gradients({k: v.grad for k, v in fresh.items()}, want, spread, "C1 after a frame of C2")
    finally:
        rend.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ e. descent on geometry
def test_six_adam_steps_on_means_log_scales_and_quaternions_lower_the_loss_every_time(pkg, gpu):
    """Camera C1, the target rendered from perturbed means, log-scales and quaternions (composed_reference.geometry_records).  The
    learning rate is not chosen here: composed_reference.GEOMETRY_LR = 3e-3 is the largest of {1e-2, 3e-3, 1e-3, 3e-4} for which the
    CPU run -- the oracle's forward, the chained reference gradient, the same Adam -- falls at every step
    (tests/test_backward_cameras_api.py asserts that choice).  Its seven losses there:
        17.4541  14.0703  11.2633  9.0736  7.38947  6.14226  5.25778
    (at 1e-2 the CPU run rises once, 4.67932 -> 4.75464).  The assertion here is monotone decrease and nothing tighter."""
    n, w, h = comp.RENDER_SCENE
    rec, target_rec = comp.geometry_records(pkg.synth)
    moving = ("means", "log_scales", "quats")
    params = _parameters(rec, requires_grad=moving)
    gs = pkg.Scene.from_tensors(**{k: v.detach() for k, v in params.items()})
    rend = pkg.Renderer(gs)
    try:
        u = _uniforms(pkg, comp.GEOMETRY_CAMERA, w, h)
        with torch.no_grad():
            target = rend.differentiable_render(u, **_parameters(target_rec)).clone()
        opt = torch.optim.Adam([params[k] for k in moving], lr=comp.GEOMETRY_LR)
        losses = []
        for step in range(comp.GEOMETRY_STEPS + 1):            # seven losses, six steps: as the CPU run
            opt.zero_grad()
            loss = ((rend.differentiable_render(u, **params) - target) ** 2).sum()
            losses.append(loss.item())
            loss.backward()
            assert all(params[k].grad is not None and params[k].grad.abs().max() > 0 for k in moving)
            if step < comp.GEOMETRY_STEPS:
                opt.step()
        print(f"lr {comp.GEOMETRY_LR:g}: losses " + " ".join(f"{v:.6g}" for v in losses))
        assert losses[0] > 0 and all(b < a for a, b in zip(losses, losses[1:])), losses
    finally:
        rend.close()
        gs.close()
