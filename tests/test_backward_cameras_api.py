"""The yardsticks of gs_blend_backward and gs_project_backward under a moved, rotated camera, and end to end, without a GPU.

Every earlier test of the two passes looks through the default camera (tests/backward_cameras.py), whose view matrix is
diag(1, -1, -1, 1) and whose position is the origin.  Here:
  1a  four single-term mutations -- the view matrix read transposed in each of its three uses, the view direction taken from p --
      change NO BIT under that camera (the gap, written down) and move some element by more than a thousand bounds under C1 and C2;
  1b  tests/project_backward_reference.py against torch.autograd under C1 and C2, with the bound of the default camera's test;
  1c  the forward value of the record function F that the reference differentiates, against np_reference.preprocess fed the same
      exact inputs (derived bound) and against the oracle's binary32 record (the tolerances of tests/float64_check.py);
  1d  the seam between the two passes: the two references chained against ONE float64 torch function from parameters to image
      (tests/composed_reference.py), and two deliberate slips at the seam that it notices;
  2b  the branch scene of tests/project_backward_scenes.py moved together with its camera still stands on the intended side of
      every branch;
  2e  six Adam steps on means, log-scales and quaternions with the oracle's forward and the composed reference gradient: the
      learning rate tests/test_gpu_backward_cameras.py uses is the largest of four for which the loss falls at every step."""
import contextlib

import numpy as np
import pytest

import aa_reference as aa
import backward_cameras as bc
import composed_reference as comp
import float64_cases as fc
import float64_check as f64
import np_reference as npr
import project_backward_reference as pref
import project_backward_scenes as psc
import transform_reference as tref
from helpers import oracle_frame
from test_blend_backward_api import _grads
from test_project_backward_api import SCENES, _autograd

CAMERA_MUTATIONS = ("view_transposed", "view_transposed_in_a", "view_transposed_in_g_j", "camera_at_origin")
_frames = {}


def frame(pkg, oracle, kind, cam, sh16=False):
    """(records, width, height, oracle vertices, uniforms, oracle stages) of a synthetic scene under a camera of
    backward_cameras.CAMERAS, on coefficients rounded to binary16 where asked: computed once, never changed."""
    key = (kind, cam, sh16)
    if key not in _frames:
        n, w, h = SCENES[kind]
        rec = pkg.synth.synth_records(n, seed=5, kind=kind)
        verts, u, ref = oracle_frame(oracle, rec, w, h, bc.camera(oracle, cam))
        if sh16:
            verts["sh"] = verts["sh"].astype(np.float16).astype(np.float32)
            ref = oracle.stages(verts, u)
        _frames[key] = (rec, w, h, verts, u, ref)
    return _frames[key]


def reference(pkg, oracle, kind, cam, antialiased=False, sh16=False, k=15, mutate=None):
    rec, w, h, verts, u, ref = frame(pkg, oracle, kind, cam, sh16)
    g = psc.random_gradients(len(rec))
    return pref.backward(*pref.unpack_vertices(verts, sh16=sh16), u, ref["tiles"] != 0, ref["attr"]["color_radii"][:, 0] > 0,
                         colour=g["colour"], opacity_grad=g["opacity"], conic=g["conic"], uv=g["uv"], antialiased=antialiased,
                         sh_rest_coeffs=k, mutate=mutate)


# ------------------------------------------------------------------------------------------------ 0. the cameras
@pytest.mark.parametrize("kind", ["A", "T"])
@pytest.mark.parametrize("cam", bc.MOVED)
def test_the_moved_cameras_keep_the_scene_in_view_bind_both_clamps_and_are_asymmetric(pkg, oracle, kind, cam):
    rec, w, h, verts, u, ref = frame(pkg, oracle, kind, cam)
    want = reference(pkg, oracle, kind, cam)
    bc.assert_conditions(u, want["visible"], want["binds"], f"{kind}, {cam}")
    # the premise of taking the clamps' branches from the binary32 restatement: its depth is the frame's, bit for bit
    pv, _, _, _ = pref.clamp_branches(pref.unpack_vertices(verts)[0], u[0])
    vis = ref["tiles"] != 0
    assert np.array_equal(pv[vis, 2].view(np.uint32), ref["attr"]["depth"][vis].view(np.uint32))


def test_the_default_camera_is_the_one_the_gap_is_about(pkg, oracle):
    u = oracle.camera_uniforms(bc.camera(oracle, "default"), 72, 40)
    assert np.array_equal(np.asarray(u[0]["view_mat"]).reshape(4, 4), np.diag([1.0, -1.0, -1.0, 1.0]).astype(np.float32))
    assert not np.asarray(u[0]["camera_position"]).reshape(-1)[:3].any()
    assert u.tobytes() == oracle.camera_uniforms(oracle.default_camera(), 72, 40).tobytes()
    assert bc.camera(pkg, "C1").tobytes() == bc.camera(oracle, "C1").tobytes()


# ------------------------------------------------------------------------------------------------ 1a. mutations
@pytest.mark.parametrize("kind", ["A", "T"])
@pytest.mark.parametrize("mutation", CAMERA_MUTATIONS)
def test_under_the_default_camera_the_camera_mutations_change_no_bit(pkg, oracle, mutation, kind):
    """The gap: a reference -- or a kernel -- with this slip passes every test that looks through the default camera."""
    assert mutation in pref.MUTATIONS
    want = reference(pkg, oracle, kind, "default", antialiased=True)
    bent = reference(pkg, oracle, kind, "default", antialiased=True, mutate=mutation)
    for name in pref.OUTPUTS:
        assert np.abs(want[name]).max() > 0
        assert np.array_equal(bent[name].view(np.uint64), want[name].view(np.uint64)), name
        assert np.array_equal(bent["A"][name].view(np.uint64), want["A"][name].view(np.uint64)), name
    for name in pref.RECORD:
        assert np.array_equal(bent["record"][name][0].view(np.uint64), want["record"][name][0].view(np.uint64)), name


MOVES = {"view_transposed": "means", "view_transposed_in_a": "log_scales", "view_transposed_in_g_j": "means", "camera_at_origin": "means"}


@pytest.mark.parametrize("kind", ["A", "T"])
@pytest.mark.parametrize("cam", bc.MOVED)
@pytest.mark.parametrize("mutation", CAMERA_MUTATIONS)
def test_under_the_moved_cameras_each_camera_mutation_moves_an_element_by_more_than_a_thousand_bounds(pkg, oracle, mutation, cam, kind):
    want = reference(pkg, oracle, kind, cam)
    bent = reference(pkg, oracle, kind, cam, mutate=mutation)
    name = MOVES[mutation]
    moved = np.abs(bent[name] - want[name]) / np.maximum(pref.bound(want, name), 1e-300)
    print(f"{mutation}, {kind}, {cam}: {name} moves by up to {float(moved.max()):.3g} bounds")
    assert moved.max() > 1000.0
    if mutation == "camera_at_origin":       # the basis values themselves: d_sh_rest, which the default camera's suite cannot bend
        rest = np.abs(bent["sh_rest"] - want["sh_rest"]) / np.maximum(pref.bound(want, "sh_rest"), 1e-300)
        assert rest.max() > 1000.0


# ------------------------------------------------------------------------------------------------ 1b. autograd
@pytest.mark.parametrize("k", [0, 15])
@pytest.mark.parametrize("sh16", [False, True], ids=["fp32", "binary16"])
@pytest.mark.parametrize("antialiased", [False, True], ids=["reference mode", "antialiased"])
@pytest.mark.parametrize("kind", ["A", "T"])
@pytest.mark.parametrize("cam", bc.MOVED)
def test_under_the_moved_cameras_the_sums_are_the_gradients_autograd_finds(pkg, oracle, cam, kind, antialiased, sh16, k):
    rec, w, h, verts, u, ref = frame(pkg, oracle, kind, cam, sh16)
    g = psc.random_gradients(len(rec))
    want = reference(pkg, oracle, kind, cam, antialiased, sh16, k)
    got = _autograd(verts, u, ref["tiles"] != 0, ref["attr"]["color_radii"][:, 0] > 0, g, antialiased, sh16, k)
    for name in pref.OUTPUTS:
        assert got[name].shape == want[name].shape, name
        if want[name].size == 0:
            continue
        err, lim = np.abs(got[name] - want[name]), pref.bound(want, name)
        assert np.abs(want[name]).max() > 0
        print(f"{name}: worst error / bound = {float((err / np.maximum(lim, 1e-300)).max()):.3g}")
        bad = np.argwhere(~(err <= lim))
        assert len(bad) == 0, (name, len(bad), tuple(bad[0]), got[name][tuple(bad[0])], want[name][tuple(bad[0])], lim[tuple(bad[0])])
        assert (want[name][~want["visible"]] == 0).all()


# ------------------------------------------------------------------------------------------------ 1c. F's value
@contextlib.contextmanager
def _binary32_sh_constants():
    """np_reference evaluates the SH polynomial with the constants' decimal values; the frame holds them in binary32.  For the
    comparison of two binary64 evaluations of the same inputs the constants are inputs: np_reference gets the frame's."""
    saved = (npr.SH_C0, npr.SH_C1, npr.SH_C2, npr.SH_C3)
    npr.SH_C0, npr.SH_C1, npr.SH_C2, npr.SH_C3 = pref.SH_C0, pref.SH_C1, list(pref.SH_C2), list(pref.SH_C3)
    try:
        yield
    finally:
        npr.SH_C0, npr.SH_C1, npr.SH_C2, npr.SH_C3 = saved


def _np_reference_from_the_frames_inputs(verts, u, sh16, frustum):
    """np_reference.preprocess on the stored binary32 values (pref.unpack_vertices) and the frame's binary32 uniforms, all
    converted exactly; every binary32 constant of the frame likewise."""
    pos, scale, quat, opac, sh = (a.astype(np.float64) for a in pref.unpack_vertices(verts, sh16=sh16))
    scene = dict(pos=pos, scale=scale, opacity=opac, rot=quat / np.sqrt((quat * quat).sum(axis=1, keepdims=True)), sh=sh)
    u0 = u[0]
    cam = dict(proj=np.asarray(u0["proj_mat"], np.float64).reshape(4, 4).T, view=np.asarray(u0["view_mat"], np.float64).reshape(4, 4).T,
               tan_fovx=float(np.float32(u0["tan_fovx"])), tan_fovy=float(np.float32(u0["tan_fovy"])),
               cam=np.asarray(u0["camera_position"], np.float64).reshape(-1)[:3], width=int(u0["width"]), height=int(u0["height"]))
    with _binary32_sh_constants():
        return npr.preprocess(scene, cam, dict(near=float(np.float32(0.2)), dilation=pref.DILATION, frustum=frustum))


@pytest.mark.parametrize("sh16", [False, True], ids=["fp32", "binary16"])
@pytest.mark.parametrize("kind", ["A", "T"])
@pytest.mark.parametrize("cam", list(bc.CAMERAS))
def test_the_forward_value_of_f_is_np_references_from_the_same_inputs_within_the_counted_roundings(pkg, oracle, cam, kind, sh16):
    """Both sides are binary64 evaluations of identical inputs, so the tolerance is the module's own: 2 k 2^-53 magnitude of the
    forward triple, k counted by the arithmetic.  Two things np_reference does differently are inputs too and are given to it:
    the SH constants (above), and the clamp's limit -- the frame multiplies tz with the binary32 product 1.3f * tan_fov, np_reference
    with frustum * tan_fov in binary64.  One `frustum` serves one axis (frustum = limit / tan_fov: two more roundings, k + 2), so a
    Gaussian whose x clamp binds is compared with the run made for x, one whose y clamp binds with the run made for y, and one
    where BOTH bind (a corner) is left to the comparison with the oracle below; the test asserts these stay few.
    The antialiased opacity: np_reference returns the dilated matrix only, and aa_reference.comp64 takes det_raw from
    (a + 0.3) - 0.3, whose two roundings of a value of magnitude a + 0.3 the counted magnitudes know nothing of: they enter as
    d(a0) <= 2 u a, d(c0) <= 2 u c, so d(det_raw) <= 2 u (a |c0| + c |a0|) and d(o comp) <= o comp d(det_raw) / (2 det_raw).
    Derived, added to the bound of that one field."""
    rec, w, h, verts, u, ref = frame(pkg, oracle, kind, cam, sh16)
    vis, red = ref["tiles"] != 0, ref["attr"]["color_radii"][:, 0] > 0
    fields = pref.unpack_vertices(verts, sh16=sh16)
    record = {aa_: pref.backward(*fields, u, vis, red, antialiased=aa_)["record"] for aa_ in (False, True)}
    binds = pref.backward(*fields, u, vis, red)["binds"]
    _, _, _, lim = pref.clamp_branches(fields[0], u[0])
    tans = (float(np.float32(u[0]["tan_fovx"])), float(np.float32(u[0]["tan_fovy"])))
    runs = [_np_reference_from_the_frames_inputs(verts, u, sh16, float(lim[a]) / tans[a]) for a in (0, 1)]
    both = binds.all(axis=1)
    assert both.sum() <= vis.sum() // 20, (both.sum(), vis.sum())
    use_y = binds[:, 1] & ~both
    pick = lambda key: np.where((use_y[:, None] if runs[0][key].ndim > 1 else use_y), runs[1][key], runs[0][key])  # noqa: E731
    rows = vis & ~both
    assert rows.sum() > len(rec) // 4
    assert np.array_equal(pick("rgb")[vis, 0] > 0, red[vis]), "np_reference and the frame decide red's clamp differently"

    def check(name, got, npv, extra=0.0, more_k=0):
        val, mag, k = got
        err = np.abs(val - npv.reshape(val.shape))[rows]
        tol = (2.0 * (k + more_k) * pref.U53 * mag + extra)[rows]
        print(f"{cam}, {kind}: {name}: worst error / bound = {float((err / np.maximum(tol, 1e-300)).max()):.3g}  (k = {k + more_k})")
        assert (err <= tol).all(), (name, float((err / np.maximum(tol, 1e-300)).max()))

    check("uv", record[False]["uv"], pick("uv"))
    check("conic", record[False]["conic"], pick("conic"), more_k=2)
    check("opacity", record[False]["opacity"], pick("opacity"))
    check("rgb", record[False]["rgb"], pick("rgb"))
    raw = record[False]["rgb_raw"]
    assert np.array_equal(raw[0][rows][:, 1:], record[False]["rgb"][0][rows][:, 1:])
    assert np.array_equal(raw[0][rows & red, 0], record[False]["rgb"][0][rows & red, 0]) and (record[False]["rgb"][0][rows & ~red, 0] == 0).all()
    assert (raw[0][rows & ~red, 0] <= 0).all()
    pre = {key: pick(key) for key in ("cov2d", "det", "opacity")}
    a, b, c = pre["cov2d"].T
    a0, c0 = a - pref.DILATION, c - pref.DILATION
    det_raw = a0 * c0 - b * b
    want = pre["opacity"] * aa.comp64(pre, dict(dilation=pref.DILATION))
    with np.errstate(divide="ignore", invalid="ignore"):
        extra = np.where(det_raw > 0, want * 2.0 * pref.U53 * (a * np.abs(c0) + c * np.abs(a0)) / (2.0 * det_raw), 0.0)
    rows = rows & (det_raw > 0) & (record[True]["opacity"][0][:, 0] > 0)      # (where both sides hold a factor, not the constant 0)
    assert rows.sum() > len(rec) // 4
    check("opacity after the antialiased factor", record[True]["opacity"], want, extra=extra[:, None], more_k=2)
    for name in ("uv", "conic", "rgb"):      # the mode changes the opacity alone
        assert np.array_equal(record[True][name][0][vis], record[False][name][0][vis])


@pytest.mark.parametrize("sh16", [False, True], ids=["fp32", "binary16"])
@pytest.mark.parametrize("kind", ["A", "T"])
@pytest.mark.parametrize("cam", list(bc.CAMERAS))
def test_the_forward_value_of_f_is_the_oracles_binary32_record_within_float64_checks_tolerances(pkg, oracle, cam, kind, sh16):
    """The tolerances are float64_check.reference()'s per-Gaussian err of conic, uv, rgb and opacity: SLACK x the modelled
    uncertainty of one binary32 evaluation (K_COV ulp of the covariance's terms over lambda_min for the conic, K_UV ulp of
    |uv| + W + H plus the view transform's error through the focal length for uv, K_RGB ulp of 1 + 3 sum |SH| for rgb, K_OPACITY
    ulp for the opacity), justified there for binary64 against the oracle's binary32 -- the comparison made here, on every visible
    Gaussian and both clamps' branches.  Reference mode only: the oracle has no antialiased mode (the device's factor is compared
    with float64 by tests/test_gpu_antialiased.py)."""
    rec, w, h, verts, u, ref = frame(pkg, oracle, kind, cam, sh16)
    vis, red = ref["tiles"] != 0, ref["attr"]["color_radii"][:, 0] > 0
    record = pref.backward(*pref.unpack_vertices(verts, sh16=sh16), u, vis, red)["record"]
    c = bc.CAMERAS[cam]
    err = f64.reference(fc.Frame(f"{kind}, {cam}", rec, position=c["position"], rotation=c["rotation"], fov=c["fov"], width=w, height=h,
                                 sh16=sh16))["err"]
    attr = ref["attr"]
    for name, oracles in (("uv", attr["uv"][:, :2]), ("conic", attr["conic_opacity"][:, :3]), ("opacity", attr["conic_opacity"][:, 3:4]),
                          ("rgb", attr["color_radii"][:, :3])):
        d = np.abs(record[name][0] - oracles.astype(np.float64))[vis]
        ratio = d / err[name][vis][:, None]
        print(f"{cam}, {kind}: {name}: worst |F - oracle| / float64_check's tolerance = {float(ratio.max()):.3g}")
        assert (ratio <= 1.0).all(), name
    assert vis.sum() > len(rec) // 4


# ------------------------------------------------------------------------------------------------ 1d. the seam
_seams = {}


def _render_frame(pkg, oracle, cam, antialiased):
    """(vertices, uniforms, oracle stages, grad_rgb, grad_alpha) of composed_reference.RENDER_SCENE under `cam`: computed once."""
    key = (cam, antialiased)
    if key not in _seams:
        n, w, h = comp.RENDER_SCENE
        verts = oracle.activate_records(pkg.synth.synth_records(n, seed=9, kind="A"))
        u = oracle.camera_uniforms(bc.camera(oracle, cam), w, h)
        G, ga = _grads(h, w, seed=29)
        _seams[key] = (verts, u, comp.frame(oracle, verts, u, antialiased), G, ga)
    return _seams[key]


def _seam(pkg, oracle, cam, antialiased, bend=None):
    """(worst |autograd - chained references| / tolerance per output, want): tolerance = the projection's bound + the projection's
    magnitudes of the blend's own bounds -- both derived; the second is how far two evaluations of the blend's sums may differ,
    carried through the projection by the absolute values of its partials."""
    verts, u, ref, G, ga = _render_frame(pkg, oracle, cam, antialiased)
    want, spread, blend = comp.composed(oracle, verts, u, ref, G, ga, antialiased, binary64=True, bend=bend)
    key = (cam, antialiased, "autograd")
    if key not in _seams:
        _seams[key] = comp.composed_autograd(verts, u, ref, blend["pairs"], G, ga, antialiased)
    got = _seams[key]
    worst = {}
    for name in comp.NAMES:
        tol = pref.bound(want, name) + spread[name]
        err = np.abs(got[name] - want[name])
        assert ((tol > 0) | (err == 0)).all(), name
        worst[name] = float((err / np.maximum(tol, 1e-300)).max())
    return worst, want


@pytest.mark.parametrize("antialiased", [False, True], ids=["reference mode", "antialiased"])
@pytest.mark.parametrize("cam", list(bc.CAMERAS))
def test_the_two_references_chained_are_autograd_of_one_function_from_parameters_to_image(pkg, oracle, cam, antialiased):
    """The blend's sums enter from the binary64 replay of the binary32 walk's decisions: that variant, not the definition's
    binary32 walk, is the exact derivative of the smooth function autograd differentiates (tests/backward_reference.py), and the
    two variants share every line that decides what a sum MEANS -- which is what the seam is about."""
    worst, want = _seam(pkg, oracle, cam, antialiased)
    n = comp.RENDER_SCENE[0]
    assert 4 * want["visible"].sum() >= n
    for name in comp.NAMES:
        assert np.abs(want[name]).max() > 0, name
        print(f"{cam}, {'antialiased' if antialiased else 'reference mode'}: {name}: worst error / bound = {worst[name]:.3g}")
        assert worst[name] <= 1.0, (name, worst[name])
    if cam != "default":
        verts, u, ref, G, ga = _render_frame(pkg, oracle, cam, antialiased)
        V = bc.view_block(u)
        assert np.abs(V - V.T).max() > 0.1 and np.abs(np.asarray(u[0]["camera_position"])[:3]).max() > 0


def _swap_conic(g):
    return dict(g, conic=np.ascontiguousarray(g["conic"][:, ::-1]))


def _swap_uv(g):
    return dict(g, uv=np.ascontiguousarray(g["uv"][:, ::-1]))


@pytest.mark.parametrize("bend", [_swap_conic, _swap_uv], ids=["conic 0 and 2 swapped", "uv swapped"])
@pytest.mark.parametrize("cam", list(bc.CAMERAS))
def test_a_slip_at_the_seam_fails_the_chained_comparison_by_more_than_a_thousand_bounds(pkg, oracle, cam, bend):
    worst, _ = _seam(pkg, oracle, cam, False, bend=bend)
    print(f"{cam}: {bend.__name__}: worst error / bound = " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert max(worst["means"], worst["log_scales"], worst["quats"]) > 1000.0


# ------------------------------------------------------------------------------------------------ 2b. the moved branch scene
def moved_branch_frame(pkg, oracle):
    """The branch scene and the default camera moved together by backward_cameras.BRANCH_MOVE: the vertices through
    tests/transform_reference.py (host, float64, rounded to float32), the camera through transform_camera.  Returns (vertices,
    camera, uniforms, oracle stages)."""
    if "branch" not in _seams:
        w, h = psc.BRANCH_FRAME
        verts = oracle.activate_records(psc.branch_records())
        moved = tref.transform_vertices(verts, **bc.BRANCH_MOVE).astype(np.float32)
        moved = np.ascontiguousarray(moved).view(verts.dtype).reshape(len(verts))
        cam = pkg.transform_camera(bc.camera(pkg, "default"), **bc.BRANCH_MOVE)
        u = oracle.camera_uniforms(cam.view(oracle.CAMERA_DT), w, h)
        _seams["branch"] = (moved, cam, u, oracle.stages(moved, u))
    return _seams["branch"]


def test_the_moved_branch_scene_stands_on_the_intended_side_of_every_branch_by_a_margin(pkg, oracle):
    """The margins of test_the_branch_scene_stands_on_the_intended_side_of_every_branch_by_a_margin under an asymmetric view.
    THE NEEDLE: its two vanishing scales stay exactly 0 and, in this reference's association, its det_raw is still 0.0 (asserted).
    But after the move that is no longer true "in any association", which is what the unmoved scene's docstring claims and what a
    device run needs: the needle's axis is now a rounded rotation of world x, so cov01 and cov11 are products of rounding-sized
    factors, not exact zeros, and det_raw = cov00 cov11 - cov01^2 is a difference of two nearly equal such products whose sign the
    order of the operations decides.  So the needle ALONE is dropped from this scene's device run
    (tests/test_gpu_backward_cameras.py keeps Gaussians 0..6); every other margin is asserted as the unmoved scene's test has it."""
    verts, cam, u, ref = moved_branch_frame(pkg, oracle)
    V = bc.view_block(u)
    assert np.abs(V - V.T).max() > 0.1 and np.abs(np.asarray(u[0]["camera_position"])[:3]).max() > 0.1
    want = pref.backward(*pref.unpack_vertices(verts), u, ref["tiles"] != 0, ref["attr"]["color_radii"][:, 0] > 0, antialiased=True)
    assert want["visible"].all()
    m = want["margin"]["clamp"]
    for g in psc.BRANCH_BEYOND_X:
        assert want["binds"][g, 0] and m[g, 0] > 1.3 and not want["binds"][g, 1] and m[g, 1] < 0.5
    for g in psc.BRANCH_BEYOND_Y:
        assert want["binds"][g, 1] and m[g, 1] > 1.3 and not want["binds"][g, 0] and m[g, 0] < 0.5
    assert not want["binds"][psc.BRANCH_INSIDE_X].any() and (m[psc.BRANCH_INSIDE_X] < 0.5).all()
    assert want["binds"].sum() == 4
    r = ref["attr"]["color_radii"][:, 0]
    assert r[psc.BRANCH_RED_OFF] == 0 and want["margin"]["r"][psc.BRANCH_RED_OFF] < -0.1
    assert r[psc.BRANCH_RED_ON] > 0.5 and want["margin"]["r"][psc.BRANCH_RED_ON] > 0.5
    assert (np.delete(want["det_raw"], psc.BRANCH_NEEDLE) > 1e-3).all()
    print(f"the moved needle's det_raw: {want['det_raw'][psc.BRANCH_NEEDLE]!r}")
    assert want["det_raw"][psc.BRANCH_NEEDLE] == 0.0
    assert psc.BRANCH_NEEDLE == len(verts) - 1               # (dropping it leaves the other Gaussians' ids as they are)


# ------------------------------------------------------------------------------------------------ 2e. descent on geometry
def test_the_geometry_learning_rate_is_the_largest_for_which_the_reference_descent_falls_every_step(pkg, oracle):
    """Six Adam steps on means, log-scales and quaternions under C1: the oracle's forward, the composed reference gradient
    (tests/composed_reference.py, the definition's binary32 walk), torch's Adam on float32 parameters.  The rate the device test
    uses is chosen here, not there."""
    chosen, losses = None, {}
    for lr in comp.GEOMETRY_RATES:
        losses[lr] = comp.reference_descent(pkg, oracle, lr)
        print(f"lr {lr:g}: losses " + " ".join(f"{v:.6g}" for v in losses[lr]))
        if chosen is None and all(b < a for a, b in zip(losses[lr], losses[lr][1:])):
            chosen = lr
    assert chosen == comp.GEOMETRY_LR, (chosen, losses)
    assert len(losses[chosen]) == 7 and losses[chosen][0] > 0
