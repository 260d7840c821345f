"""gs_project_backward / Renderer.project_backward / Renderer.differentiable_render without a GPU.  The yardstick the GPU tests
compare with (tests/project_backward_reference.py) is pinned here: its binary32 p_view[2] is the oracle's depth bit for bit, its
sums are the gradients torch.autograd finds for an independent float64 restatement of the record function F (written below as a
forward function only, branches fixed as the frame took them) within the bound the module derives, and each single-term mutation
of its chain that the default camera can see moves some element by more than a thousand bounds (the four it cannot, and the same
comparisons under moved, rotated cameras: tests/test_backward_cameras_api.py).  Then the entry point's refusals, the structure's layout and the
wrapper's tensor checks."""
import ctypes as C

import numpy as np
import pytest

import project_backward_reference as pref
import project_backward_scenes as psc
import record_function_torch as rft
from helpers import FakeTensor, forbid_c, hand_made_renderer, oracle_frame

SCENES = {"A": (600, 72, 40), "T": (1500, 64, 64)}   # synth_records(n, seed=5, kind): n, width, height; and "branch"
INVALID = -1                                         # GS_ERR_INVALID
_frames = {}


def frame(pkg, oracle, kind):
    """(records, width, height, oracle vertices, uniforms, oracle stages) of a test scene: computed once, never changed."""
    if kind not in _frames:
        if kind == "branch":
            rec, (w, h) = psc.branch_records(), psc.BRANCH_FRAME
        else:
            n, w, h = SCENES[kind]
            rec = pkg.synth.synth_records(n, seed=5, kind=kind)
        verts, u, ref = oracle_frame(oracle, rec, w, h)
        _frames[kind] = (rec, w, h, verts, u, ref)
    return _frames[kind]


def reference(pkg, oracle, kind, antialiased=False, sh16=False, k=15, mutate=None, grads=None):
    rec, w, h, verts, u, ref = frame(pkg, oracle, kind)
    g = psc.random_gradients(len(rec)) if grads is None else grads
    fields = pref.unpack_vertices(verts, sh16=sh16)
    return pref.backward(*fields, u, ref["tiles"] != 0, ref["attr"]["color_radii"][:, 0] > 0, colour=g["colour"], opacity_grad=g["opacity"],
                         conic=g["conic"], uv=g["uv"], antialiased=antialiased, sh_rest_coeffs=k, mutate=mutate)


@pytest.mark.parametrize("kind", ["A", "T", "branch"])
def test_the_binary32_depth_of_the_restatement_is_the_oracles_bit_for_bit(pkg, oracle, kind):
    rec, w, h, verts, u, ref = frame(pkg, oracle, kind)
    pv, ratio, clamped, lim = pref.clamp_branches(pref.unpack_vertices(verts)[0], u[0])
    vis = ref["tiles"] != 0
    assert vis.sum() > 5
    assert np.array_equal(pv[vis, 2].view(np.uint32), ref["attr"]["depth"][vis].view(np.uint32))


def test_the_branch_scene_stands_on_the_intended_side_of_every_branch_by_a_margin(pkg, oracle):
    rec, w, h, verts, u, ref = frame(pkg, oracle, "branch")
    want = reference(pkg, oracle, "branch", antialiased=True)
    assert want["visible"].all()
    m = want["margin"]["clamp"]
    for g in psc.BRANCH_BEYOND_X:
        assert want["binds"][g, 0] and m[g, 0] > 1.3 and not want["binds"][g, 1] and m[g, 1] < 0.5
    for g in psc.BRANCH_BEYOND_Y:
        assert want["binds"][g, 1] and m[g, 1] > 1.3 and not want["binds"][g, 0] and m[g, 0] < 0.5
    assert not want["binds"][psc.BRANCH_INSIDE_X].any() and (m[psc.BRANCH_INSIDE_X] < 0.5).all()
    r = ref["attr"]["color_radii"][:, 0]
    assert r[psc.BRANCH_RED_OFF] == 0 and want["margin"]["r"][psc.BRANCH_RED_OFF] < -0.1
    assert r[psc.BRANCH_RED_ON] > 0.5 and want["margin"]["r"][psc.BRANCH_RED_ON] > 0.5
    assert want["det_raw"][psc.BRANCH_NEEDLE] == 0.0 and (np.delete(want["det_raw"], psc.BRANCH_NEEDLE) > 1e-3).all()
    assert (want["sh_dc"][psc.BRANCH_RED_OFF, 0] == 0) and (want["sh_rest"][psc.BRANCH_RED_OFF, :, 0] == 0).all()
    assert (want["A"]["sh_dc"][psc.BRANCH_RED_OFF, 0] == 0) and (want["sh_dc"][psc.BRANCH_RED_OFF, 1:] != 0).all()
    assert want["opacity_logits"][psc.BRANCH_NEEDLE] == 0 and want["A"]["opacity_logits"][psc.BRANCH_NEEDLE] == 0


# ------------------------------------------------------------------------------------------------ torch.autograd
def _autograd(verts, u, visible, red_flows, g, antialiased, sh16, k):
    """F as a FORWARD function in torch float64 (tests/record_function_torch.py: the visible Gaussians, the frame's branches as
    constants), and sum_x g_x x differentiated by torch.autograd with respect to the six parameter tensors."""
    import torch
    f = rft.forward(verts, u, visible, red_flows, antialiased, sh16)
    idx = f["idx"]
    T = lambda a: torch.tensor(np.asarray(a, np.float64))  # noqa: E731
    loss = ((T(g["conic"][idx]) * f["conic"]).sum() + (T(g["opacity"][idx]) * f["opacity"]).sum() + (T(g["uv"][idx]) * f["uv"]).sum()
            + (T(g["colour"][idx]) * f["rgb"]).sum())
    loss.backward()
    return rft.gradients(f, len(visible), k)


CASES = [("A", False, False, 15), ("A", True, False, 8), ("A", False, True, 3), ("T", False, False, 0), ("T", True, False, 15),
         ("T", True, True, 3), ("branch", False, False, 15), ("branch", True, False, 15), ("branch", True, True, 8), ("A", True, True, 0)]


@pytest.mark.parametrize("kind,antialiased,sh16,k", CASES)
def test_the_sums_are_the_gradients_autograd_finds_for_the_forward_function(pkg, oracle, kind, antialiased, sh16, k):
    rec, w, h, verts, u, ref = frame(pkg, oracle, kind)
    g = psc.random_gradients(len(rec))
    want = reference(pkg, oracle, kind, antialiased, sh16, k)
    got = _autograd(verts, u, ref["tiles"] != 0, ref["attr"]["color_radii"][:, 0] > 0, g, antialiased, sh16, k)
    print(f"counted roundings: {want['k']}")
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


# ------------------------------------------------------------------------------------------------ teeth
TEETH = {"no_direction": ("A", False, "means"), "clamp_is_constant": ("branch", False, "means"),
         "no_tangent_projection": ("A", False, "quats"), "no_comp_cov": ("T", True, "log_scales"),
         "red_always_flows": ("branch", False, "sh_dc"), "s_not_squared": ("A", False, "log_scales")}


@pytest.mark.parametrize("mutation", list(TEETH))
def test_each_single_term_mutation_moves_an_element_by_more_than_a_thousand_bounds(pkg, oracle, mutation):
    kind, antialiased, name = TEETH[mutation]
    want = reference(pkg, oracle, kind, antialiased)
    bent = reference(pkg, oracle, kind, antialiased, mutate=mutation)
    moved = np.abs(bent[name] - want[name]) / np.maximum(pref.bound(want, name), 1e-300)
    print(f"{mutation}: {name} moves by up to {float(moved.max()):.3g} bounds")
    assert moved.max() > 1000.0
    if mutation == "clamp_is_constant":      # only the Gaussians whose clamp binds move
        rows = np.abs(bent[name] - want[name]).reshape(len(want[name]), -1).max(axis=1) > 0
        assert rows[list(psc.BRANCH_BEYOND_X + psc.BRANCH_BEYOND_Y)].all() and not rows[psc.BRANCH_INSIDE_X]
    if mutation == "red_always_flows":
        assert moved[psc.BRANCH_RED_OFF, 0] > 1000.0 and (moved[psc.BRANCH_RED_ON] == 0).all()


# ------------------------------------------------------------------------------------------------ the C entry point
def _refused(pkg, r, g, word):
    L = pkg.binding.lib()
    assert L.gs_project_backward(r, g) == INVALID
    msg = L.gs_last_error()
    assert msg and word in msg, msg


OUT_MEMBERS = ("d_means", "d_log_scales", "d_quats", "d_opacity_logits", "d_sh_dc", "d_sh_rest")
IN_MEMBERS = ("d_colour", "d_opacity", "d_conic", "d_uv")


def test_invalid_arguments_are_refused_without_a_device(pkg):
    PG = pkg.binding.ProjectGrads
    fake = C.c_void_p(8)              # (r is not dereferenced before every member of g has been checked)
    _refused(pkg, None, C.byref(PG()), b"null")
    _refused(pkg, fake, None, b"null")
    _refused(pkg, None, None, b"null")
    for member in IN_MEMBERS + OUT_MEMBERS:
        for offset in (4, 2, 1):
            g = PG(**{m: 8192 for m in IN_MEMBERS + OUT_MEMBERS}, sh_rest_coeffs=15)
            setattr(g, member, 8192 + offset)
            _refused(pkg, fake, C.byref(g), b"aligned")
    for k in (1, 2, 4, 7, 9, 14, 16, 45, 2 ** 31):
        _refused(pkg, fake, C.byref(PG(d_means=8192, d_sh_rest=8192, sh_rest_coeffs=k)), b"sh_rest_coeffs")
        _refused(pkg, fake, C.byref(PG(sh_rest_coeffs=k)), b"sh_rest_coeffs")
    for k in (3, 8, 15):
        _refused(pkg, fake, C.byref(PG(d_means=8192, sh_rest_coeffs=k)), b"d_sh_rest")
    g = PG(d_colour=4096 + 4)         # misaligned with nothing asked for: still refused, by the pointer's value alone
    _refused(pkg, fake, C.byref(g), b"aligned")


def test_the_structure_has_the_headers_layout(pkg):
    PG = pkg.binding.ProjectGrads
    names = list(IN_MEMBERS + OUT_MEMBERS) + ["sh_rest_coeffs"]
    assert [f[0] for f in PG._fields_] == names
    assert C.sizeof(PG) == 88 and [getattr(PG, k).offset for k in names] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 80]
    assert "gs_project_backward" in pkg.binding.SYMBOLS
    assert "gs_project_backward.hip" in pkg.binding.KERNEL_SOURCES
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gs3d_hip.h")).read()
    body = header[header.index("} gs_project_grads;") - 2000:header.index("} gs_project_grads;")]
    body = body[body.rindex("typedef struct"):]
    order = [body.index(" " + m + ";") if m != "sh_rest_coeffs" else body.index("sh_rest_coeffs;") for m in names]
    assert order == sorted(order), "the header declares the members in another order"


# ------------------------------------------------------------------------------------------------ the wrapper
def _Fake(shape, dtype="torch.float64", **how):
    """helpers.FakeTensor, float64 unless told: the dtype of what project_backward takes and adds to."""
    return FakeTensor(shape, dtype, **how)


def test_the_wrapper_checks_its_tensors_before_it_reaches_c(pkg, monkeypatch):
    forbid_c(pkg, monkeypatch)
    rend = hand_made_renderer(pkg, frame_hw=(40, 72))
    f32 = "torch.float32"
    ins = dict(colour=_Fake((100, 3)), opacity=_Fake((100,)), conic=_Fake((100, 3)), uv=_Fake((100, 2)))
    out = dict(means=_Fake((100, 3)), log_scales=_Fake((100, 3)), quats=_Fake((100, 4)), opacity_logits=_Fake((100,)),
               sh_dc=_Fake((100, 3)), sh_rest=_Fake((100, 15, 3)))
    with pytest.raises(AssertionError, match="C library was reached"):   # everything in order: the call goes through to C
        rend.project_backward(**ins, out=dict(out))
    with pytest.raises(AssertionError, match="C library was reached"):
        rend.project_backward(uv=ins["uv"], out=dict(means=out["means"], sh_rest=_Fake((100, 8, 3))))
    bad_in = [("colour", _Fake((100, 3), f32), TypeError), ("colour", _Fake((100, 4)), ValueError), ("colour", _Fake((99, 3)), ValueError),
              ("opacity", _Fake((100, 1)), ValueError), ("opacity", np.zeros(100), TypeError), ("conic", _Fake((100, 2)), ValueError),
              ("conic", _Fake((100, 3), device="cuda:1"), ValueError), ("uv", _Fake((100, 2), contiguous=False), ValueError),
              ("uv", _Fake((100, 2), device="cpu"), ValueError)]
    for name, tensor, error in bad_in:
        with pytest.raises(error, match=name):
            rend.project_backward(**dict(ins, **{name: tensor}), out=dict(out))
    bad_out = [("means", _Fake((100, 3), f32), TypeError), ("means", _Fake((100, 4)), ValueError), ("log_scales", _Fake((99, 3)), ValueError),
               ("quats", _Fake((100, 3)), ValueError), ("opacity_logits", _Fake((100, 1)), ValueError), ("sh_dc", _Fake((100, 1, 3)), ValueError),
               ("sh_rest", _Fake((100, 7, 3)), ValueError), ("sh_rest", _Fake((100, 15, 3), contiguous=False), ValueError),
               ("sh_rest", _Fake((100, 45)), ValueError), ("sh_dc", _Fake((100, 3), device="cpu"), ValueError)]
    for name, tensor, error in bad_out:
        with pytest.raises(error, match=name):
            rend.project_backward(**ins, out=dict(out, **{name: tensor}))
    with pytest.raises(TypeError, match="unknown"):
        rend.project_backward(**ins, out=dict(out, scales=_Fake((100, 3))))
    with pytest.raises(ValueError, match="sh_degree"):
        rend.project_backward(**ins, sh_degree=4)
    with pytest.raises(ValueError, match=r"uv: the tensor is on the CPU; the arrays of Renderer\.project_backward live on the renderer's device"):
        rend.project_backward(uv=_Fake((100, 2), device="cpu"), out=dict(out))
