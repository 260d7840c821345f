"""gs_photometric_loss / Renderer.photometric_loss without a GPU.  The yardstick the GPU tests compare with
(tests/photometric_loss_reference.py) is pinned here: its gradient and terms are what torch.autograd finds for an independent
float64 restatement written the way the trainers write it (tests/photometric_loss_torch.py), within the bound the module derives,
on every image of tests/photometric_loss_images.py and lambda in 0, 0.2, 1; it lies within a QUARTER of that bound of the same
formulas in binary80, so the yardstick itself is inside the contract; and each single-term mutation of it misses the bound by
more than ten times on some listed image.  Then the entry point's refusals, the structure's layout and the wrapper's checks."""
import ctypes as C
import os

import numpy as np
import pytest

import photometric_loss_images as pli
import photometric_loss_reference as plr
import photometric_loss_torch as plt_

INVALID = -1
LAMBDAS = (0.0, 0.2, 1.0)
_cache = {}


def reference(name, lam, mutate=None, dtype=np.float64):
    key = (name, lam, mutate, dtype)
    if key not in _cache:
        _cache[key] = plr.evaluate(*pli.images(name), lam, dtype=dtype, mutate=mutate)
    return _cache[key]


def limit(name, lam):
    key = ("bound", name, lam)
    if key not in _cache:
        _cache[key] = plr.bound(*pli.images(name), lam)
    return _cache[key]


def _ratios(got_grad, got_terms, name, lam, which="grad64"):
    """(worst |got - want| / bound over the gradient, the same per term).  which: "grad64" for a binary64 evaluation, "grad" for the
    device's bound, which holds the rounding to binary32.  A NaN term (ssim at lambda = 0) must be NaN on both sides; a term whose
    bound is 0 (l1 of equal images) allows no error at all: an error there counts as infinitely many bounds."""
    want, lim = reference(name, lam), limit(name, lam)
    assert np.isfinite(lim[which]).all() and (lim[which] > 0).all(), name
    g = float((np.abs(np.asarray(got_grad, np.float64) - want["grad"]) / lim[which]).max())
    t = []
    for k in range(4):
        if np.isnan(want["terms"][k]):
            assert lam == 0 and k == 2 and np.isnan(got_terms[k])
            t.append(0.0)
        else:
            err = abs(float(got_terms[k]) - float(want["terms"][k]))
            t.append(0.0 if err == 0 else (float("inf") if lim["terms"][k] == 0 else float(err / lim["terms"][k])))
    return g, t


# ------------------------------------------------------------------------------------------------ 1. autograd
@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("name", pli.NAMES)
def test_the_reference_is_what_autograd_finds_for_the_trainers_own_formulation(name, lam):
    terms, grad = plt_.loss_and_gradient(*pli.images(name), lam)
    g, t = _ratios(grad, terms, name, lam)
    print(f"{name}, lambda {lam}: gradient error / bound {g:.3g}; terms {['%.3g' % v for v in t]}; "
          f"largest bound / largest |gradient| {float(limit(name, lam)['grad64'].max() / max(np.abs(reference(name, lam)['grad']).max(), 1e-300)):.3g}")
    assert g <= 1.0 and max(t) <= 1.0


# ------------------------------------------------------------------------------------------------ 2. the yardstick is inside the contract
@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("name", pli.NAMES)
def test_the_reference_lies_within_a_quarter_of_the_bound_of_binary80(name, lam):
    assert np.finfo(np.longdouble).nmant >= 63, "this host's long double is no wider than binary64"
    exact = reference(name, lam, dtype=np.longdouble)
    want, lim = reference(name, lam), limit(name, lam)
    own = lim["grad64"]    # (the bound without the device's rounding to binary32, which the yardstick does not make)
    if lam == 0:    # the contract there is exact -- grad = fl(sign(x - y) / n), one correctly rounded division -- and so is the yardstick
        assert np.array_equal(want["grad"], exact["grad"].astype(np.float64))
        g = 0.0
    else:
        g = float((np.abs(want["grad"] - exact["grad"]).astype(np.float64) / own).max())
    t = [0.0 if np.isnan(want["terms"][k]) or want["terms"][k] == exact["terms"][k] else float(abs(want["terms"][k] - exact["terms"][k]) / lim["terms"][k])
         for k in range(4)]
    print(f"{name}, lambda {lam}: gradient {g:.3g}, terms {['%.3g' % v for v in t]} of the bound")
    assert (own > 0).all() and g <= 0.25 and max(t) <= 0.25


# ------------------------------------------------------------------------------------------------ 3. mutations
@pytest.mark.parametrize("mutation", plr.MUTATIONS)
def test_each_mutation_of_the_reference_misses_the_bound_by_ten_times_on_some_image(mutation):
    worst, where = 0.0, None
    for name in pli.NAMES:
        for lam in LAMBDAS:
            m = reference(name, lam, mutate=mutation)
            g, t = _ratios(m["grad"], m["terms"], name, lam, which="grad")     # (the device's bound, the wider one)
            if max([g] + t) > worst:
                worst, where = max([g] + t), (name, lam)
    print(f"{mutation}: worst error / bound = {worst:.3g} on {where}")
    assert worst >= 10.0, (mutation, worst)


def test_the_mutations_are_the_eight_the_contract_names():
    assert set(plr.MUTATIONS) == {"drop_P2", "drop_P3", "replicate_padding", "window_not_normalised", "sign0_is_1", "swap_C1_C2",
                                  "mean_over_HW", "sigma_1"}
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gs3d_hip.h")).read()
    assert f"K_CONV = {plr.K_CONV} per" in header
    g = plr.window()
    assert g.dtype == np.float64 and abs(g.sum() - 1) < 4e-16 and np.array_equal(g, g[::-1])
    assert [v.hex() for v in g[:6]] == ["0x1.0d956b52a1d6fp-10", "0x1.f1fe01ae5a5b7p-8", "0x1.26eb175d83f66p-5", "0x1.bff0fe8e98418p-4",
                                        "0x1.b43c3f52b19f2p-3", "0x1.106560aa892c0p-2"]       # gs_loss.hip's constants


# ------------------------------------------------------------------------------------------------ 4. the C entry point
MEMBERS = ("image", "target", "width", "height", "image_stride", "target_stride", "lambda_dssim", "terms", "grad_rgb")


def _refused(pkg, rc, word):
    assert rc == INVALID
    msg = pkg.binding.lib().gs_last_error()
    assert msg and word in msg, msg


def _good(pkg, **over):
    return pkg.binding.PhotoLoss(**dict(dict(image=8192, target=8192, width=64, height=48, image_stride=3, target_stride=4, lambda_dssim=0.2,
                                             terms=8192, grad_rgb=8192), **over))


def test_invalid_arguments_are_refused_without_a_device(pkg):
    L = pkg.binding.lib()
    fake = C.c_void_p(8)              # (r is not dereferenced before every member of l has been checked)
    _refused(pkg, L.gs_photometric_loss(None, C.byref(_good(pkg))), b"null")
    _refused(pkg, L.gs_photometric_loss(fake, None), b"null")
    _refused(pkg, L.gs_photometric_loss(None, None), b"null")
    for outs in (dict(terms=None), dict(grad_rgb=None), dict()):
        _refused(pkg, L.gs_photometric_loss(fake, C.byref(_good(pkg, image=None, **outs))), b"image")
        _refused(pkg, L.gs_photometric_loss(fake, C.byref(_good(pkg, target=None, **outs))), b"target")
    for extent in (0, -1, 16385, 2 ** 31 - 1):
        _refused(pkg, L.gs_photometric_loss(fake, C.byref(_good(pkg, width=extent))), b"width")
        _refused(pkg, L.gs_photometric_loss(fake, C.byref(_good(pkg, height=extent))), b"height")
    for stride in (0, 1, 2, 5, -3):
        _refused(pkg, L.gs_photometric_loss(fake, C.byref(_good(pkg, image_stride=stride))), b"image_stride")
        _refused(pkg, L.gs_photometric_loss(fake, C.byref(_good(pkg, target_stride=stride))), b"target_stride")
    for lam in (-1e-300, 1.0000000000000002, float("nan"), float("inf"), -float("inf")):
        _refused(pkg, L.gs_photometric_loss(fake, C.byref(_good(pkg, lambda_dssim=lam))), b"lambda_dssim")
    for member in ("image", "target", "grad_rgb"):
        for offset in (2, 1, 3):
            _refused(pkg, L.gs_photometric_loss(fake, C.byref(_good(pkg, **{member: 8192 + offset}))), b"aligned")
    for offset in (4, 2, 1):
        _refused(pkg, L.gs_photometric_loss(fake, C.byref(_good(pkg, terms=8192 + offset))), b"terms must be 8-byte aligned")
    # nothing asked for: the members are still checked ...
    _refused(pkg, L.gs_photometric_loss(fake, C.byref(_good(pkg, terms=None, grad_rgb=None, width=0))), b"width")
    # ... and a call that passes them is done, without a device and without reading r
    assert L.gs_photometric_loss(fake, C.byref(_good(pkg, terms=None, grad_rgb=None))) == 0
    assert L.gs_photometric_loss(fake, C.byref(_good(pkg, terms=None, grad_rgb=None, image=None, target=None))) == 0


def test_the_structure_has_the_headers_layout(pkg):
    PL = pkg.binding.PhotoLoss
    assert [f[0] for f in PL._fields_] == list(MEMBERS)
    assert C.sizeof(PL) == 56 and [getattr(PL, k).offset for k in MEMBERS] == [0, 8, 16, 20, 24, 28, 32, 40, 48]
    assert "gs_photometric_loss" in pkg.binding.SYMBOLS and "gs_loss.hip" in pkg.binding.KERNEL_SOURCES
    assert hasattr(pkg, "PhotoLoss") and hasattr(pkg.Renderer, "photometric_loss") and hasattr(pkg.Renderer, "differentiable_photometric_loss")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gs3d_hip.h")).read()
    body = header[:header.index("} gs_photo_loss;")]
    body = body[body.rindex("typedef struct"):]
    order = [min(body.index(sep + m + end) for sep in (" ", "*") for end in (";", ",") if sep + m + end in body) for m in MEMBERS]
    assert order == sorted(order), "the header declares the members in another order"
    assert f"#define GS_PHOTO_LOSS_MAX_EXTENT {pkg.binding.PHOTO_LOSS_MAX_EXTENT}" in header
    assert "int gs_photometric_loss(gs_renderer* r, const gs_photo_loss* l);" in header


def test_the_wrapper_checks_its_tensors_before_it_reaches_c(pkg, monkeypatch):
    from test_project_backward_api import _Fake

    class NoC:
        def __getattr__(self, name):
            raise AssertionError("the C library was reached")
    monkeypatch.setattr(pkg.binding, "lib", lambda: NoC())

    class SceneStub:
        num_vertices, device = 100, 0
    rend = object.__new__(pkg.Renderer)
    rend.scene, rend._h, rend._frame_hw, rend._frames = SceneStub(), None, None, 0      # (no frame rendered: the loss needs none)
    f32 = "torch.float32"
    img, tgt = _Fake((40, 72, 4), f32), _Fake((40, 72, 3), f32)
    grad, terms = _Fake((40, 72, 3), f32), _Fake((4,))
    for kw in (dict(grad=grad, terms=terms), dict(grad=None, terms=terms), dict(grad=grad, terms=None), dict(grad=None, terms=None)):
        with pytest.raises(AssertionError, match="C library was reached"):   # everything in order: the call goes through to C
            rend.photometric_loss(img, tgt, 0.2, **kw)
    bad = [("image", dict(image=_Fake((40, 72, 3), "torch.float64")), TypeError), ("image", dict(image=_Fake((40, 72, 2), f32)), ValueError),
           ("image", dict(image=_Fake((40, 72), f32)), ValueError), ("image", dict(image=_Fake((0, 72, 3), f32)), ValueError),
           ("image", dict(image=_Fake((40, 16385, 3), f32)), ValueError), ("image", dict(image=_Fake((40, 72, 3), f32, contiguous=False)), ValueError),
           ("image", dict(image=_Fake((40, 72, 3), f32, device="cpu")), ValueError), ("target", dict(target=_Fake((40, 71, 3), f32)), ValueError),
           ("target", dict(target=_Fake((40, 72, 5), f32)), ValueError), ("target", dict(target=_Fake((40, 72, 3), "torch.float16")), TypeError),
           ("target", dict(target=_Fake((40, 72, 3), f32, device="cuda:1")), ValueError), ("grad", dict(grad=_Fake((40, 72, 4), f32)), ValueError),
           ("grad", dict(grad=_Fake((40, 72, 3))), TypeError), ("terms", dict(terms=_Fake((3,))), ValueError),
           ("terms", dict(terms=_Fake((4,), f32)), TypeError), ("terms", dict(terms=_Fake((4,), contiguous=False)), ValueError),
           ("lambda_dssim", dict(lambda_dssim=1.5), ValueError), ("lambda_dssim", dict(lambda_dssim=float("nan")), ValueError)]
    for name, change, error in bad:
        with pytest.raises(error, match=name):
            rend.photometric_loss(**dict(dict(image=img, target=tgt, lambda_dssim=0.2, grad=grad, terms=terms), **change))
