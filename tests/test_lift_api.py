"""gs_lift_pixels / Renderer.lift_pixels / Renderer.differentiable_feature_maps without a GPU: the yardstick the GPU tests compare
with (tests/lift_reference.py) is pinned to the oracle's image bit for bit, agrees with the two yardsticks it is the sibling of
(contribution_reference's weights, feature_reference's blend, whose transpose it is), and the entry point and its Python
wrappers refuse what they must before anything touches a device."""
import ctypes as C

import numpy as np
import pytest

import contribution_reference as cref
import feature_reference as fref
import lift_reference as lref
from helpers import assert_images_identical, FakeTensor as _Fake, forbid_c, hand_made_renderer, oracle_frame

SCENES = {"A": (600, 72, 40), "T": (1500, 64, 64)}   # synth_records(n, seed=5, kind): n, width, height
INVALID = -1                                         # GS_ERR_INVALID
CHANNELS = 3
U53, U24 = 2.0 ** -53, 2.0 ** -24


def _values(h, w, channels, seed=23):
    return np.random.default_rng(seed).standard_normal((h, w, channels)).astype(np.float32)


def _mask(h, w):
    m = np.zeros((h, w), np.uint8)
    m[5:29, 11:43] = 7                               # aligned to neither tiles nor 8 x 8 blocks; any nonzero value counts
    return m


@pytest.fixture(scope="module", params=sorted(SCENES))
def walked(request, pkg, oracle):
    n, w, h = SCENES[request.param]
    rec = pkg.synth.synth_records(n, seed=5, kind=request.param)
    _, _, ref = oracle_frame(oracle, rec, w, h)
    vals = _values(h, w, CHANNELS)
    return request.param, w, h, ref, vals, lref.lift(oracle, ref, w, h, vals)


def test_the_reference_walks_to_the_oracles_image(walked):
    kind, w, h, ref, vals, got = walked
    assert (ref["image"][..., :3] != 0).any()
    assert_images_identical(got["image"], ref["image"], label=f"lift reference, kind {kind}")


@pytest.mark.parametrize("masked", [False, True], ids=["no mask", "mask"])
def test_the_weights_are_those_of_the_contribution_reference(walked, oracle, masked):
    """weight[g] sums w, the contribution reference sums q = rint(w 2^24): they differ by at most one half per term, plus what
    n_g binary64 adds can lose.  The Gaussians that receive terms are exactly those with pixels > 0, term for term."""
    kind, w, h, ref, vals, whole = walked
    mask = _mask(h, w) if masked else None
    got = lref.lift(oracle, ref, w, h, vals, mask) if masked else whole
    con = cref.contributions(oracle, ref, w, h, mask)
    pixels = con["pixels"].astype(np.int64)
    assert (pixels > 0).sum() > 50
    assert np.array_equal(got["terms"], pixels)
    assert np.array_equal(got["terms"] > 0, got["weight"] > 0)
    scaled = got["weight"] * 2.0 ** 24
    bound = 0.5 * pixels + pixels * U53 * scaled
    assert (np.abs(scaled - con["weight"].astype(np.float64)) <= bound).all()
    assert int(got["blended"].sum()) == cref.contributions(oracle, ref, w, h)["blended"]   # per pixel, counted or not
    if masked:
        assert (got["terms"] <= whole["terms"]).all() and got["terms"].sum() < whole["terms"].sum()
        assert (got["weight"] <= whole["weight"]).all()


def test_the_lift_is_the_transpose_of_the_feature_blend(walked, oracle):
    """<feature_maps(f), v> = <f, lift(v)>.  The forward rounds three times per term in binary32 ((f alpha) T against f w, and the
    add) and adds up to m - 1 more times per pixel; the lift is exact per term and sums in binary64.  Bound: 2 (m_max + 3) 2^-24
    sum |f w v|, m_max the longest blended run at a pixel; the factor 2 covers second-order terms and the binary64 dot products."""
    kind, w, h, ref, vals, got = walked
    n = SCENES[kind][0]
    f = np.random.default_rng(31).standard_normal((n, CHANNELS)).astype(np.float32)
    fwd = fref.feature_maps(oracle, ref, w, h, f)["features"]
    lhs = float((fwd.astype(np.float64) * vals.astype(np.float64)).sum())
    rhs = float((f.astype(np.float64) * got["out"]).sum())
    m_max = int(got["blended"].max())
    scale = float((np.abs(f.astype(np.float64)) * got["A"]).sum())
    assert m_max > 3 and scale > 0
    print(f"kind {kind}: <Bf, v> = {lhs!r}, <f, B'v> = {rhs!r}, difference {abs(lhs - rhs):.3g}, bound {2 * (m_max + 3) * U24 * scale:.3g}")
    assert abs(lhs - rhs) <= 2 * (m_max + 3) * U24 * scale


def test_the_channel_less_reference_has_the_same_weights(walked, oracle):
    kind, w, h, ref, vals, got = walked
    bare = lref.lift(oracle, ref, w, h)
    assert bare["out"].shape == (SCENES[kind][0], 0)
    for k in ("weight", "terms", "blended"):
        assert np.array_equal(bare[k], got[k]), k


# ------------------------------------------------------------------------------------------------ the C entry point
def _refused(pkg, r, l, word):
    L = pkg.binding.lib()
    assert L.gs_lift_pixels(r, l) == INVALID
    msg = L.gs_last_error()
    assert msg and word in msg, msg


def test_invalid_arguments_are_refused_without_a_device(pkg):
    PL = pkg.binding.PixelLift
    fake = C.c_void_p(8)              # (r is not dereferenced before every member of l has been checked)
    _refused(pkg, None, C.byref(PL()), b"null")
    _refused(pkg, fake, None, b"null")
    _refused(pkg, None, None, b"null")
    _refused(pkg, fake, C.byref(PL(values=4096, channels=257, out=8192)), b"channels")
    _refused(pkg, fake, C.byref(PL(values=None, channels=3, out=8192)), b"values")
    _refused(pkg, fake, C.byref(PL(values=4096, channels=3, out=None, out_weight=8192)), b"out")
    for member, offset in (("values", 2), ("out", 4), ("out_weight", 4), ("out", 1), ("out_weight", 2)):
        l = PL(values=4096, channels=3, out=8192)
        setattr(l, member, 8192 + offset)
        _refused(pkg, fake, C.byref(l), b"aligned")
        l = PL(channels=0)
        setattr(l, member, 4096 + offset)
        _refused(pkg, fake, C.byref(l), b"aligned")


def test_the_structure_has_the_headers_layout(pkg):
    PL = pkg.binding.PixelLift
    assert [f[0] for f in PL._fields_] == ["values", "channels", "mask", "out", "out_weight"]
    assert C.sizeof(PL) == 40
    assert (PL.values.offset, PL.channels.offset, PL.mask.offset, PL.out.offset, PL.out_weight.offset) == (0, 8, 16, 24, 32)
    assert "gs_lift_pixels" in pkg.binding.SYMBOLS
    assert "gs_lift.hip" in pkg.binding.KERNEL_SOURCES
    assert pkg.binding.LIFT_CHANNELS_MAX == 256


# ------------------------------------------------------------------------------------------------ the wrapper
def test_the_wrapper_checks_its_tensors_before_it_reaches_c(pkg, monkeypatch):
    forbid_c(pkg, monkeypatch)
    rend = hand_made_renderer(pkg, frame_hw=(40, 72))
    f64 = "torch.float64"
    good = dict(values=_Fake((40, 72, 5)), out=_Fake((100, 5), f64), weight=_Fake((100,), f64), mask=_Fake((40, 72), "torch.uint8"))
    with pytest.raises(AssertionError, match="C library was reached"):   # everything in order: the call goes through to C
        rend.lift_pixels(**good)
    with pytest.raises(AssertionError, match="C library was reached"):
        rend.lift_pixels(None, weight=_Fake((100,), f64))
    with pytest.raises(AssertionError, match="C library was reached"):
        rend.lift_pixels(good["values"], out=good["out"], mask=_Fake((40, 72), "torch.bool"))
    bad = [("values", _Fake((40, 72, 5), f64), TypeError), ("out", _Fake((100, 5)), TypeError),
           ("weight", _Fake((100,), "torch.int64"), TypeError), ("mask", _Fake((40, 72), "torch.float32"), TypeError),
           ("out", np.zeros((100, 5), np.float64), TypeError),
           ("values", _Fake((72, 40, 5)), ValueError), ("values", _Fake((40, 72)), ValueError),
           ("values", _Fake((40, 72, 257)), ValueError),
           ("out", _Fake((100, 4), f64), ValueError),                    # a channel mismatch between values and out
           ("out", _Fake((99, 5), f64), ValueError), ("out", _Fake((5, 100), f64), ValueError), ("out", _Fake((100,), f64), ValueError),
           ("weight", _Fake((99,), f64), ValueError), ("weight", _Fake((100, 1), f64), ValueError),
           ("mask", _Fake((72, 40), "torch.uint8"), ValueError), ("mask", _Fake((40, 72, 1), "torch.uint8"), ValueError),
           ("values", _Fake((40, 72, 5), contiguous=False), ValueError), ("out", _Fake((100, 5), f64, contiguous=False), ValueError),
           ("mask", _Fake((40, 72), "torch.uint8", contiguous=False), ValueError),
           ("values", _Fake((40, 72, 5), device="cpu"), ValueError), ("weight", _Fake((100,), f64, device="cpu"), ValueError),
           ("out", _Fake((100, 5), f64, device="cuda:1"), ValueError)]
    for name, tensor, error in bad:
        with pytest.raises(error, match=name):
            rend.lift_pixels(**dict(good, **{name: tensor}))
    with pytest.raises(ValueError, match=r"weight: the tensor is on the CPU; the arrays of Renderer\.lift_pixels live on the renderer's device"):
        rend.lift_pixels(None, weight=_Fake((100,), f64, device="cpu"))
    with pytest.raises(ValueError, match="out"):                         # values without an output for them, and the reverse
        rend.lift_pixels(good["values"], weight=good["weight"])
    with pytest.raises(ValueError, match="out"):
        rend.lift_pixels(None, out=good["out"])


# ------------------------------------------------------------------------------------------------ the autograd function
def _dense_renderer(pkg, monkeypatch, n=7, h=3, w=4):
    """A Renderer whose frame is a small dense matrix B (h w x n): feature_maps is B f, lift_pixels is B' v in float64, and
    render reaches a C library that does nothing.  CPU tensors throughout."""
    import torch
    B = torch.tensor(np.random.default_rng(3).random((h * w, n)), dtype=torch.float32)
    calls = []

    class Lib:
        def gs_render(self, *args):
            return 0
    monkeypatch.setattr(pkg.binding, "lib", lambda: Lib())
    rend = object.__new__(pkg.Renderer)
    rend.scene, rend._h, rend._frame_hw, rend._frames = None, None, (h, w), 0

    def feature_maps(features=None, out=None, **kw):
        assert out is True and not features.requires_grad and features.is_contiguous()
        calls.append("feature_maps")
        return dict(out=(B @ features).reshape(h, w, -1))

    def lift_pixels(values, out=None, weight=None, mask=None):
        assert out is True and weight is None and mask is None
        assert values.dtype == torch.float32 and values.is_contiguous() and tuple(values.shape[:2]) == (h, w)
        calls.append("lift_pixels")
        return dict(out=B.double().T @ values.reshape(h * w, -1).double())
    monkeypatch.setattr(rend, "feature_maps", feature_maps, raising=False)
    monkeypatch.setattr(rend, "lift_pixels", lift_pixels, raising=False)
    return rend, B, calls


def test_the_gradient_of_feature_maps_is_the_lift_of_the_incoming_gradient(pkg, monkeypatch):
    import torch
    rend, B, calls = _dense_renderer(pkg, monkeypatch)
    n, c = B.shape[1], 5
    f = torch.tensor(np.random.default_rng(4).standard_normal((n, c)), dtype=torch.float32, requires_grad=True)
    v = torch.tensor(np.random.default_rng(5).standard_normal((3, 4, c)), dtype=torch.float32)
    rend.render(np.zeros(1, pkg.binding.UNIFORMS_DT))
    out = rend.differentiable_feature_maps(f)
    assert out.shape == (3, 4, c) and out.requires_grad
    assert torch.equal(out.detach(), (B @ f.detach()).reshape(3, 4, c))
    (grad,) = torch.autograd.grad((out * v).sum(), f)
    assert calls == ["feature_maps", "lift_pixels"]
    assert grad.dtype == torch.float32 and grad.shape == (n, c)
    want = (B.double().T @ v.reshape(12, c).double()).float()
    assert torch.equal(grad, want)
    # a non-contiguous incoming gradient, in float64 graphs too, reaches lift_pixels as contiguous float32
    out = rend.differentiable_feature_maps(f)
    (grad,) = torch.autograd.grad((out.permute(1, 0, 2) * v.permute(1, 0, 2)).sum(), f)
    assert torch.equal(grad, want)


def test_a_backward_after_another_frame_raises(pkg, monkeypatch):
    import torch
    rend, B, calls = _dense_renderer(pkg, monkeypatch)
    f = torch.ones((B.shape[1], 2), dtype=torch.float32, requires_grad=True)
    u = np.zeros(1, pkg.binding.UNIFORMS_DT)
    rend.render(u)
    out = rend.differentiable_feature_maps(f)
    rend.render(u)                                   # another frame: the lists the forward walked are gone
    with pytest.raises(RuntimeError, match="frame"):
        out.sum().backward()
    assert calls == ["feature_maps"] and f.grad is None
    out = rend.differentiable_feature_maps(f)        # forward again on the new frame: the backward goes through
    out.sum().backward()
    assert f.grad is not None and f.grad.shape == f.shape
