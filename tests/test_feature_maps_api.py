"""gs_blend_features / Renderer.feature_maps without a GPU: the yardstick the GPU tests compare with (tests/feature_reference.py)
is pinned to the oracle's image bit for bit, its outputs keep the invariants the definition implies, and the entry point and its
Python wrapper refuse what they must before anything touches a device."""
import ctypes as C

import numpy as np
import pytest

import feature_reference as fref
from helpers import assert_images_identical, FakeTensor as _Fake, forbid_c, hand_made_renderer, oracle_frame

SCENES = {"A": (600, 72, 40), "T": (1500, 64, 64)}   # synth_records(n, seed=5, kind): n, width, height
INVALID = -1                                         # GS_ERR_INVALID


@pytest.fixture(scope="module", params=sorted(SCENES))
def walked(request, pkg, oracle):
    n, w, h = SCENES[request.param]
    rec = pkg.synth.synth_records(n, seed=5, kind=request.param)
    _, _, ref = oracle_frame(oracle, rec, w, h)
    colours = np.ascontiguousarray(ref["attr"]["color_radii"][:, :3])
    return request.param, w, h, ref, fref.feature_maps(oracle, ref, w, h, colours)


def test_with_the_records_colours_the_reference_blends_the_oracles_image(walked):
    kind, w, h, ref, got = walked
    assert got["features"].shape == (h, w, 3) and (ref["image"][..., :3] != 0).any()
    assert_images_identical(got["features"], ref["image"][..., :3], label=f"feature reference, kind {kind}")


def test_the_reference_keeps_the_invariants_of_the_definition(walked):
    kind, w, h, ref, got = walked
    T, alpha, median, depth = got["T"], got["alpha"], got["median"], got["depth"]
    assert np.array_equal(alpha.view(np.uint32), (np.float32(1.0) - T).view(np.uint32))
    assert ((T > 0) & (T <= 1)).all()
    # while T >= 0.5 the break of :83 cannot fire, so the median is set exactly where the walk ends below one half
    assert np.array_equal(np.isfinite(median), T < np.float32(0.5))
    assert np.isfinite(median).sum() > w * h // 20 and (~np.isfinite(median)).sum() > w * h // 20
    assert (median[~np.isfinite(median)] == np.inf).all()
    b = ref["boundaries"].astype(np.int64)
    tx = (w + 15) // 16
    for y, x in np.argwhere(np.isfinite(median)):
        t = (y // 16) * tx + x // 16
        ids = ref["sorted_payload"][b[2 * t]:b[2 * t + 1]]
        assert median[y, x].view(np.uint32) in ref["attr"]["depth"][ids].view(np.uint32), (x, y)
    # a pixel that blended nothing: all four outputs at their start values; depth > 0 exactly where something was blended
    nothing = T == 1
    assert (depth[nothing] == 0).all() and (alpha[nothing] == 0).all() and (got["features"][nothing] == 0).all()
    assert (depth[~nothing] > 0).all()
    # the expected depth is a sub-convex combination of the list's depths: depth / alpha lies within their range (to rounding)
    vis = ref["tiles"] != 0
    lo, hi = ref["attr"]["depth"][vis].min(), ref["attr"]["depth"][vis].max()
    norm = depth[~nothing].astype(np.float64) / alpha[~nothing]
    assert (norm > lo * (1 - 1e-4)).all() and (norm < hi * (1 + 1e-4)).all()


def test_an_empty_list_gives_zero_zero_zero_and_infinity(walked, oracle):
    kind, w, h, ref, got = walked
    tx = (w + 15) // 16
    emptied = dict(ref, boundaries=ref["boundaries"].copy())
    for t in (1, tx + 2):             # two tiles' lists cut to nothing; every other list stays
        emptied["boundaries"][2 * t + 1] = emptied["boundaries"][2 * t]
    colours = np.ascontiguousarray(ref["attr"]["color_radii"][:, :3])
    cut = fref.feature_maps(oracle, emptied, w, h, colours)
    rest = np.ones((h, w), bool)
    for t in (1, tx + 2):
        ys, xs = slice(16 * (t // tx), 16 * (t // tx) + 16), slice(16 * (t % tx), 16 * (t % tx) + 16)
        assert got["alpha"][ys, xs].max() > 0
        assert (cut["features"][ys, xs] == 0).all() and (cut["alpha"][ys, xs] == 0).all() and (cut["depth"][ys, xs] == 0).all()
        assert (cut["median"][ys, xs] == np.inf).all() and (cut["T"][ys, xs] == 1).all()
        rest[ys, xs] = False
    for k in ("features", "alpha", "depth", "median"):
        assert np.array_equal(cut[k][rest].view(np.uint32), got[k][rest].view(np.uint32)), k


def test_the_channel_less_reference_has_the_same_alpha_and_depths(walked, oracle):
    kind, w, h, ref, got = walked
    bare = fref.feature_maps(oracle, ref, w, h)
    assert bare["features"].shape == (h, w, 0)
    for k in ("alpha", "depth", "median", "T"):
        assert np.array_equal(bare[k].view(np.uint32), got[k].view(np.uint32)), k


# ------------------------------------------------------------------------------------------------ the C entry point
def _refused(pkg, r, m, word):
    L = pkg.binding.lib()
    assert L.gs_blend_features(r, m) == INVALID
    msg = L.gs_last_error()
    assert msg and word in msg, msg


def test_invalid_arguments_are_refused_without_a_device(pkg):
    FM = pkg.binding.FeatureMaps
    fake = C.c_void_p(8)              # (r is not dereferenced before every member of m has been checked)
    _refused(pkg, None, C.byref(FM()), b"null")
    _refused(pkg, fake, None, b"null")
    _refused(pkg, None, None, b"null")
    _refused(pkg, fake, C.byref(FM(features=4096, channels=257, out_features=8192)), b"channels")
    _refused(pkg, fake, C.byref(FM(features=None, channels=3, out_features=8192)), b"features")
    _refused(pkg, fake, C.byref(FM(features=4096, channels=3, out_features=None, out_alpha=8192)), b"out_features")
    for member in ("features", "out_features", "out_alpha", "out_depth", "out_depth_median"):
        m = FM(features=4096, channels=3, out_features=8192)
        setattr(m, member, 2)
        _refused(pkg, fake, C.byref(m), b"aligned")
        m = FM(channels=0)
        setattr(m, member, 4096 + 2)
        _refused(pkg, fake, C.byref(m), b"aligned")


def test_the_structure_has_the_headers_layout(pkg):
    FM = pkg.binding.FeatureMaps
    assert [f[0] for f in FM._fields_] == ["features", "channels", "out_features", "out_alpha", "out_depth", "out_depth_median"]
    assert C.sizeof(FM) == 48 and FM.out_features.offset == 16 and FM.channels.offset == 8
    assert "gs_blend_features" in pkg.binding.SYMBOLS


# ------------------------------------------------------------------------------------------------ the wrapper
def test_the_wrapper_checks_its_tensors_before_it_reaches_c(pkg, monkeypatch):
    forbid_c(pkg, monkeypatch)
    rend = hand_made_renderer(pkg, frame_hw=(40, 72))
    good = dict(features=_Fake((100, 5)), out=_Fake((40, 72, 5)), alpha=_Fake((40, 72)), depth=_Fake((40, 72)),
                median_depth=_Fake((40, 72)))
    with pytest.raises(AssertionError, match="C library was reached"):   # everything in order: the call goes through to C
        rend.feature_maps(**good)
    with pytest.raises(AssertionError, match="C library was reached"):
        rend.feature_maps(alpha=_Fake((40, 72)))
    bad = [("features", _Fake((100, 5), "torch.float64"), TypeError), ("out", _Fake((40, 72, 5), "torch.float16"), TypeError),
           ("alpha", _Fake((40, 72), "torch.int32"), TypeError), ("depth", np.zeros((40, 72), np.float32), TypeError),
           ("features", _Fake((99, 5)), ValueError), ("features", _Fake((100,)), ValueError),
           ("features", _Fake((100, 257)), ValueError),
           ("out", _Fake((40, 72, 4)), ValueError),                      # a channel mismatch between features and out
           ("out", _Fake((72, 40, 5)), ValueError), ("out", _Fake((40, 72)), ValueError),
           ("alpha", _Fake((72, 40)), ValueError), ("alpha", _Fake((40, 72, 1)), ValueError),
           ("depth", _Fake((40, 73)), ValueError), ("median_depth", _Fake((40 * 72,)), ValueError),
           ("out", _Fake((40, 72, 5), contiguous=False), ValueError), ("features", _Fake((100, 5), contiguous=False), ValueError),
           ("median_depth", _Fake((40, 72), contiguous=False), ValueError),
           ("alpha", _Fake((40, 72), device="cpu"), ValueError), ("features", _Fake((100, 5), device="cpu"), ValueError),
           ("depth", _Fake((40, 72), device="cuda:1"), ValueError)]
    for name, tensor, error in bad:
        with pytest.raises(error, match=name):
            rend.feature_maps(**dict(good, **{name: tensor}))
    with pytest.raises(ValueError, match=r"alpha: the tensor is on the CPU; the arrays of Renderer\.feature_maps live on the renderer's device"):
        rend.feature_maps(alpha=_Fake((40, 72), device="cpu"))
    with pytest.raises(ValueError, match="out"):                         # features without an output for them, and the reverse
        rend.feature_maps(features=_Fake((100, 5)), alpha=_Fake((40, 72)))
    with pytest.raises(ValueError, match="out"):
        rend.feature_maps(out=_Fake((40, 72, 5)))
