"""CPU checks of the antialiased mode (gs_set_antialiased): the C ABI exports it and refuses a null renderer, the binding has it,
and the float64 factor the GPU tests compare against (aa_reference.comp64) is what the formula says on cases with a closed form."""
import ctypes

import numpy as np

import aa_reference as aa
import np_reference as npr

GS_ERR_INVALID = -1


def test_library_exports_the_antialiased_setters(pkg):
    L = pkg.binding.lib()
    for name in ("gs_set_antialiased", "gs_get_antialiased", "gs_debug_alpha_cut_scan"):
        assert hasattr(L, name), name
        assert name in pkg.binding.SYMBOLS


def test_null_renderer_is_refused_with_a_message(pkg):
    L = pkg.binding.lib()
    L.gs_set_antialiased.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.gs_get_antialiased.argtypes = [ctypes.c_void_p]
    assert L.gs_set_antialiased(None, 1) == GS_ERR_INVALID
    assert b"null" in L.gs_last_error()
    assert L.gs_set_antialiased(None, 0) == GS_ERR_INVALID
    assert L.gs_get_antialiased(None) == GS_ERR_INVALID
    assert b"null" in L.gs_last_error()


def test_binding_has_the_setter_and_the_property(pkg):
    assert callable(getattr(pkg.Renderer, "set_antialiased", None))
    assert isinstance(pkg.Renderer.__dict__.get("antialiased"), property)
    assert callable(getattr(pkg, "debug_alpha_cut_scan", None))


def _one_gaussian(scale, rot=(1.0, 0.0, 0.0, 0.0), z=-5.0):
    return dict(pos=np.array([[0.0, 0.0, z]]), scale=np.array([scale], float), opacity=np.array([0.8]),
                rot=np.array([rot], float), sh=np.zeros((1, 16, 3)))


def test_comp64_on_isotropic_splats_is_s_over_s_plus_dilation():
    """A sphere on the optical axis projects to an isotropic 2D Gaussian of variance s = (f sigma / z)^2 per axis (f_x = f_y: the
    reference derives tan_fovy from the aspect ratio), so comp = sqrt(s^2 / (s + 0.3)^2) = s / (s + 0.3)."""
    W, H = 640, 360
    cam = npr.camera((0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0), 45.0, 0.1, 1000.0, W, H)
    f = W / (2 * cam["tan_fovx"])
    assert abs(H / (2 * cam["tan_fovy"]) - f) <= 1e-9 * f
    for sigma in (1e-4, 1e-3, 3e-3, 1e-2, 0.1, 1.0):
        pre = npr.preprocess(_one_gaussian([sigma] * 3), cam)
        s = (f * sigma / 5.0) ** 2
        got = aa.comp64(pre)[0]
        assert abs(got - s / (s + 0.3)) <= 1e-12, (sigma, got, s / (s + 0.3))
        assert 0.0 < got < 1.0
        assert aa.comp64(pre, sqrt=False)[0] == got * got or abs(aa.comp64(pre, sqrt=False)[0] / (got * got) - 1) <= 1e-12
        assert aa.comp64(pre, raw_from_dilated=True)[0] == 1.0


def test_comp64_of_a_degenerate_covariance_is_zero():
    """A splat flat in the two directions the camera sees (a needle along the view axis has a point as its footprint, a disc seen
    edge-on a segment): det(cov2D) = 0, comp = 0 -- the splat keeps its lists and never contributes."""
    W, H = 640, 360
    cam = npr.camera((0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0), 45.0, 0.1, 1000.0, W, H)
    for scale in ([0.05, 0.0, 0.0], [0.0, 0.05, 0.0], [0.0, 0.0, 0.3]):
        pre = npr.preprocess(_one_gaussian(scale), cam)
        assert pre["tiles"][0] > 0  # still in the lists: the dilation keeps det > 0
        assert aa.comp64(pre)[0] == 0.0


def test_tolerance_separates_the_mutations_on_a_sub_pixel_scene(pkg):
    """The bound of aa_reference.comp_tolerance is tight enough that the three mutations the GPU test rejects (a dilation of 0.31,
    no square root, det(cov2D) from the dilated matrix) are outside it for most splats of a sub-pixel scene, while the float64
    factor itself, rounded to binary32, is inside it for every one."""
    rec = pkg.synth.synth_records(3000, seed=5, kind="A")
    rng = np.random.default_rng(5)
    rec[:, 55:58] = rng.uniform(-7.5, -4.5, (len(rec), 3))
    cam = npr.camera((0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0), 45.0, 0.1, 1000.0, 640, 360)
    scene = npr.activate(rec)
    pre = npr.preprocess(scene, cam)
    vis = pre["tiles"] > 0
    assert vis.sum() > 1000
    want = aa.comp64(pre)
    c32 = want.astype(np.float32)
    assert not aa.comp_violations(c32, pre, want)[vis].any()
    pre31 = npr.preprocess(scene, cam, dict(dilation=0.31))
    for mutated in (aa.comp64(pre31, rules=dict(dilation=0.31)), aa.comp64(pre, sqrt=False), aa.comp64(pre, raw_from_dilated=True)):
        assert aa.comp_violations(mutated.astype(np.float32), pre, want)[vis].mean() > 0.5
