"""gs_photometric_loss on the device (gs_loss.hip) against its definition restated in numpy (tests/photometric_loss_reference.py,
pinned to torch.autograd and to binary80 by tests/test_photometric_loss_api.py): grad_rgb and the four terms within the bound that
module derives, on the images of tests/photometric_loss_images.py -- sizes below the window's radius, the kernel's tile exactly and
one more in either axis, 5 x 6 workgroups -- both pixel strides, lambda 0 and 1, badly conditioned images, a NaN pixel; that two
calls give the same bits; that the call stands beside a frame without touching it; and the autograd function down to forty Adam
steps of a small scene.  Then the sizes at which the SUMS change regime (pli.REDUCTION_SIZES): a lane of k_loss_finish takes a
second row, exactly the unrolled eight, a ninth, twelve; k_loss_l1 fills its capped grid, then strides; the extent of 16384 in
either axis; on uniform images within the same bound and on dyadic images, whose l1 and mse are one correctly rounded division,
bit for bit; the renderer's scratch carried across sizes, before any gradient call, and at pixel stride 4.  Images of the first
seven sections are at most 70 x 90, the frame 200 x 120; the reduction sizes reach 33 x 16384 (1.6 M values, 3072 rows)."""
import numpy as np
import pytest
import torch  # at collection, before the package loads its library: both must bind the same HIP runtime

import photometric_loss_images as pli
import photometric_loss_reference as plr
from test_gpu_project_backward import _parameters

pytestmark = pytest.mark.gpu
_cache = {}


@pytest.fixture(scope="module")
def rend(pkg, gpu):
    """A renderer that never renders: the loss needs its device, its stream and its scratch, not a frame."""
    scene = pkg.Scene.from_records(pkg.synth.synth_records(64, seed=3, kind="A"), device=0)
    r = pkg.Renderer(scene)
    yield r
    r.close()
    scene.close()


def _reference(key, x, y, lam):
    key = (key, lam)
    if key not in _cache:
        _cache[key] = (plr.evaluate(x, y, lam), plr.bound(x, y, lam))
    return _cache[key]


def _call(rend, x, y, lam, grad=True, terms=True):
    out = rend.photometric_loss(torch.tensor(x).cuda(), torch.tensor(y).cuda(), lam, grad=grad, terms=terms)
    return (None if out["grad_rgb"] is None else out["grad_rgb"].cpu().numpy(), None if out["terms"] is None else out["terms"].cpu().numpy())


def _assert_within_bound(grad, terms, want, lim, label, where=None):
    where = np.ones(want["grad"].shape, bool) if where is None else where
    assert grad.dtype == np.float32 and grad.shape == want["grad"].shape
    err, b = np.abs(grad.astype(np.float64) - want["grad"])[where], lim["grad"][where]
    assert np.isfinite(b).all() and (b > 0).all(), label
    ratios = [float((err / b).max())]
    for k, name in enumerate(plr.TERMS):
        if np.isnan(want["terms"][k]):
            assert np.isnan(terms[k]), (label, name)
            ratios.append(0.0)
            continue
        e = abs(float(terms[k]) - float(want["terms"][k]))
        ratios.append(0.0 if e == 0 else (float("inf") if lim["terms"][k] == 0 else e / float(lim["terms"][k])))
    print(f"{label}: worst error / bound: gradient {ratios[0]:.3g}, " + ", ".join(f"{n} {r:.3g}" for n, r in zip(plr.TERMS, ratios[1:])))
    bad = np.argwhere(~(np.abs(grad.astype(np.float64) - want["grad"]) <= lim["grad"]) & where)
    assert len(bad) == 0, f"{label}: grad_rgb{tuple(bad[0])} = {grad[tuple(bad[0])]!r} against {want['grad'][tuple(bad[0])]!r}, bound {lim['grad'][tuple(bad[0])]:.3g}"
    assert max(ratios[1:]) <= 1.0, (label, ratios)


# ------------------------------------------------------------------------------------------------ 1. sizes and strides
@pytest.mark.parametrize("h,w", pli.SIZES, ids=[f"{h}x{w}" for h, w in pli.SIZES])
def test_gradient_and_terms_lie_within_the_bound_at_every_size(rend, h, w):
    name = f"uniform_{h}x{w}"
    x, y = pli.images(name)
    want, lim = _reference(name, x, y, 0.2)
    grad, terms = _call(rend, x, y, 0.2)
    _assert_within_bound(grad, terms, want, lim, name)


@pytest.mark.parametrize("sx,sy", [(3, 3), (3, 4), (4, 3), (4, 4)])
def test_both_pixel_strides_of_either_image(rend, sx, sy):
    name = "uniform_37x53"
    x, y = pli.images(name)
    want, lim = _reference(name, x, y, 0.2)
    plain = _call(rend, x, y, 0.2)
    grad, terms = _call(rend, x if sx == 3 else pli.widen(x, 0.75), y if sy == 3 else pli.widen(y, -3.0), 0.2)
    _assert_within_bound(grad, terms, want, lim, f"{name}, strides {sx} and {sy}")
    assert np.array_equal(grad.view(np.uint32), plain[0].view(np.uint32)) and np.array_equal(terms.view(np.uint64), plain[1].view(np.uint64))


# ------------------------------------------------------------------------------------------------ 2. lambda 0 and 1, forward only
@pytest.mark.parametrize("lam", [0.0, 1.0])
def test_the_ends_of_lambda_and_the_forward_alone(rend, lam):
    name = "uniform_37x53"
    x, y = pli.images(name)
    want, lim = _reference(name, x, y, lam)
    grad, terms = _call(rend, x, y, lam)
    _assert_within_bound(grad, terms, want, lim, f"{name}, lambda {lam}")
    if lam == 0:
        n = 3 * x.shape[0] * x.shape[1]
        exact = (np.sign(x.astype(np.float64) - y.astype(np.float64)) / n).astype(np.float32)
        assert np.isnan(terms[2]) and terms[0] == terms[1]
        assert np.array_equal(grad.view(np.uint32), exact.view(np.uint32)), "lambda = 0: the gradient is fl32(sign(x - y) / n)"
    none, alone = _call(rend, x, y, lam, grad=None)
    assert none is None and np.array_equal(alone.view(np.uint64), terms.view(np.uint64)), "the forward alone gives other terms"
    only, none = _call(rend, x, y, lam, terms=None)
    assert none is None and np.array_equal(only.view(np.uint32), grad.view(np.uint32))


# ------------------------------------------------------------------------------------------------ 3. conditioning
@pytest.mark.parametrize("name", pli.CONDITIONING)
def test_badly_conditioned_images(rend, name):
    x, y = pli.images(name)
    want, lim = _reference(name, x, y, 0.2)
    grad, terms = _call(rend, x, y, 0.2)
    _assert_within_bound(grad, terms, want, lim, name)
    if name in ("equal", "const_0.5_0.5"):      # x == y: ssim within its bound of 1, the gradient within its bound of 0
        assert abs(terms[2] - 1.0) <= lim["terms"][2] and terms[1] == 0 and terms[3] == 0
        assert (np.abs(grad.astype(np.float64)) <= lim["grad"]).all()


# ------------------------------------------------------------------------------------------------ 4. a NaN pixel
def test_a_nan_goes_where_the_arithmetic_takes_it_and_nowhere_else(rend):
    x, y = pli.images("uniform_37x53")
    x = x.copy()
    x[18, 30, 1] = np.nan
    want, lim = _reference("nan_37x53", x, y, 0.2)
    grad, terms = _call(rend, x, y, 0.2)
    far = np.ones(x.shape, bool)
    far[18 - 10:18 + 11, 30 - 10:30 + 11, 1] = False
    assert np.array_equal(np.isnan(want["grad"]), ~far), "the reference's NaNs are not the pixels within 10 of the bad one, in its channel"
    assert np.array_equal(np.isnan(grad), np.isnan(want["grad"]))
    assert np.isnan(terms).all() and np.isnan(want["terms"]).all()
    err = np.abs(grad.astype(np.float64) - want["grad"])[far]
    print(f"worst error / bound away from the NaN: {float((err / lim['grad'][far]).max()):.3g}")
    assert np.isfinite(lim["grad"][far]).all() and (err <= lim["grad"][far]).all()
    # the fourth float of a stride-4 image is never read: a NaN there changes nothing, bit for bit
    clean, _ = pli.images("uniform_37x53")
    plain = _call(rend, clean, y, 0.2)
    wide = pli.widen(clean, 0.0)
    wide[18, 30, 3] = np.nan
    grad4, terms4 = _call(rend, wide, pli.widen(y, np.nan), 0.2)
    assert np.array_equal(grad4.view(np.uint32), plain[0].view(np.uint32)) and np.array_equal(terms4.view(np.uint64), plain[1].view(np.uint64))


# ------------------------------------------------------------------------------------------------ 5. reproducible; written, not added
def test_two_calls_give_the_same_bits_and_outputs_are_overwritten(rend):
    x, y = (torch.tensor(a).cuda() for a in pli.images("uniform_70x90"))
    first = rend.photometric_loss(x, y, 0.2)
    grad = torch.full((70, 90, 3), 7.0, dtype=torch.float32, device="cuda")
    terms = torch.full((4,), 7.0, dtype=torch.float64, device="cuda")
    second = rend.photometric_loss(x, y, 0.2, grad=grad, terms=terms)
    assert second["grad_rgb"] is grad and second["terms"] is terms and second["loss"].dim() == 0 and second["loss"].dtype == torch.float64
    assert np.array_equal(first["grad_rgb"].cpu().numpy().view(np.uint32), grad.cpu().numpy().view(np.uint32))
    assert np.array_equal(first["terms"].cpu().numpy().view(np.uint64), terms.cpu().numpy().view(np.uint64))
    assert float(second["loss"]) == float(terms[0]) and np.abs(grad.cpu().numpy()).max() < 1.0


# ------------------------------------------------------------------------------------------------ 6. beside a frame
def test_the_call_stands_beside_a_frame_and_leaves_it_alone(pkg, gpu, rend):
    w, h = 200, 120
    scene = pkg.Scene.from_records(pkg.synth.synth_records(4000, seed=1, kind="A"), device=0)
    r = pkg.Renderer(scene)
    try:
        u = pkg.camera_uniforms(pkg.make_camera(), w, h)
        target = torch.tensor(pli.uniform(h, w, seed=8)).cuda()
        # before any frame, at a size unrelated to any frame
        x, y = pli.images("uniform_37x53")
        want, lim = _reference("uniform_37x53", x, y, 0.2)
        _assert_within_bound(*_call(r, x, y, 0.2), want, lim, "before any frame")
        # the frame's own RGBA, with no synchronise between the render and the loss
        rgba = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        r.render(u, rgba.data_ptr())
        queued = r.photometric_loss(rgba, target, 0.2)
        r.synchronize()
        alpha = r.feature_maps(alpha=True)["alpha"].cpu().numpy()
        after = r.photometric_loss(rgba, target, 0.2)
        for k in ("grad_rgb", "terms"):
            assert np.array_equal(queued[k].cpu().numpy().view(np.uint8), after[k].cpu().numpy().view(np.uint8)), k
        assert float(after["terms"][3]) > 0 and rgba[..., :3].abs().max() > 0
        again = r.feature_maps(alpha=True)["alpha"].cpu().numpy()
        assert np.array_equal(alpha.view(np.uint32), again.view(np.uint32)) and alpha.max() > 0
        # ... against the reference, on the frame the device rendered
        frame = rgba.cpu().numpy()
        want, lim = plr.evaluate(frame, target.cpu().numpy(), 0.2), plr.bound(frame, target.cpu().numpy(), 0.2)
        _assert_within_bound(after["grad_rgb"].cpu().numpy(), after["terms"].cpu().numpy(), want, lim, "the frame at 200 x 120")
    finally:
        r.close()
        scene.close()


# ------------------------------------------------------------------------------------------------ 7. autograd
def test_the_autograd_function_scales_the_saved_gradient(rend):
    x, y = (torch.tensor(a).cuda() for a in pli.images("uniform_37x53"))
    direct = rend.photometric_loss(x, y, 0.2)
    img = x.clone().requires_grad_()
    loss = rend.differentiable_photometric_loss(img, y)
    assert loss.dim() == 0 and loss.dtype == torch.float64 and loss.is_cuda and float(loss.detach()) == float(direct["loss"])
    (2.5 * loss).backward()
    want = (np.float32(2.5) * direct["grad_rgb"].cpu().numpy()).astype(np.float32)
    assert np.array_equal(img.grad.cpu().numpy().view(np.uint32), want.view(np.uint32))
    # an RGBA image: the fourth float carries a zero gradient; the target none at all
    wide = torch.tensor(pli.widen(pli.images("uniform_37x53")[0], 0.5)).cuda().requires_grad_()
    t = y.clone().requires_grad_()
    rend.differentiable_photometric_loss(wide, t, 0.2).backward()
    g = wide.grad.cpu().numpy()
    assert np.array_equal(g[..., :3].view(np.uint32), direct["grad_rgb"].cpu().numpy().view(np.uint32)) and (g[..., 3] == 0).all() and t.grad is None


def _perturbed(pkg):
    from composed_reference import RENDER_SCENE
    n, w, h = RENDER_SCENE
    target = pkg.synth.synth_records(n, seed=9, kind="A")
    rng = np.random.default_rng(53)
    rec = target.copy()
    rec[:, 0:3] += 0.02 * rng.standard_normal((n, 3)).astype(np.float32)       # means
    rec[:, 55:58] += 0.15 * rng.standard_normal((n, 3)).astype(np.float32)     # log-scales
    rec[:, 54] += 0.3 * rng.standard_normal(n).astype(np.float32)              # opacity logits
    return rec, target, w, h


def test_render_loss_backward_fills_all_six_gradients(pkg, gpu):
    from test_gpu_project_backward import NAMES
    rec, target_rec, w, h = _perturbed(pkg)
    params = _parameters(rec, requires_grad=NAMES)
    gs = pkg.Scene.from_tensors(**{k: v.detach() for k, v in params.items()})
    r = pkg.Renderer(gs)
    try:
        u = pkg.camera_uniforms(pkg.make_camera(), w, h)
        with torch.no_grad():
            photo = r.differentiable_render(u, **_parameters(target_rec)).clone()
        rgb = r.differentiable_render(u, **params)
        r.differentiable_photometric_loss(rgb, photo).backward()
        visible = torch.as_tensor(r.stage("tiles") != 0).cuda()
        assert int(visible.sum()) > 10
        for name in NAMES:
            g = params[name].grad
            assert g is not None and bool(torch.isfinite(g).all()), name
            assert bool((g[visible].reshape(int(visible.sum()), -1).abs().sum(dim=1) > 0).any()), name
            assert bool((g[~visible] == 0).all()), name
    finally:
        r.close()
        gs.close()


def test_forty_adam_steps_lower_the_photometric_loss(pkg, gpu):
    rec, target_rec, w, h = _perturbed(pkg)
    moving = ("means", "log_scales", "opacity_logits")
    params = _parameters(rec, requires_grad=moving)
    gs = pkg.Scene.from_tensors(**{k: v.detach() for k, v in params.items()})
    r = pkg.Renderer(gs)
    try:
        u = pkg.camera_uniforms(pkg.make_camera(), w, h)
        with torch.no_grad():
            photo = r.differentiable_render(u, **_parameters(target_rec)).clone()
        opt = torch.optim.Adam([params[k] for k in moving], lr=3e-3)
        losses = []
        for step in range(41):
            opt.zero_grad()
            loss = r.differentiable_photometric_loss(r.differentiable_render(u, **params), photo)
            losses.append(loss.item())
            if step < 40:
                loss.backward()
                opt.step()
        print("losses " + " ".join(f"{v:.5g}" for v in losses[::5]))
        assert losses[0] > 0 and losses[-1] < losses[0], losses
    finally:
        r.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ 8. where the sums change regime
# pli.REDUCTION_SIZES, each on the path it was chosen for.  tests/test_photometric_loss_api.py shows on a model of the partition
# that one dropped, doubled or stale row of partial sums at any of these sizes misses a term's bound by more than ten times.
LAM = pli.REDUCTION_LAMBDA
SSIM_SIZES = [(h, w) for h, w, lam in pli.REDUCTION_SIZES if lam != 0]
L1_SIZES = [(h, w) for h, w, lam in pli.REDUCTION_SIZES if lam == 0]
SENTINEL = 7.0     # what the outputs hold before a call: an element the call does not write is far outside any bound


def _ids(sizes):
    return [f"{h}x{w}" for h, w in sizes]


def _rows(h, w, lam):
    gy, gx = pli.ssim_rows(h, w)
    return gy * gx if lam != 0 else pli.l1_rows(h, w)


def _call_prefilled(rend, x, y, lam):
    h, w = x.shape[:2]
    grad = torch.full((h, w, 3), SENTINEL, dtype=torch.float32, device="cuda")
    terms = torch.full((4,), SENTINEL, dtype=torch.float64, device="cuda")
    return _call(rend, x, y, lam, grad=grad, terms=terms)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _sign_over_n(x, y):
    """lambda = 0: grad_rgb is fl32(sign(x - y) / n), one correctly rounded division and one rounding to binary32."""
    n = 3 * x.shape[0] * x.shape[1]
    return (np.sign(x[..., :3].astype(np.float64) - y[..., :3].astype(np.float64)) / n).astype(np.float32)


def _assert_exact_l1_and_mse(terms, x, y, label):
    l1, mse = pli.dyadic_exact(x, y)
    assert float(terms[1]).hex() == l1.hex() and float(terms[3]).hex() == mse.hex(), \
        f"{label}: l1 {float(terms[1]).hex()} against {l1.hex()}, mse {float(terms[3]).hex()} against {mse.hex()}"


@pytest.mark.parametrize("h,w", SSIM_SIZES, ids=_ids(SSIM_SIZES))
def test_the_finish_adds_every_row_of_the_window_path(rend, h, w):
    name = f"uniform_{h}x{w}"
    x, y = pli.images(name)
    want, lim = _reference(name, x, y, LAM)
    grad, terms = _call_prefilled(rend, x, y, LAM)
    _assert_within_bound(grad, terms, want, lim, f"{name}, {_rows(h, w, LAM)} rows")
    none, alone = _call(rend, x, y, LAM, grad=None)      # k_loss_ssim<false>: the same finish, no maps
    assert none is None and _same_bits(alone, terms), "the forward alone gives other terms"


@pytest.mark.parametrize("h,w", L1_SIZES, ids=_ids(L1_SIZES))
def test_the_one_pass_of_lambda_zero_up_to_its_cap_and_striding_beyond(rend, h, w):
    name = f"uniform_{h}x{w}"
    x, y = pli.images(name)
    want, lim = _reference(name, x, y, 0.0)
    grad, terms = _call_prefilled(rend, x, y, 0.0)
    _assert_within_bound(grad, terms, want, lim, f"{name}, lambda 0, {_rows(h, w, 0.0)} rows")
    assert np.isnan(terms[2]) and terms[0] == terms[1]
    assert _same_bits(grad, _sign_over_n(x, y)), "lambda = 0: the gradient is fl32(sign(x - y) / n)"
    none, alone = _call(rend, x, y, 0.0, grad=None)      # k_loss_l1<false>
    assert none is None and _same_bits(alone, terms), "the forward alone gives other terms"


@pytest.mark.parametrize("lam", [LAM, 0.0], ids=["window", "lambda0"])
@pytest.mark.parametrize("h,w", SSIM_SIZES + L1_SIZES, ids=_ids(SSIM_SIZES + L1_SIZES))
def test_dyadic_images_give_l1_and_mse_bit_for_bit(rend, h, w, lam):
    """Every size on both paths.  The sums of |x - y| and (x - y)^2 are exact in binary64 in ANY order (pli.dyadic), so l1 and mse are
    one correctly rounded division by n whatever the device's association: unlike the bound, no slack for a row's arithmetic."""
    name = f"dyadic_{h}x{w}"
    x, y = pli.images(name)
    grad, terms = _call_prefilled(rend, x, y, lam)
    label = f"{name}, lambda {lam}, {_rows(h, w, lam)} rows"
    _assert_exact_l1_and_mse(terms, x, y, label)
    if lam == 0:
        assert float(terms[0]).hex() == float(terms[1]).hex() and np.isnan(terms[2]), label
        assert _same_bits(grad, _sign_over_n(x, y)), label
    else:
        want, lim = _reference(name, x, y, lam)
        _assert_within_bound(grad, terms, want, lim, label)


def test_the_scratch_of_one_size_does_not_reach_the_sums_of_the_next(rend):
    """One renderer, one scratch: 3072 rows, then 257, then k_loss_l1's 2048 (of which 257 .. 2047 would still hold the first call's
    sums had nothing rewritten them), 302, and the first size again.  A finish that reads a row beyond this call's count, or a
    kernel that leaves one of its rows unwritten, adds a stale row: l1 and mse of a dyadic pair then miss their bit pattern."""
    order = [(33, 16384, LAM), (16, 4112, LAM), (350, 1249, 0.0), (161, 160, 0.0), (33, 16384, LAM)]
    assert [_rows(*o) for o in order] == [3072, 257, 2048, 302, 3072]
    got = []
    for k, (h, w, lam) in enumerate(order):
        x, y = pli.images(f"dyadic_{h}x{w}")
        got.append(_call_prefilled(rend, x, y, lam))
        _assert_exact_l1_and_mse(got[-1][1], x, y, f"call {k + 1}, {h} x {w}, lambda {lam}")
        if lam == 0:
            assert _same_bits(got[-1][0], _sign_over_n(x, y))
    assert _same_bits(got[4][1], got[0][1]) and _same_bits(got[4][0], got[0][0]), "the first size again gives other bits"
    x, y = pli.images("dyadic_33x16384")
    want, lim = _reference("dyadic_33x16384", x, y, LAM)
    _assert_within_bound(*got[4], want, lim, "33 x 16384 after three other sizes")


def test_the_forward_alone_on_a_renderer_that_never_formed_a_gradient(pkg, gpu):
    """The map scratch has never been allocated when k_loss_ssim<false> runs; the later call with the gradient allocates it."""
    h, w = 17, 16384
    name = f"uniform_{h}x{w}"
    x, y = pli.images(name)
    want, lim = _reference(name, x, y, LAM)
    scene = pkg.Scene.from_records(pkg.synth.synth_records(64, seed=3, kind="A"), device=0)
    r = pkg.Renderer(scene)
    try:
        none, alone = _call(r, x, y, LAM, grad=None)
        grad, terms = _call_prefilled(r, x, y, LAM)
    finally:
        r.close()
        scene.close()
    assert none is None and _same_bits(alone, terms), "the forward alone gives other terms"
    _assert_within_bound(grad, terms, want, lim, f"{name} on a fresh renderer")


@pytest.mark.parametrize("h,w,lam", [(33, 16384, LAM), (350, 1249, 0.0)], ids=["33x16384", "350x1249-lambda0"])
def test_two_calls_give_the_same_bits_where_lanes_take_many_rows(rend, h, w, lam):
    name = f"uniform_{h}x{w}"
    x, y = pli.images(name)
    want, lim = _reference(name, x, y, lam)
    first, second = _call_prefilled(rend, x, y, lam), _call_prefilled(rend, x, y, lam)
    assert _same_bits(first[0], second[0]) and _same_bits(first[1], second[1])
    _assert_within_bound(*second, want, lim, f"{name}, lambda {lam}, the second call")


def test_pixel_stride_four_at_the_extent(rend):
    """17 x 16384 at strides (4, 4): p * stride there is the largest index any test forms.  Bit-equal to strides (3, 3)."""
    h, w = 17, 16384
    name = f"uniform_{h}x{w}"
    x, y = pli.images(name)
    want, lim = _reference(name, x, y, LAM)
    plain = _call_prefilled(rend, x, y, LAM)
    grad, terms = _call_prefilled(rend, pli.widen(x, 0.75), pli.widen(y, -3.0), LAM)
    _assert_within_bound(grad, terms, want, lim, f"{name}, strides 4 and 4")
    assert _same_bits(grad, plain[0]) and _same_bits(terms, plain[1])
