"""gs_photometric_loss / Renderer.photometric_loss without a GPU.  The yardstick the GPU tests compare with
(tests/photometric_loss_reference.py) is pinned here: its gradient and terms are what torch.autograd finds for an independent
float64 restatement written the way the trainers write it (tests/photometric_loss_torch.py), within the bound the module derives,
on every image of tests/photometric_loss_images.py and lambda in 0, 0.2, 1; it lies within a QUARTER of that bound of the same
formulas in binary80, so the yardstick itself is inside the contract; and each single-term mutation of it misses the bound by
more than ten times on some listed image.  Then the sizes at which the device's SUMS change regime (pli.REDUCTION_SIZES): that
they reach the regimes they were chosen for, recomputed from the kernels' constants; that the dyadic images' l1 and mse are what
integer arithmetic gives; and, on a model of the device's partition into partial-sum rows (tests/photometric_loss_rows.py), that
one dropped, doubled or stale row anywhere misses a term's bound by more than ten times, so the GPU tests at those sizes have
teeth.  Then the entry point's refusals, the structure's layout and the wrapper's checks."""
import ctypes as C
import os
from fractions import Fraction

import numpy as np
import pytest

from helpers import forbid_c, hand_made_renderer
import photometric_loss_images as pli
import photometric_loss_reference as plr
import photometric_loss_rows as plrows
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
    _assert_within_a_quarter_of_binary80(name, lam)


@pytest.mark.parametrize("h,w", [(1, pli.MAX_EXTENT), (pli.MAX_EXTENT, 1)])
def test_the_reference_lies_within_a_quarter_of_the_bound_of_binary80_on_the_thin_images_at_the_extent(h, w):
    """One pixel across: every window is mostly padding, and the sums have 3 x 16384 addends.  New geometry for the yardstick."""
    assert (h, w, pli.REDUCTION_LAMBDA) in pli.REDUCTION_SIZES
    _assert_within_a_quarter_of_binary80(f"uniform_{h}x{w}", pli.REDUCTION_LAMBDA)


def _assert_within_a_quarter_of_binary80(name, lam):
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


# ------------------------------------------------------------------------------------------------ 4. where the sums change regime
SSIM_SIZES = tuple((h, w) for h, w, lam in pli.REDUCTION_SIZES if lam != 0)
L1_SIZES = tuple((h, w) for h, w, lam in pli.REDUCTION_SIZES if lam == 0)
_IDS = [f"{h}x{w}-lambda{lam}" for h, w, lam in pli.REDUCTION_SIZES]


def test_the_reduction_sizes_stay_out_of_the_per_name_tests():
    assert not set(SSIM_SIZES + L1_SIZES) & set(pli.SIZES)
    assert len(pli.NAMES) == len(pli.SIZES) + len(pli.CONDITIONING) == 16, "the NAMES product (torch and binary80 per entry) has grown"
    assert not any(f"{h}x{w}" in name for h, w, _ in pli.REDUCTION_SIZES for name in pli.NAMES)
    assert len(set(pli.REDUCTION_SIZES)) == len(pli.REDUCTION_SIZES) == 13 and len(SSIM_SIZES) == 8 and len(L1_SIZES) == 5
    assert all(lam in (0.0, pli.REDUCTION_LAMBDA) for _, _, lam in pli.REDUCTION_SIZES)


def test_the_constants_are_the_kernels(pkg):
    src = open(os.path.join(os.path.dirname(pkg.binding.__file__), "csrc", "gs_loss.hip")).read()
    for text in (f"constexpr int kLossTile = {pli.TILE};", f"constexpr int kLossThreads = {pli.THREADS};",
                 f"constexpr uint32_t kLossL1Groups = {pli.L1_GROUPS};", f"#pragma unroll {pli.FINISH_UNROLL}\n    for (uint32_t r = threadIdx.x; r < rows;"):
        assert text in src, text
    assert pkg.binding.PHOTO_LOSS_MAX_EXTENT == pli.MAX_EXTENT


def test_the_ssim_path_sizes_reach_the_regimes_their_comments_claim():
    T, U8, tiles = pli.THREADS, pli.FINISH_UNROLL, {hw: pli.ssim_rows(*hw) for hw in SSIM_SIZES}
    rows = {hw: gy * gx for hw, (gy, gx) in tiles.items()}
    assert all(1 <= v <= pli.MAX_EXTENT for hw in SSIM_SIZES for v in hw)
    assert tiles[16, 4112] == (1, 257) and rows[16, 4112] == T + 1                 # lane 0 of the finish, and no other, takes a second row
    assert tiles[272, 272] == (17, 17) and rows[272, 272] > T                      # many tiles in both axes, and a second row for some lanes
    assert tiles[1, 16384] == (1, pli.MAX_EXTENT // pli.TILE) == (1, 1024)         # the extent across: 1024 tiles in a row ...
    assert 1 + plr.RADIUS < pli.TILE                                               # ... whose tile rows above and below row 0 are all padding
    assert tiles[16384, 1] == (1024, 1)                                            # the extent down: gridDim.y = 1024
    assert tiles[368, 1424] == (23, 89) and rows[368, 1424] == U8 * T - 1          # lanes take 7 or 8 rows: lane 255 stops one short of the body
    assert tiles[17, 16384] == (2, 1024) and rows[17, 16384] == U8 * T             # 8 rows for every lane: the unrolled body alone
    assert tiles[48, 10928] == (3, 683) and rows[48, 10928] == U8 * T + 1          # lane 0 takes a 9th row: the body, then a remainder of one
    assert tiles[33, 16384] == (3, 1024) and rows[33, 16384] == 12 * T == 3072     # 12 rows per lane:
    assert 12 > U8 and 12 % U8 != 0 and 33 % pli.TILE == 1                         # body plus remainder; the last tile row holds ONE image row
    assert max(rows.values()) == 3072 and sorted(rows.values()) == [257, 289, 1024, 1024, 2047, 2048, 2049, 3072]
    # every SSIM-path row count fits the scratch k_loss_l1 may have sized (photo_loss_partials: max(rows, L1_GROUPS)) or exceeds it
    assert sum(r > pli.L1_GROUPS for r in rows.values()) == 2


def test_the_l1_path_sizes_reach_the_regimes_their_comments_claim():
    T, cap = pli.THREADS, pli.L1_GROUPS * pli.THREADS
    E = {hw: 3 * hw[0] * hw[1] for hw in L1_SIZES}
    rows = {hw: pli.l1_rows(*hw) for hw in L1_SIZES}
    assert cap == 524288
    assert E[160, 160] == 76800 == 300 * T and rows[160, 160] == 300 < pli.L1_GROUPS             # every workgroup full, no stride
    assert E[161, 160] == 77280 and rows[161, 160] == 302 and 0 < E[161, 160] % T < T            # the last workgroup partly idle
    assert E[126, 1387] == cap - 2 and rows[126, 1387] == pli.L1_GROUPS                          # the cap's grid, no lane strides, two idle
    assert -(-E[126, 1387] // T) == pli.L1_GROUPS                                                # ... reached, not exceeded
    assert E[183, 955] == cap + 7 and rows[183, 955] == pli.L1_GROUPS                            # seven lanes take a second element
    assert -(-E[183, 955] // T) > pli.L1_GROUPS                                                  # ... only because of the cap
    assert E[350, 1249] == 1311450 and 2 * cap < E[350, 1249] < 3 * cap and rows[350, 1249] == pli.L1_GROUPS   # lanes take 2 or 3


@pytest.mark.parametrize("h,w,lam", pli.REDUCTION_SIZES, ids=_IDS)
def test_the_dyadic_images_terms_are_what_integer_arithmetic_gives(h, w, lam):
    x, y = pli.images(f"dyadic_{h}x{w}")
    n = 3 * h * w
    assert 256 * n < 2 ** 53 and 65536 * n < 2 ** 53, "the scaled sums could leave binary64's integers"
    for a in (x, y):
        k = a.astype(np.float64) * 256
        assert a.dtype == np.float32 and a.shape == (h, w, 3) and np.array_equal(k, np.rint(k)) and k.min() >= 0 and k.max() <= 256
    assert not np.array_equal(x, y)
    l1, mse = pli.dyadic_exact(x, y)
    terms = plr.evaluate(x, y, 0.0)["terms"]          # (l1 and mse do not depend on lambda)
    assert terms[1] == l1 and terms[3] == mse and terms[0] == l1 and l1 > 0 and mse > 0
    if n <= 3 * 161 * 160:      # the same from rationals, where that is quick
        fx, fy = ([Fraction(float(v)) for v in a.ravel()] for a in (x, y))
        assert l1 == float(sum(abs(p - q) for p, q in zip(fx, fy)) / n) and mse == float(sum((p - q) ** 2 for p, q in zip(fx, fy)) / n)


def _partition(h, w, lam):
    """(the model's [rows][3] partial sums, the reference's l1, ssim, mse, their bounds, n) on the uniform images."""
    key = ("rows", h, w, lam)
    if key not in _cache:
        x, y = pli.images(f"uniform_{h}x{w}")
        q = plr.evaluate(x, y, lam, parts=True)
        _cache[key] = (plrows.partial_rows(x, y, lam, q), q["terms"][1:].copy(), plr.bound(x, y, lam)["terms"][1:].copy(), float(q["n"]))
    return _cache[key]


def _escapes(delta, n, lim):
    """delta: [k][3], what a fault adds to the three sums.  (rows of delta that move NO term by more than ten bounds, the weakest
    row's best ratio.)  ssim at lambda = 0 is not evaluated (a NaN bound): it cannot witness."""
    with np.errstate(invalid="ignore"):
        ratio = np.where(np.isnan(lim), 0.0, np.abs(delta) / n / lim)
    best = ratio.max(axis=1)
    return np.flatnonzero(~(best > 10.0)), float(best.min())


def test_the_partition_model_has_the_row_counts_of_the_launch():
    for h, w, lam in pli.REDUCTION_SIZES:
        gy, gx = pli.ssim_rows(h, w)
        assert len(_partition(h, w, lam)[0]) == (gy * gx if lam != 0 else pli.l1_rows(h, w))
    # ... and its order: tile (by, bx) of the SSIM path is row by * gx + bx, element e of the L1 path is in row (e / THREADS) mod rows
    x, y = pli.images("uniform_272x272")
    d = np.abs(x.astype(np.float64) - y.astype(np.float64))
    rows = _partition(272, 272, pli.REDUCTION_LAMBDA)[0]
    assert rows[3 * 17 + 5, 0] == pytest.approx(d[48:64, 80:96].sum(), rel=1e-13) and rows[16 * 17 + 16, 0] == pytest.approx(d[256:, 256:].sum(), rel=1e-13)
    x, y = pli.images("uniform_183x955")
    d = np.abs(x.astype(np.float64) - y.astype(np.float64)).ravel()
    rows = _partition(183, 955, 0.0)[0]
    assert rows[0, 0] == pytest.approx(d[:256].sum() + d[524288:].sum(), rel=1e-13) and rows[1, 0] == pytest.approx(d[256:512].sum(), rel=1e-13)
    assert (rows[:, 1] == 0).all()


@pytest.mark.parametrize("h,w,lam", pli.REDUCTION_SIZES, ids=_IDS)
def test_one_dropped_doubled_or_stale_partial_row_misses_the_bound_by_ten_times(h, w, lam):
    """The GPU tests hold the terms to plr.bound at these sizes; that is only a test of the finish if ONE wrong row shows.  Every row
    of every size, three faults each; no row may escape.  (Had one escaped, the remedy is another seed or image for that size, never
    another factor: none was needed, every size is on the uniform images of seeds 1 and 2 like the sizes of pli.SIZES.)"""
    rows, terms, lim, n = _partition(h, w, lam)
    witness = ~np.isnan(lim)
    assert (np.abs(rows.sum(axis=0) / n - terms)[witness] <= lim[witness]).all(), "the model's rows do not sum to the reference's terms"
    assert witness.sum() == (3 if lam != 0 else 2) and (lim[witness] > 0).all()
    escaped, weakest = _escapes(rows, n, lim)          # dropped: the sums lose the row; doubled: they gain it once more
    print(f"{h} x {w}, lambda {lam}: {len(rows)} rows; a dropped or doubled row moves a term by at least {weakest:.3g} bounds", end="")
    assert len(escaped) == 0, f"dropping or doubling row {escaped[0]} of {len(rows)} moves no term by ten bounds ({weakest:.3g})"
    for oh, ow, olam in pli.REDUCTION_SIZES:           # stale: the row still holds what another size's call left at its index
        if (oh, ow, olam) == (h, w, lam):
            continue
        other = _partition(oh, ow, olam)[0]
        k = min(len(rows), len(other))
        escaped, ratio = _escapes(other[:k] - rows[:k], n, lim)
        weakest = min(weakest, ratio)
        assert len(escaped) == 0, f"row {escaped[0]} left by {oh} x {ow}, lambda {olam}, moves no term by ten bounds ({ratio:.3g})"
    print(f"; any fault, a stale row included, by at least {weakest:.3g}")


# ------------------------------------------------------------------------------------------------ 5. the C entry point
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

    forbid_c(pkg, monkeypatch)
    rend = hand_made_renderer(pkg, frame_hw=None, frames=0)      # (no frame rendered: the loss needs none)
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
