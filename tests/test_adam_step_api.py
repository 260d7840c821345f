"""gs_scene_adam_step and gs_visible_mask as far as a machine without a GPU can check them: the yardstick
(tests/adam_step_reference.py) against torch.optim.Adam, what keeping the moments in binary32 costs, the mask's semantics, every
refusal of the Python layer and of the C ABI (they come before a device is touched), and the learning rate of the device's
end-to-end test, chosen here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import adam_step_reference as ar
import composed_reference as comp
from helpers import FakeTensor as _Fake, forbid_c, hand_made_renderer, hand_made_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GS_ERR_INVALID = -1
U53, TINY = 2.0 ** -53, 2.0 ** -1074
LR = dict(means=1.6e-4, log_scales=5e-3, quats=1e-3, opacity_logits=5e-2, sh_dc=2.5e-3, sh_rest=1.25e-4)


def _params(pkg, n=40, seed=3, k=15, dtype=np.float32):
    return {name: v.astype(dtype) for name, v in ar.cut(pkg.synth.synth_records(n, seed=seed, kind="A"), k).items()}


# ------------------------------------------------------------------------------------------------ the ABI's shape
def test_the_symbols_are_declared_listed_and_exported_and_the_structures_have_the_headers_layout(pkg):
    with open(os.path.join(ROOT, "include", "gs3d_hip.h")) as f:
        header = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    L = pkg.binding.lib()
    for name in ("gs_scene_adam_step", "gs_visible_mask"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in pkg.binding.SYMBOLS and hasattr(L, name)
    assert "gs_optim.hip" in pkg.binding.KERNEL_SOURCES
    with open(os.path.join(ROOT, "3dgs.cpp_amd", "csrc", "Makefile")) as f:
        assert re.search(r"^KERNELS\s*:=.*\bgs_optim\.hip\b", f.read(), flags=re.M)
    G, S = pkg.binding.AdamGroup, pkg.binding.AdamStep
    assert [f[0] for f in G._fields_] == ["param", "grad", "exp_avg", "exp_avg_sq", "lr"] and C.sizeof(G) == 40
    names = list(ar.NAMES) + ["sh_rest_coeffs", "mask", "beta1", "beta2", "eps", "bias_correction1", "bias_correction2", "zero_grads"]
    assert [f[0] for f in S._fields_] == names
    assert [getattr(S, k).offset for k in names] == [0, 40, 80, 120, 160, 200, 240, 248, 256, 264, 272, 280, 288, 296] and C.sizeof(S) == 304
    body = header[header.index("} gs_adam_group;"):header.index("} gs_adam_step;")]
    order = [re.search(r"\b%s\b" % m, body).start() for m in names]
    assert order == sorted(order), "the header declares the members in another order"


# ------------------------------------------------------------------------------------------------ against torch
def test_with_the_stores_kept_in_binary64_five_steps_are_torchs_adam_within_the_counted_roundings(pkg):
    """Both sides evaluate the same real function of the same binary64 inputs; they differ in association and so in roundings.
    torch (single-tensor, foreach=False): m' = m + (1 - beta1) (g - m) [lerp]; v' = beta2 v + (1 - beta2) g g in its own order;
    the same sqrt, /, + for d; p + (-lr / bc1) m' / d in its own order.  With u = 2^-53, per element and step, |ours - torch| is at
    most -- e_m, e_v, e_p the accumulated differences, carried from step to step because the state is:
        e_m += 6 u (|m| + |g|)          three roundings a side, each of a value of magnitude at most |m| + |g|
        e_v += 8 u v'                   four a side; every term is >= 0, so v' itself is the magnitude
        |d root| <= min(sqrt(e_v), e_v / sqrt(v'))                      (|sqrt a - sqrt b| = |a - b| / (sqrt a + sqrt b))
        e_d = |d root| / sqrt(bc2) + 6 u d                              sqrt, /, + a side, all terms >= 0
        e_U = (lr / bc1) e_m / d + |U| e_d / d + 4 u |U|                the quotient's two arguments, then two roundings a side
        e_p += e_U + 2 u (|p| + |U|)                                    the subtraction, a side
    each line with 8 * 2^-1074 for results that fall into the denormals (a rounding there is absolute, not relative).  First
    order; the neglected products of two differences are below 2^-20 of the bound, which is widened by that factor."""
    torch = pytest.importorskip("torch")
    params = _params(pkg, dtype=np.float64)
    m, v = ar.zeros_like(params, np.float64), ar.zeros_like(params, np.float64)
    tp = {name: torch.tensor(p.copy(), dtype=torch.float64) for name, p in params.items()}
    opt = torch.optim.Adam([dict(params=[tp[name]], lr=LR[name]) for name in params], betas=ar.BETAS, eps=ar.EPS, foreach=False)
    e = {name: [np.zeros(p.shape) for _ in range(3)] for name, p in params.items()}     # e_m, e_v, e_p
    worst = 0.0
    for t in range(1, 6):
        grads = ar.random_gradients(params, seed=100 + t)
        every = np.abs(np.concatenate([g.reshape(-1) for g in grads.values()]))
        assert (every == 0).any() and (every == 1e30).any() and (every == 1e-30).any() and ((every != 0) & (every < 2.0 ** -1022)).any()
        for name in params:
            tp[name].grad = torch.tensor(grads[name].copy())
        before = {name: (params[name].copy(), m[name].copy()) for name in params}
        ar.step(params, {k: g.copy() for k, g in grads.items()}, m, v, LR, t=t, zero_grads=False, store=np.float64)
        opt.step()
        bc1, bc2 = ar.bias_corrections(ar.BETAS, t)
        for name in params:
            p0, m0 = before[name]
            g, e_m, e_v, e_p = grads[name], *e[name]
            size = LR[name] / bc1
            with np.errstate(all="ignore"):
                e_m += 6 * U53 * (np.abs(m0) + np.abs(g)) + 8 * TINY
                e_v += 8 * U53 * v[name] + 8 * TINY
                root = np.sqrt(v[name])
                d_root = np.where(root > 0, np.minimum(np.sqrt(e_v), e_v / np.where(root > 0, root, 1.0)), np.sqrt(e_v))
                d = root / np.sqrt(bc2) + ar.EPS
                e_d = d_root / np.sqrt(bc2) + 6 * U53 * d
                U = np.abs(size * (m[name] / d))
                e_U = size * e_m / d + U * e_d / d + 4 * U53 * U + 8 * TINY
                e_p += e_U + 2 * U53 * (np.abs(p0) + U) + 8 * TINY
            state = opt.state[tp[name]]
            for what, got, want, tol in (("exp_avg", state["exp_avg"].numpy(), m[name], e_m), ("exp_avg_sq", state["exp_avg_sq"].numpy(), v[name], e_v),
                                         ("param", tp[name].detach().numpy(), params[name], e_p)):
                err, lim = np.abs(got - want), tol * (1 + 2.0 ** -20)
                assert np.isfinite(got).all() and np.isfinite(want).all()
                ratio = float((err / np.maximum(lim, 1e-300)).max())
                worst = max(worst, ratio)
                assert (err <= lim).all(), (t, name, what, ratio)
            # the bound is the count it claims to be: where no propagated moment error dominates it stays a few ulp of |p| + |U|
            assert np.median(e_p / (np.abs(params[name]) + U + 1e-300)) < 64 * t * U53, (t, name)
    print(f"worst |torch - reference| / bound over five steps: {worst:.3g}")
    assert worst > 0, "torch and the reference agree to the bit everywhere: the comparison has no torch in it?"


def test_keeping_the_moments_in_binary32_costs_one_binary32_rounding_per_step_compounded(pkg):
    """The moments are functions of the gradients alone.  exp_avg_sq: every term is >= 0, so a store's rounding (2^-24) and the
    step's four binary64 roundings stay relative: |v32 - v64| <= ((1 + 2^-24 + 4 u)^t - 1) v64.  exp_avg may cancel, so the same
    compounding is on its magnitude A_t = beta1 A_(t-1) + (1 - beta1) |g|: b_t = b_(t-1) + (2^-24 + 4 u) (A_t + b_(t-1)).  Gradients
    here stay where binary32 neither overflows nor underflows (1e-3 .. 1e2 and exact zeros): g = 1e30 makes exp_avg_sq +inf in
    binary32 by design, and the device test has those."""
    params = _params(pkg)
    rng = np.random.default_rng(11)
    runs = {store: (ar.zeros_like(params, store), ar.zeros_like(params, store), {k: p.astype(store) for k, p in params.items()})
            for store in (np.float32, np.float64)}
    A = ar.zeros_like(params, np.float64)
    b = ar.zeros_like(params, np.float64)
    step = 2.0 ** -24 + 4 * U53
    for t in range(1, 9):
        grads = {k: rng.standard_normal(p.shape) * 10.0 ** rng.integers(-3, 3, p.shape) * (rng.random(p.shape) > 0.1) for k, p in params.items()}
        for store, (m, v, p) in runs.items():
            ar.step(p, {k: g.copy() for k, g in grads.items()}, m, v, LR, t=t, store=store)
        for name in params:
            A[name] = ar.BETAS[0] * A[name] + (1 - ar.BETAS[0]) * np.abs(grads[name])
            b[name] = b[name] + step * (A[name] + b[name])
            m32, m64 = runs[np.float32][0][name].astype(np.float64), runs[np.float64][0][name]
            v32, v64 = runs[np.float32][1][name].astype(np.float64), runs[np.float64][1][name]
            assert (np.abs(m32 - m64) <= b[name]).all(), (t, name)
            assert (np.abs(v32 - v64) <= ((1 + step) ** t - 1) * v64).all(), (t, name)
            assert runs[np.float32][0][name].dtype == np.float32 and (m32 != m64).any()


# ------------------------------------------------------------------------------------------------ the mask
@pytest.mark.parametrize("zero_grads", [True, False])
def test_unmasked_rows_keep_their_bits_and_exactly_the_masked_gradients_are_zeroed(pkg, zero_grads):
    n = 40
    params = _params(pkg, n)
    m = {k: np.full(p.shape, 0.25, np.float32) for k, p in params.items()}
    v = {k: np.full(p.shape, 0.5, np.float32) for k, p in params.items()}
    rng = np.random.default_rng(5)
    grads = {k: rng.standard_normal(p.shape) for k, p in params.items()}
    for g in grads.values():
        g[rng.random(g.shape) < 0.2] = -0.0           # a zero the step did not write is told from one it wrote by its sign
        g[7] = np.nan                                 # a NaN in an unmasked row goes nowhere
    mask = (np.arange(n) % 3 == 1).astype(np.uint8)
    assert mask[7] == 1 and mask[6] == 0
    grads2 = {k: g.copy() for k, g in grads.items()}
    for g in grads2.values():
        g[7], g[6] = 1.0, np.nan
    g_was = {k: g.copy() for k, g in grads2.items()}
    was = {k: (params[k].copy(), m[k].copy(), v[k].copy()) for k in params}
    ar.step(params, grads2, m, v, LR, t=3, mask=mask, zero_grads=zero_grads)
    off, on = mask == 0, mask != 0
    for k in params:
        for got, old in zip((params[k], m[k], v[k]), was[k]):
            assert np.array_equal(got[off].view(np.uint32), old[off].view(np.uint32)), k
            assert np.isfinite(got[on]).all() and (got[on] != old[on]).any(), k
        assert np.array_equal(grads2[k][off].view(np.uint64), g_was[k][off].view(np.uint64)), k
        assert np.isnan(grads2[k][6]).all() and (np.signbit(grads2[k][off]) & (grads2[k][off] == 0)).any()
        if zero_grads:
            assert (grads2[k][on].view(np.uint64) == 0).all(), f"{k}: a consumed gradient is not +0.0"
        else:
            assert (grads2[k][on] != 0).any() and (grads2[k][7] == 1.0).all()


def test_a_mask_of_ones_is_no_mask_and_a_mask_of_zeros_is_no_step(pkg):
    a, b, c = (dict(p=_params(pkg), g=None) for _ in range(3))
    for run, mask in ((a, None), (b, np.ones(40, np.uint8)), (c, np.zeros(40, np.uint8))):
        run["g"] = ar.random_gradients(run["p"], seed=9)
        run["m"], run["v"] = ar.zeros_like(run["p"], np.float32), ar.zeros_like(run["p"], np.float32)
        ar.step(run["p"], run["g"], run["m"], run["v"], LR, t=1, mask=mask)
    start = _params(pkg)
    for k in start:
        for what in "pmvg":
            assert a[what][k].tobytes() == b[what][k].tobytes(), (k, what)
        assert c["p"][k].tobytes() == start[k].tobytes() and not c["m"][k].any() and c["g"][k].tobytes() == ar.random_gradients(start, seed=9)[k].tobytes()


# ------------------------------------------------------------------------------------------------ the Python layer
def test_the_wrapper_checks_its_tensors_before_it_reaches_c(pkg, monkeypatch):
    forbid_c(pkg, monkeypatch)
    scene = hand_made_scene(pkg)
    f64 = "torch.float64"
    shapes = dict(means=(100, 3), log_scales=(100, 3), quats=(100, 4), opacity_logits=(100,), sh_dc=(100, 3), sh_rest=(100, 15, 3))

    def dicts(**change):
        d = dict(params={k: _Fake(s) for k, s in shapes.items()}, grads={k: _Fake(s, f64) for k, s in shapes.items()},
                 exp_avg={k: _Fake(s) for k, s in shapes.items()}, exp_avg_sq={k: _Fake(s) for k, s in shapes.items()})
        for what, (name, tensor) in change.items():
            d[what][name] = tensor
        return d

    def call(d, **kw):
        scene.adam_step(d["params"], d["grads"], d["exp_avg"], d["exp_avg_sq"], kw.pop("lr", LR), step=kw.pop("step", 1), **kw)

    with pytest.raises(AssertionError, match="C library was reached"):   # everything in order: the call goes through to C
        call(dicts())
    with pytest.raises(AssertionError, match="C library was reached"):   # ... also with one group, a mask and one rate for all
        only = {what: {"means": t["means"]} for what, t in dicts().items()}
        call(only, lr=1e-3, mask=_Fake((100,), "torch.uint8"))
    bad = [("params", "means", _Fake((100, 3), f64), TypeError), ("grads", "means", _Fake((100, 3)), TypeError),
           ("exp_avg", "quats", _Fake((100, 4), "torch.float16"), TypeError), ("exp_avg_sq", "quats", _Fake((100, 4), f64), TypeError),
           ("params", "means", _Fake((100, 4)), ValueError), ("grads", "log_scales", _Fake((99, 3), f64), ValueError),
           ("exp_avg", "opacity_logits", _Fake((100, 1)), ValueError), ("params", "sh_rest", _Fake((100, 7, 3)), ValueError),
           ("grads", "sh_rest", _Fake((100, 8, 3), f64), ValueError), ("exp_avg_sq", "sh_rest", _Fake((100, 45)), ValueError),
           ("params", "sh_dc", _Fake((100, 3), contiguous=False), ValueError), ("grads", "sh_dc", _Fake((100, 3), f64, contiguous=False), ValueError),
           ("exp_avg", "means", _Fake((100, 3), device="cpu"), ValueError), ("params", "quats", _Fake((100, 4), device="cuda:1"), ValueError),
           ("grads", "quats", np.zeros((100, 4)), TypeError)]
    for what, name, tensor, error in bad:
        with pytest.raises(error, match=name):
            call(dicts(**{what: (name, tensor)}))
    for what in ("params", "grads", "exp_avg", "exp_avg_sq"):               # a partial group, whichever member is missing
        d = dicts()
        del d[what]["log_scales"]
        with pytest.raises(ValueError, match="log_scales: a partial group"):
            call(d)
        with pytest.raises(ValueError, match="partial group"):
            call(dicts(**{what: ("quats", None)}))
    with pytest.raises(TypeError, match="unknown"):
        call(dicts(grads=("scales", _Fake((100, 3), f64))))
    for mask, error in ((_Fake((100,), "torch.bool"), TypeError), (_Fake((99,), "torch.uint8"), ValueError), (_Fake((100, 1), "torch.uint8"), ValueError),
                        (_Fake((100,), "torch.uint8", device="cpu"), ValueError)):
        with pytest.raises(error, match="mask"):
            call(dicts(), mask=mask)
    with pytest.raises(KeyError):
        call(dicts(), lr=dict(means=1e-3))
    for step in (0, -1, 1.5):
        with pytest.raises(ValueError, match="step"):
            call(dicts(), step=step)


def test_visible_mask_checks_its_tensor_before_it_reaches_c(pkg, monkeypatch):
    forbid_c(pkg, monkeypatch)
    rend = hand_made_renderer(pkg)
    with pytest.raises(AssertionError, match="C library was reached"):
        rend.visible_mask(out=_Fake((100,), "torch.uint8"), accumulate=True)
    for out, error in ((_Fake((100,), "torch.int8"), TypeError), (_Fake((101,), "torch.uint8"), ValueError),
                       (_Fake((100,), "torch.uint8", contiguous=False), ValueError), (_Fake((100,), "torch.uint8", device="cpu"), ValueError)):
        with pytest.raises(error, match="out"):
            rend.visible_mask(out=out)


# ------------------------------------------------------------------------------------------------ the C ABI's refusals
def good_step(pkg, keep, n=4, k=15, groups=ar.NAMES):
    """A gs_adam_step over host memory (never dereferenced: every call that uses it must fail before a device is touched)."""
    a = pkg.binding.AdamStep()
    width = dict(ar.WIDTH, sh_rest=3 * max(k, 1))
    for name in groups:
        g = getattr(a, name)
        arrays = [np.zeros(n * width[name], dt) for dt in (np.float32, np.float64, np.float32, np.float32)]
        keep.extend(arrays)
        g.param, g.grad, g.exp_avg, g.exp_avg_sq = (x.ctypes.data for x in arrays)
        g.lr = 1e-3
    a.sh_rest_coeffs = k
    a.beta1, a.beta2, a.eps, a.bias_correction1, a.bias_correction2, a.zero_grads = 0.9, 0.999, 1e-15, 0.1, 0.001, 1
    return a


REFUSALS = [("a partial group", "some but not all", lambda a: setattr(a.quats, "grad", None)),
            ("a partial group", "some but not all", lambda a: setattr(a.sh_dc, "param", None)),
            ("a partial group", "some but not all", lambda a: (setattr(a.means, "param", None), setattr(a.means, "grad", None), setattr(a.means, "exp_avg", None))),
            ("param off by 2", "4-byte", lambda a: setattr(a.means, "param", a.means.param + 2)),
            ("exp_avg off by 1", "4-byte", lambda a: setattr(a.log_scales, "exp_avg", a.log_scales.exp_avg + 1)),
            ("exp_avg_sq off by 3", "4-byte", lambda a: setattr(a.sh_rest, "exp_avg_sq", a.sh_rest.exp_avg_sq + 3)),
            ("grad off by 4", "8-byte", lambda a: setattr(a.opacity_logits, "grad", a.opacity_logits.grad + 4)),
            ("grad off by 1", "8-byte", lambda a: setattr(a.sh_dc, "grad", a.sh_dc.grad + 1)),
            ("sh_rest_coeffs 7", "sh_rest_coeffs", lambda a: setattr(a, "sh_rest_coeffs", 7)),
            ("sh_rest_coeffs 16", "sh_rest_coeffs", lambda a: setattr(a, "sh_rest_coeffs", 16)),
            ("sh_rest with 0", "sh_rest", lambda a: setattr(a, "sh_rest_coeffs", 0)),
            ("lr nan", "lr", lambda a: setattr(a.quats, "lr", float("nan"))),
            ("lr inf", "lr", lambda a: setattr(a.means, "lr", float("inf"))),
            ("lr < 0", "lr", lambda a: setattr(a.sh_dc, "lr", -1e-9)),
            ("beta1 = 1", "beta", lambda a: setattr(a, "beta1", 1.0)),
            ("beta1 < 0", "beta", lambda a: setattr(a, "beta1", -0.1)),
            ("beta2 = 1", "beta", lambda a: setattr(a, "beta2", 1.0)),
            ("beta2 nan", "beta", lambda a: setattr(a, "beta2", float("nan"))),
            ("eps < 0", "eps", lambda a: setattr(a, "eps", -1e-20)),
            ("eps inf", "eps", lambda a: setattr(a, "eps", float("inf"))),
            ("eps nan", "eps", lambda a: setattr(a, "eps", float("nan"))),
            ("bc1 = 0", "bias", lambda a: setattr(a, "bias_correction1", 0.0)),
            ("bc1 > 1", "bias", lambda a: setattr(a, "bias_correction1", 1.0000001)),
            ("bc2 = 0", "bias", lambda a: setattr(a, "bias_correction2", 0.0)),
            ("bc2 nan", "bias", lambda a: setattr(a, "bias_correction2", float("nan")))]


def test_the_c_call_refuses_bad_arguments_before_it_touches_a_device(pkg):
    """With s == NULL every one of these is GS_ERR_INVALID whatever else holds; the message names the argument at fault, so the
    refusal is the one meant.  (tests/test_gpu_adam_step.py repeats them on a live scene and checks that nothing moved.)"""
    L = pkg.binding.lib()
    keep = []
    for label, word, bend in REFUSALS:
        a = good_step(pkg, keep)
        bend(a)
        assert L.gs_scene_adam_step(None, C.byref(a), None) == GS_ERR_INVALID, label
        assert word in L.gs_last_error().decode(), (label, L.gs_last_error().decode())
    assert L.gs_scene_adam_step(None, C.byref(good_step(pkg, keep)), None) == GS_ERR_INVALID and "null" in L.gs_last_error().decode()
    assert L.gs_scene_adam_step(None, None, None) == GS_ERR_INVALID
    mask = np.zeros(4, np.uint8)
    assert L.gs_visible_mask(None, C.c_void_p(mask.ctypes.data), 0) == GS_ERR_INVALID and "null" in L.gs_last_error().decode()
    # the edges that are NOT refused reach the null check instead: lr = 0, eps = 0, beta = 0, a bias correction of exactly 1
    a = good_step(pkg, keep)
    a.means.lr, a.eps, a.beta1, a.beta2, a.bias_correction1, a.bias_correction2 = 0.0, 0.0, 0.0, 0.0, 1.0, 1.0
    assert L.gs_scene_adam_step(None, C.byref(a), None) == GS_ERR_INVALID and "null" in L.gs_last_error().decode()


# ------------------------------------------------------------------------------------------------ the end-to-end choice
def test_the_sparse_reference_descent_falls_at_every_step_at_the_geometry_learning_rate(pkg, oracle):
    """The loop tests/test_backward_cameras_api.py runs for composed_reference.geometry_records -- the oracle's forward, the chained
    reference gradient -- with this reference's step under each frame's visibility in place of torch's Adam, at
    composed_reference.GEOMETRY_LR for GEOMETRY_STEPS steps.  The rate tests/test_gpu_adam_step.py uses is the one asserted here."""
    assert ar.GEOMETRY_LR == comp.GEOMETRY_LR
    losses = ar.sparse_descent(pkg, oracle, ar.GEOMETRY_LR)
    print(f"lr {ar.GEOMETRY_LR:g}: losses " + " ".join(f"{v:.6g}" for v in losses))
    assert len(losses) == comp.GEOMETRY_STEPS + 1 == 7 and losses[0] > 0
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    assert np.allclose(losses, ar.GEOMETRY_LOSSES, rtol=1e-5), "the losses written beside the constant are not this run's"
