"""gs_blend_backward / Renderer.blend_backward without a GPU: the entry point and the wrapper refuse what they must before
anything touches a device, and the yardstick the GPU tests compare with (tests/backward_reference.py) is pinned three ways: its
walk gives the oracle's image bit for bit, its d_colour is lift_reference's lift of grad_rgb bit for bit, and -- walked in
binary64 over the binary32 walk's decisions -- its four sums are the gradients torch.autograd finds for a dense restatement of
render.comp:66-88 written here, independently, within the bound the module derives.  That last test pins every formula and
sign, the clamp rule included."""
import ctypes as C

import numpy as np
import pytest

import backward_reference as bref
import lift_reference as lref
from helpers import assert_images_identical, FakeTensor as _Fake, forbid_c, hand_made_renderer, oracle_frame

SCENES = {"A": (600, 72, 40), "T": (1500, 64, 64)}   # synth_records(n, seed=5, kind): n, width, height
INVALID = -1                                         # GS_ERR_INVALID


def _grads(h, w, seed=41):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((h, w, 3)).astype(np.float32), rng.standard_normal((h, w)).astype(np.float32)


@pytest.fixture(scope="module", params=sorted(SCENES))
def walked(request, pkg, oracle):
    n, w, h = SCENES[request.param]
    rec = pkg.synth.synth_records(n, seed=5, kind=request.param)
    _, _, ref = oracle_frame(oracle, rec, w, h)
    G, ga = _grads(h, w)
    return request.param, w, h, ref, G, ga, bref.backward(oracle, ref, w, h, G, ga)


def test_the_reference_walks_to_the_oracles_image(walked):
    kind, w, h, ref, G, ga, got = walked
    assert (ref["image"][..., :3] != 0).any()
    assert_images_identical(got["image"], ref["image"], label=f"backward reference, kind {kind}")


def test_d_colour_is_the_lift_of_grad_rgb_bit_for_bit(walked, oracle):
    kind, w, h, ref, G, ga, got = walked
    lifted = lref.lift(oracle, ref, w, h, G)
    assert (lifted["terms"] > 2).sum() > 100
    assert np.array_equal(got["colour"].view(np.uint64), lifted["out"].view(np.uint64))
    assert np.array_equal(got["terms"]["colour"], lifted["terms"]) and np.array_equal(got["A"]["colour"], lifted["A"])
    assert np.array_equal(got["blended"], lifted["blended"])
    for name in ("opacity", "conic", "uv"):         # a flowing pair is a blended pair
        assert (got["terms"][name] <= got["terms"]["colour"]).all()
    assert got["terms"]["colour"].sum() - got["terms"]["opacity"].sum() == got["clamped"]


def _dense_loss(conic, opac, uv, col, ref, w, h, pairs, G, ga):
    """render.comp:66-88 over the given pair sets as one dense differentiable function per tile, in torch float64 on the CPU:
    image = sum_e colour_e alpha_e T_e, T_e the product of (1 - alpha) over the blended entries in front, out_alpha = 1 - T_f;
    alpha = o exp(power) where the pair flows, the constant 0.99 where it is clamped, 0 where the pixel does not blend the
    entry.  conic [N][3], opac [N], uv [N][2], col [N][3]: torch float64 records of all N Gaussians.  Returns the scalar
    sum(G image) + sum(ga out_alpha)."""
    import torch
    bounds, payload = ref["boundaries"].astype(np.int64), ref["sorted_payload"]
    clamp = float(np.float32(0.99))
    tx = (w + 15) // 16
    loss = torch.zeros((), dtype=torch.float64)
    for t, decided in pairs.items():
        if not decided:
            continue
        x0, y0 = 16 * (t % tx), 16 * (t // tx)
        ys, xs = np.mgrid[y0:min(y0 + 16, h), x0:min(x0 + 16, w)]
        ys, xs = ys.ravel(), xs.ravel()
        ids = torch.as_tensor(payload[bounds[2 * t]:bounds[2 * t + 1]][[d[0] for d in decided]].astype(np.int64))
        blend = np.zeros((len(decided), len(xs)), bool)
        flow = np.zeros_like(blend)
        for e, (_, at, fl) in enumerate(decided):
            blend[e, at] = True
            flow[e, at[fl]] = True
        blend, flow = torch.as_tensor(blend), torch.as_tensor(flow)
        dx = uv[ids, 0][:, None] - torch.as_tensor(xs.astype(np.float64))[None, :]
        dy = uv[ids, 1][:, None] - torch.as_tensor(ys.astype(np.float64))[None, :]
        c = conic[ids]
        power = -0.5 * (c[:, 0:1] * dx * dx + c[:, 2:3] * dy * dy) - c[:, 1:2] * dx * dy
        power = torch.where(flow, power, torch.zeros_like(power))       # (masked BEFORE exp: no 0 * inf in the backward)
        alpha = torch.where(flow, opac[ids][:, None] * torch.exp(power), torch.full_like(power, clamp))
        alpha = torch.where(blend, alpha, torch.zeros_like(alpha))
        through = torch.cumprod(1.0 - alpha, dim=0)
        T = torch.cat([torch.ones((1, len(xs)), dtype=torch.float64), through[:-1]], dim=0)
        image = torch.einsum("ep,ec->pc", alpha * T, col[ids])
        loss = loss + (image * torch.as_tensor(G[ys, xs].astype(np.float64))).sum()
        loss = loss + ((1.0 - through[-1]) * torch.as_tensor(ga[ys, xs].astype(np.float64))).sum()
    return loss


def _dense_autograd(ref, w, h, pairs, G, ga):
    """The gradients of _dense_loss with respect to the oracle's records' colour, opacity, conic, uv."""
    import torch
    attr = ref["attr"]

    def leaf(a):
        return torch.tensor(np.asarray(a, np.float64), requires_grad=True)
    conic, opac = leaf(attr["conic_opacity"][:, :3]), leaf(attr["conic_opacity"][:, 3])
    uv, col = leaf(attr["uv"][:, :2]), leaf(attr["color_radii"][:, :3])
    _dense_loss(conic, opac, uv, col, ref, w, h, pairs, G, ga).backward()
    return dict(colour=col.grad.numpy(), opacity=opac.grad.numpy(), conic=conic.grad.numpy(), uv=uv.grad.numpy())


@pytest.mark.parametrize("with_alpha", [False, True], ids=["grad_alpha None", "grad_alpha random"])
def test_in_binary64_the_sums_are_the_gradients_autograd_finds(pkg, oracle, with_alpha):
    n, w, h = SCENES["A"]
    rec = pkg.synth.synth_records(n, seed=5, kind="A")
    _, _, ref = oracle_frame(oracle, rec, w, h)
    G, ga = _grads(h, w)
    ga = ga if with_alpha else None
    first = bref.backward(oracle, ref, w, h, G, ga)
    got = bref.backward(oracle, ref, w, h, G, ga, dtype=np.float64, replay=first["pairs"])
    for name in bref.OUTPUTS:                                # the replay takes the same decisions
        assert np.array_equal(got["terms"][name], first["terms"][name]), name
    want = _dense_autograd(ref, w, h, first["pairs"], G, np.zeros((h, w), np.float32) if ga is None else ga)
    for name in bref.OUTPUTS:
        err, lim = np.abs(got[name] - want[name]), bref.bound(got, name)
        assert (got["terms"][name] > 2).sum() > 100 and np.abs(want[name]).max() > 0
        print(f"{name}: worst error / bound = {float((err / np.maximum(lim, 1e-300)).max()):.3g}")
        bad = np.argwhere(~(err <= lim))
        assert len(bad) == 0, (name, len(bad), tuple(bad[0]), got[name][tuple(bad[0])], want[name][tuple(bad[0])], lim[tuple(bad[0])])


def test_clamped_pairs_carry_a_gradient_to_the_colour_only(pkg, oracle):
    """Opaque splats whose o exp(power) exceeds 0.99 near their centres (the saturated quadrant of test_gpu_blend_chunk_loop):
    the reference reports pairs that do not flow and pixels that broke, and in binary64 autograd agrees with it: alpha = 0.99 is a
    constant there."""
    from test_gpu_blend_chunk_loop import _saturated_quadrant
    rec, w, h = _saturated_quadrant(1, 0, n_weak=40, layers=8)
    _, _, ref = oracle_frame(oracle, rec, w, h)
    G, ga = _grads(h, w, seed=43)
    first = bref.backward(oracle, ref, w, h, G, ga)
    assert first["clamped"] > 0 and first["broken"].any()
    only_clamped = (first["terms"]["colour"] > 0) & (first["terms"]["opacity"] == 0)
    assert (first["opacity"][only_clamped] == 0).all() and (first["uv"][only_clamped] == 0).all()
    got = bref.backward(oracle, ref, w, h, G, ga, dtype=np.float64, replay=first["pairs"])
    want = _dense_autograd(ref, w, h, first["pairs"], G, ga)
    for name in bref.OUTPUTS:
        err, lim = np.abs(got[name] - want[name]), bref.bound(got, name)
        assert (err <= lim).all(), (name, float((err / np.maximum(lim, 1e-300)).max()))


# ------------------------------------------------------------------------------------------------ the C entry point
def _refused(pkg, r, g, word):
    L = pkg.binding.lib()
    assert L.gs_blend_backward(r, g) == INVALID
    msg = L.gs_last_error()
    assert msg and word in msg, msg


def test_invalid_arguments_are_refused_without_a_device(pkg):
    BG = pkg.binding.BlendGrads
    fake = C.c_void_p(8)              # (r is not dereferenced before every member of g has been checked)
    _refused(pkg, None, C.byref(BG()), b"null")
    _refused(pkg, fake, None, b"null")
    _refused(pkg, None, None, b"null")
    outputs = ("d_colour", "d_opacity", "d_conic", "d_uv")
    for member in outputs:            # an output without grad_rgb, with or without grad_alpha
        _refused(pkg, fake, C.byref(BG(**{member: 8192})), b"grad_rgb")
        _refused(pkg, fake, C.byref(BG(grad_alpha=4096, **{member: 8192})), b"grad_rgb")
    for member, offset in [("grad_rgb", 2), ("grad_rgb", 1), ("grad_alpha", 2), ("grad_alpha", 3)] + \
                          [(m, o) for m in outputs for o in (4, 2, 1)]:
        g = BG(grad_rgb=4096, grad_alpha=4096, d_colour=8192, d_opacity=8192, d_conic=8192, d_uv=8192)
        setattr(g, member, 8192 + offset)
        _refused(pkg, fake, C.byref(g), b"aligned")
    g = BG(grad_alpha=4096 + 2)       # misaligned with nothing asked for: still refused, by the pointer's value alone
    _refused(pkg, fake, C.byref(g), b"aligned")


def test_the_structure_has_the_headers_layout(pkg):
    BG = pkg.binding.BlendGrads
    names = ["grad_rgb", "grad_alpha", "d_colour", "d_opacity", "d_conic", "d_uv"]
    assert [f[0] for f in BG._fields_] == names
    assert C.sizeof(BG) == 48 and [getattr(BG, k).offset for k in names] == [0, 8, 16, 24, 32, 40]
    assert "gs_blend_backward" in pkg.binding.SYMBOLS
    assert "gs_backward.hip" in pkg.binding.KERNEL_SOURCES and "gs_wave_f64.h" in pkg.binding.KERNEL_SOURCES


# ------------------------------------------------------------------------------------------------ the wrapper
def test_the_wrapper_checks_its_tensors_before_it_reaches_c(pkg, monkeypatch):
    forbid_c(pkg, monkeypatch)
    rend = hand_made_renderer(pkg, frame_hw=(40, 72))
    f64 = "torch.float64"
    good = dict(grad_rgb=_Fake((40, 72, 3)), grad_alpha=_Fake((40, 72)), colour=_Fake((100, 3), f64), opacity=_Fake((100,), f64),
                conic=_Fake((100, 3), f64), uv=_Fake((100, 2), f64))
    with pytest.raises(AssertionError, match="C library was reached"):   # everything in order: the call goes through to C
        rend.blend_backward(**good)
    with pytest.raises(AssertionError, match="C library was reached"):
        rend.blend_backward(good["grad_rgb"], uv=good["uv"])
    bad = [("grad_rgb", _Fake((40, 72, 3), f64), TypeError), ("grad_rgb", _Fake((40, 72, 4)), ValueError),
           ("grad_rgb", _Fake((72, 40, 3)), ValueError), ("grad_rgb", _Fake((40, 72, 3), contiguous=False), ValueError),
           ("grad_rgb", _Fake((40, 72, 3), device="cpu"), ValueError),
           ("grad_alpha", _Fake((40, 72, 1)), ValueError), ("grad_alpha", _Fake((40, 72), f64), TypeError),
           ("colour", _Fake((100, 3)), TypeError), ("colour", _Fake((100, 4), f64), ValueError), ("colour", _Fake((99, 3), f64), ValueError),
           ("opacity", _Fake((100, 1), f64), ValueError), ("opacity", np.zeros(100), TypeError),
           ("conic", _Fake((100, 2), f64), ValueError), ("conic", _Fake((100, 3), f64, device="cuda:1"), ValueError),
           ("uv", _Fake((100, 3), f64), ValueError), ("uv", _Fake((100, 2), f64, contiguous=False), ValueError)]
    for name, tensor, error in bad:
        with pytest.raises(error, match=name):
            rend.blend_backward(**dict(good, **{name: tensor}))
    with pytest.raises(ValueError, match="grad_rgb"):                    # an output without the gradient it is the backward of
        rend.blend_backward(None, colour=good["colour"])
    with pytest.raises(ValueError, match=r"uv: the tensor is on the CPU; the arrays of Renderer\.blend_backward live on the renderer's device"):
        rend.blend_backward(good["grad_rgb"], uv=_Fake((100, 2), f64, device="cpu"))
