"""gs_blend_backward on the device (gs_backward.hip) against its definition restated in numpy (tests/backward_reference.py, pinned
to the oracle's image, to lift_reference and to torch.autograd by tests/test_blend_backward_api.py).  The sums are binary64, the
order of the adds and the association inside a term are unspecified, so every comparison is the bound that module derives, with no
(g, component) of any of the four outputs left out:
    |got - want| <= 2 (n_g + 8) 2^-53 A        n_g and A from the reference; a row with n_g = 0 keeps the bits it held.
Outputs are views into larger device buffers with guard words, offset so that they are 8-byte aligned and nothing more; the
gradient maps are 4-byte aligned and nothing more.  Renderers start in exp mode 2 (conftest); every test runs on both depth-order
paths."""
import ctypes as C

import numpy as np
import pytest
import torch  # at collection, before the package loads its library: both must bind the same HIP runtime

import backward_reference as bref
import limit_scenes as ls
from helpers import assert_images_identical, oracle_frame
from test_gpu_blend_chunk_loop import _grazing_scene, _saturated_quadrant, _tile_list
from test_gpu_lift import CHUNK, GUARD, SENTINEL, U53, _offset_view, _limit_frame

pytestmark = pytest.mark.gpu

SCENES = {"A": (600, 72, 40), "T": (1500, 64, 64)}    # synth_records(n, seed=5, kind) at width x height; 72 x 40 = 4.5 x 2.5 tiles
NAMES = tuple(bref.OUTPUTS)                           # colour, opacity, conic, uv
_cache = {}


def _grads(h, w, seed=41):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((h, w, 3)).astype(np.float32), rng.standard_normal((h, w)).astype(np.float32)


def _freeze(want):
    for k in NAMES:
        want[k].setflags(write=False)
    return want


def _reference(pkg, oracle, kind, with_alpha=True):
    """(oracle stages, grad_rgb, grad_alpha or None, reference) of a synthetic scene: computed once, never changed."""
    key = (kind, with_alpha)
    if key not in _cache:
        n, w, h = SCENES[kind]
        if ("frame", kind) not in _cache:
            _cache[("frame", kind)] = oracle_frame(oracle, pkg.synth.synth_records(n, seed=5, kind=kind), w, h)
        _, _, ref = _cache[("frame", kind)]
        G, ga = _grads(h, w)
        ga = ga if with_alpha else None
        _cache[key] = (ref, G, ga, _freeze(bref.backward(oracle, ref, w, h, G, ga)))
    return _cache[key]


def _open(pkg, kind):
    gs = pkg.Scene.from_records(pkg.synth.synth_records(SCENES[kind][0], seed=5, kind=kind), device=0)
    return gs, pkg.Renderer(gs)


def _uniforms(pkg, kind):
    _, w, h = SCENES[kind]
    return pkg.camera_uniforms(pkg.make_camera(), w, h)


class Sums:
    """The four outputs as float64 views into larger flat device buffers: `preload` in the views, a sentinel in the guard words."""

    def __init__(self, n, preload=0.0, only=NAMES):
        self.buf, self.t, self.preload = {}, {}, float(preload)
        for name in only:
            c = bref.OUTPUTS[name]
            shape = (n, c) if c > 1 else (n,)
            numel = int(np.prod(shape))
            self.buf[name] = torch.full((numel + 2 * GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
            self.t[name] = self.buf[name][GUARD:GUARD + numel].view(shape)
            self.t[name].fill_(self.preload)
            assert self.t[name].is_contiguous() and self.t[name].data_ptr() % 8 == 0 and self.t[name].data_ptr() % 16 != 0

    def get(self, name):
        return self.t[name].cpu().numpy()

    def guards_intact(self):
        for name, b in self.buf.items():
            g = torch.cat([b[:GUARD], b[-GUARD:]]).cpu().numpy()
            assert (g == SENTINEL).all(), f"{name}: a guard word was written"


def _assert_close(sums, want, label, times=1):
    """Every element of every output within the bound, `times` calls after the preload; rows without terms keep their bits."""
    sums.guards_intact()
    worst = {}
    for name in sums.t:
        got, total = sums.get(name), want[name]
        assert got.shape == total.shape, (label, name, got.shape, total.shape)
        lim = bref.bound(want, name, sums.preload, times)
        err = np.abs(got - (sums.preload + times * total))
        worst[name] = float((err / np.maximum(lim, 1e-300)).max())
        print(f"{label}: {name}: worst error / bound = {worst[name]:.3g}")
        bad = np.argwhere(~(err <= lim))
        assert len(bad) == 0, (f"{label}: {name} is outside the bound at {len(bad)} place(s), first {tuple(bad[0])}: "
                               f"{got[tuple(bad[0])]!r} against {(sums.preload + times * total)[tuple(bad[0])]!r}, bound {lim[tuple(bad[0])]:.3g}")
        untouched = want["terms"][name] == 0
        assert (got[untouched].view(np.uint64) == np.float64(sums.preload).view(np.uint64)).all(), f"{label}: {name}: a row without terms changed"
    return worst


def _run(rend, G, ga, want, n, label, only=NAMES, preload=0.0):
    sums = Sums(n, preload, only)
    got = rend.blend_backward(_offset_view(G, torch.float32, 1), None if ga is None else _offset_view(ga, torch.float32, 1), **sums.t)
    assert sorted(got) == sorted(sums.t)
    _assert_close(sums, want, label)
    return sums


# ------------------------------------------------------------------------------------------------ 1. whole frames
@pytest.mark.parametrize("kind", sorted(SCENES))
def test_a_whole_frame_is_within_the_bound_in_either_exp_mode_and_the_pass_reads_only(pkg, oracle, gpu, kind):
    n, w, h = SCENES[kind]
    ref, G, ga, want = _reference(pkg, oracle, kind)
    assert (want["terms"]["opacity"] > 2).sum() > 300 and want["terms"]["opacity"].max() > 256   # sums that meet in every layer
    gs, rend = _open(pkg, kind)
    try:
        u = _uniforms(pkg, kind)
        before, _ = rend.render_host(u)
        assert_images_identical(before, ref["image"], label=f"kind {kind}")
        sums = _run(rend, G, ga, want, n, f"kind {kind}, exp mode 2", preload=1.5)
        rend.blend_backward(_offset_view(G, torch.float32, 1), _offset_view(ga, torch.float32, 1), **sums.t)
        _assert_close(sums, want, f"kind {kind}, a second call into the same arrays", times=2)
        after, _ = rend.render_host(u)
        assert np.array_equal(after.view(np.uint32), before.view(np.uint32)), "a frame rendered after the pass differs"
        rend.set_exp_mode(3)                                   # the pass must not care which mode the frame ran in
        rend.render_host(u)
        _run(rend, G, ga, want, n, f"kind {kind}, exp mode 3")
        # d_colour is lift_pixels of grad_rgb, on the same frame: both within (n_g - 1) 2^-53 A of the exact sum
        got = rend.blend_backward(torch.as_tensor(G).cuda(), colour=True)
        lifted = rend.lift_pixels(torch.as_tensor(G).cuda(), out=True)["out"]
        lim = 2.0 * want["terms"]["colour"][:, None] * U53 * want["A"]["colour"]
        assert (np.abs(got["colour"].cpu().numpy() - lifted.cpu().numpy()) <= lim).all()
    finally:
        rend.close()
        gs.close()


def test_grad_alpha_given_and_null_each_output_null_in_turn_and_the_tile_cull(pkg, oracle, gpu, _sort_path):
    kind = "A"
    n, w, h = SCENES[kind]
    ref, G, ga, want = _reference(pkg, oracle, kind)
    _, _, _, want_null = _reference(pkg, oracle, kind, with_alpha=False)
    assert not np.array_equal(want["opacity"], want_null["opacity"]) and np.array_equal(want["colour"], want_null["colour"])
    gs, rend = _open(pkg, kind)
    try:
        u = _uniforms(pkg, kind)
        rend.render_host(u)
        _run(rend, G, None, want_null, n, "grad_alpha NULL")
        _run(rend, G, np.zeros((h, w), np.float32), want_null, n, "grad_alpha of zeros")
        for left_out in NAMES:                                # (a NULL output is not flushed: the others are what they were)
            _run(rend, G, ga, want, n, f"without {left_out}", only=tuple(k for k in NAMES if k != left_out))
        for alone in NAMES:
            _run(rend, G, ga, want, n, f"{alone} alone", only=(alone,))
        # all four NULL: nothing is launched, through the wrapper and through the C entry point (grad_rgb NULL too)
        assert rend.blend_backward(_offset_view(G, torch.float32, 1)) == {}
        assert rend.blend_backward(None) == {}
        assert pkg.binding.lib().gs_blend_backward(rend._h, C.byref(pkg.binding.BlendGrads())) == 0
        # sums allocated by the wrapper
        got = rend.blend_backward(torch.as_tensor(G).cuda(), torch.as_tensor(ga).cuda(), colour=True, opacity=True, conic=True, uv=True)
        for name in NAMES:
            assert got[name].dtype == torch.float64 and tuple(got[name].shape) == want[name].shape
            assert (np.abs(got[name].cpu().numpy() - want[name]) <= bref.bound(want, name)).all(), name
        # culled lists (the one-pass level 1 on the bin-local path) and the same frame without the cull: longer lists, the same sums
        # (an entry the cull drops is one every pixel of the tile skips)
        rend.set_level1_fused(1)
        rend.set_tile_cull(True)
        rend.render_host(u)
        assert rend.tile_cull()[1] == (_sort_path != "1")
        listed = rend.listed_instances()
        culled = _run(rend, G, None, want_null, n, "tile cull on")
        rend.set_tile_cull(False)
        rend.render_host(u)
        assert not rend.tile_cull()[1]
        print(f"listed instances: {listed} with the cull, {rend.listed_instances()} without")
        assert rend.listed_instances() > listed or _sort_path == "1"
        plain = _run(rend, G, None, want_null, n, "tile cull off")
        for name in NAMES:
            assert (np.abs(plain.get(name) - culled.get(name)) <= bref.bound(want_null, name)).all(), name
    finally:
        rend.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ 2. list lengths around the chunks
@pytest.mark.parametrize("k", [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1])
def test_lists_that_end_around_one_and_two_chunks(pkg, oracle, gpu, k):
    sc = ls.blend_chunk(k)
    gs, rend, u, ref = _limit_frame(pkg, oracle, sc.records, sc.width, sc.height)
    try:
        assert len(_tile_list(ref, sc.width, (2, 1))) == k
        G, ga = _grads(sc.height, sc.width)
        want = bref.backward(oracle, ref, sc.width, sc.height, G, ga)
        assert (want["terms"]["uv"] != 0).sum() == len(sc.records)    # no pixel stops early: every entry of both lists flows somewhere
        rend.render_host(u)
        _run(rend, G, ga, want, len(sc.records), f"list of {k}", preload=-0.75)
    finally:
        rend.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ 3. breaks, clamps, grazing inputs
@pytest.mark.parametrize("quadrant", [0, 3])
def test_a_quadrant_that_breaks_in_the_first_chunk_while_the_rest_walk_on(pkg, oracle, gpu, quadrant):
    """More than five chunks; one 8 x 8 block of pixels has saturated by the end of chunk 1, the other three quadrants walk the whole
    list: in BOTH walks the wave that is done stays for the barriers and adds nothing more.  The opaque splats' centre pixels have
    o exp(power) > 0.99: pairs that add to d_colour only."""
    rec, w, h = _saturated_quadrant(1, quadrant)
    gs, rend, u, ref = _limit_frame(pkg, oracle, rec, w, h)
    try:
        ids = _tile_list(ref, w, (1, 1))
        assert len(ids) > 5 * CHUNK
        G, ga = _grads(h, w)
        want = bref.backward(oracle, ref, w, h, G, ga)
        assert want["clamped"] >= 1 and want["broken"].any()     # the reference alone produces both: a pair that does not flow, a break
        y0, x0 = 16 + 8 * (quadrant >> 1), 16 + 8 * (quadrant & 1)
        assert want["broken"][y0:y0 + 8, x0:x0 + 8].all() and not want["broken"][16:32, 16:32].all()
        assert (want["terms"]["colour"][ids[3 * CHUNK:]] > 0).any()
        rend.render_host(u)
        _run(rend, G, ga, want, len(rec), f"quadrant {quadrant} breaks in chunk 1", preload=2.25)
    finally:
        rend.close()
        gs.close()


def _veiled_scene():
    """64 x 64: CHUNK + 8 faint splats in tile (1, 1) behind ONE opaque splat 2000 pixels wide, in front of everything: inside the
    image its o exp(power) exceeds 0.99 at every pixel, so every pair it has is clamped."""
    w = h = 64
    n_weak = CHUNK + 8
    weak = ls._splats(ls._spread_bits(n_weak), np.ones(n_weak), np.ones(n_weak), w, h, logit=np.log(0.02 / 0.98))
    bits = np.array([0x3FC00000], np.uint32)                   # 1.5: in front of [2, 4)
    veil = ls._splats(bits, None, None, w, h, logit=12.0, pixel=(np.array([31.5]), np.array([31.5])))
    focal = w / (2.0 * np.tan(np.radians(ls.FOV) / 2.0))
    veil[:, 55:58] = np.log(2000.0 * bits.view(np.float32).astype(np.float64) / focal)[:, None]
    return np.concatenate([weak, veil]), w, h, n_weak


def test_an_opaque_splat_whose_every_pair_is_clamped_moves_its_colour_only(pkg, oracle, gpu):
    rec, w, h, veil = _veiled_scene()
    gs, rend, u, ref = _limit_frame(pkg, oracle, rec, w, h)
    try:
        G, ga = _grads(h, w)
        want = bref.backward(oracle, ref, w, h, G, ga)
        assert want["terms"]["colour"][veil] == w * h and want["terms"]["opacity"][veil] == 0 and want["clamped"] == w * h
        assert (want["terms"]["opacity"][:veil] > 0).all()     # the faint splats behind it are blended, and flow
        rend.render_host(u)
        for preload in (0.0, -0.0, 3.5):
            sums = _run(rend, G, ga, want, len(rec), f"veil, preload {preload!r}", preload=preload)
            for name in ("opacity", "conic", "uv"):            # exactly the preloaded value -- no add at all, not an add of zero
                assert (sums.get(name)[veil].view(np.uint64) == np.float64(preload).view(np.uint64)).all(), name
            assert (sums.get("colour")[veil] != preload).all()
    finally:
        rend.close()
        gs.close()


def test_grazing_splats_and_cancelling_needles(pkg, oracle, gpu):
    rec, w, h, n_graze, n_needle, _ = _grazing_scene()
    gs, rend, u, ref = _limit_frame(pkg, oracle, rec, w, h)
    try:
        G, ga = _grads(h, w)
        want = bref.backward(oracle, ref, w, h, G, ga)
        assert (want["terms"]["conic"][:n_graze] != 0).sum() > n_graze // 4
        rend.render_host(u)
        _run(rend, G, ga, want, len(rec), "grazing splats")
    finally:
        rend.close()
        gs.close()


def test_a_nan_gradient_reaches_only_the_gaussians_blended_at_its_pixel(pkg, oracle, gpu):
    kind = "A"
    n, w, h = SCENES[kind]
    ref, G, ga, want = _reference(pkg, oracle, kind)
    y, x = np.argwhere(want["blended"] >= 3)[0]
    hit = np.zeros(n, bool)                                    # the Gaussians blended at (x, y)
    tx = (w + 15) // 16
    t = (y // 16) * tx + x // 16
    at = (y % 16) * min(16, w - 16 * (x // 16)) + x % 16
    ids = _tile_list(ref, w, (x // 16, y // 16))
    for pos, pixels, _ in want["pairs"][t]:
        if at in pixels:
            hit[ids[pos]] = True
    assert hit.sum() == want["blended"][y, x]
    poisoned = G.copy()
    poisoned[y, x, 1] = np.nan
    gs, rend = _open(pkg, kind)
    try:
        rend.render_host(_uniforms(pkg, kind))
        sums = Sums(n)
        rend.blend_backward(torch.as_tensor(poisoned).cuda(), torch.as_tensor(ga).cuda(), **sums.t)
        sums.guards_intact()
        for name in NAMES:
            got = sums.get(name).reshape(n, -1)
            assert np.isfinite(got[~hit]).all(), name
            assert (np.abs(sums.get(name) - want[name]) <= bref.bound(want, name))[~hit].all(), name
        assert np.isnan(sums.get("colour")[hit, 1]).all() and np.isfinite(sums.get("colour")[hit, 0]).all()
        assert np.isnan(sums.get("opacity")[hit]).any()
    finally:
        rend.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ 4. refusals on the device
def test_before_any_frame_the_call_is_refused_and_misaligned_pointers_write_nothing(pkg, gpu):
    kind = "A"
    n, w, h = SCENES[kind]
    gs, rend = _open(pkg, kind)
    try:
        with pytest.raises(pkg.binding.GsError) as e:
            rend.blend_backward(None)
        assert e.value.code == -1 and "no frame" in str(e.value)
        with pytest.raises(pkg.binding.GsError) as e:
            rend.blend_backward(None, uv=True)
        assert e.value.code == -1 and "no frame" in str(e.value)
        rend.render_host(_uniforms(pkg, kind))
        big = torch.zeros(3 * n + 8, dtype=torch.float64, device="cuda")
        grad = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        L = pkg.binding.lib()
        for member, offset in (("d_colour", 4), ("d_opacity", 4), ("d_conic", 4), ("d_uv", 4), ("grad_rgb", 2), ("grad_alpha", 2)):
            g = pkg.binding.BlendGrads(grad_rgb=grad.data_ptr(), grad_alpha=grad.data_ptr(), d_colour=big.data_ptr(), d_opacity=big.data_ptr(),
                                       d_conic=big.data_ptr(), d_uv=big.data_ptr())
            setattr(g, member, getattr(g, member) + offset)
            assert L.gs_blend_backward(rend._h, C.byref(g)) == -1, member
        assert (big == 0).all()
    finally:
        rend.close()
        gs.close()
