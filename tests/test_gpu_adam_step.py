"""gs_scene_adam_step and gs_visible_mask on the device.  The step's contract is a bit pattern (include/gs3d_hip.h): parameters,
both moments and the gradients are compared bit for bit with tests/adam_step_reference.py, the scene with a scene built by
Scene.from_tensors from the reference's new parameters -- its vertices, cov3D, raw blob, alpha cuts and a frame, with the helpers
of tests/test_gpu_device_arrays.py.  Scenes hold at most 1 500 Gaussians, frames are at most 128 x 96."""
import ctypes as C

import numpy as np
import pytest
import torch  # at collection, before the package loads its library: both must bind the same HIP runtime

import adam_step_reference as ar
import backward_cameras as bc
import composed_reference as comp
from test_adam_step_api import LR, REFUSALS
from test_gpu_device_arrays import H, W, once, raw_blob, same, same_state, state

pytestmark = pytest.mark.gpu

B = 256                      # k_adam_step's Gaussians per workgroup (gs_optim.hip: BLOCK)
GS_ERR_INVALID = -1
_records = {}


def records(pkg, n, seed=3):
    if (n, seed) not in _records:
        r = pkg.synth.synth_records(n, seed=seed, kind="A")
        r.setflags(write=False)
        _records[(n, seed)] = r
    return _records[(n, seed)]


def zero_bands_beyond(r, k):
    """Records whose SH coefficients above the first k are zero: what Scene.from_tensors makes of an sh_rest of k coefficients."""
    r = r.copy()
    for c in range(3):
        r[:, 9 + 15 * c + k:9 + 15 * (c + 1)] = 0
    return r


def device(a, dtype=None, offset=False):
    """A contiguous device tensor holding numpy array `a`; offset: a slice one element into a larger allocation, so that a
    float32 tensor is 4-byte but not 16-byte aligned and a float64 one 8-byte but not 16-byte aligned."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    if not offset:
        return t.cuda()
    big = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
    big[1:].copy_(t.reshape(-1))
    d = big[1:].view(t.shape)
    assert d.data_ptr() % 16 == t.element_size() and d.is_contiguous()
    return d


def same_bits(dev, host, label):
    """Bitwise equality of a device tensor and the reference's array; a NaN of the reference is a NaN here (the default NaNs of
    x86 and gfx950 differ in sign)."""
    got = dev.cpu().numpy()
    assert got.dtype == host.dtype and got.shape == host.shape, (label, got.dtype, host.dtype, got.shape, host.shape)
    bits = np.uint32 if host.dtype == np.float32 else np.uint64
    nan = np.isnan(host)
    assert np.isnan(got[nan]).all(), f"{label}: a NaN of the reference is a number here"
    bad = np.argwhere((got.view(bits) != host.view(bits)) & ~nan)
    assert len(bad) == 0, f"{label}: {len(bad)} value(s) differ in their bits, first at {tuple(bad[0])}: {got[tuple(bad[0])]!r} != {host[tuple(bad[0])]!r}"


class Run:
    """A scene built from the tensors of `base` records (sh_rest with k coefficients), the trainer's state on the device and the
    reference's on the host, stepped side by side."""

    def __init__(self, pkg, base, k=15, groups=ar.NAMES, offset=False, scene=None, lr=LR):
        self.pkg, self.k, self.lr, self.offset = pkg, k, lr, offset
        full = ar.cut(base, k)
        self.base = base                                              # what the scene holds where no group is stepped
        self.host = {name: full[name] for name in groups if not (name == "sh_rest" and k == 0)}
        self.m, self.v = ar.zeros_like(self.host, np.float32), ar.zeros_like(self.host, np.float32)
        self.dev = {name: device(a, offset=offset) for name, a in self.host.items()}
        self.dm = {name: device(a, offset=offset) for name, a in self.m.items()}
        self.dv = {name: device(a, offset=offset) for name, a in self.v.items()}
        self.dg = {name: device(np.zeros(a.shape), offset=offset) for name, a in self.host.items()}
        self.g = None
        self.scene = scene or pkg.Scene.from_tensors(**{name: device(a) for name, a in full.items()})
        self.t = 0

    def step(self, mask, grads=None, zero_grads=True):
        self.t += 1
        self.g = grads or ar.random_gradients(self.host, seed=40 + self.t)
        for name, g in self.g.items():
            self.dg[name].copy_(torch.from_numpy(g))
        dmask = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask, np.uint8)).cuda()
        self.scene.adam_step(self.dev, self.dg, self.dm, self.dv, self.lr, ar.BETAS, ar.EPS, self.t, mask=dmask, zero_grads=zero_grads)
        ar.step(self.host, self.g, self.m, self.v, self.lr, ar.BETAS, ar.EPS, self.t, mask=mask, zero_grads=zero_grads)

    def check_tensors(self, label):
        for name in self.host:
            same_bits(self.dev[name], self.host[name], f"{label}: {name}")
            same_bits(self.dm[name], self.m[name], f"{label}: exp_avg of {name}")
            same_bits(self.dv[name], self.v[name], f"{label}: exp_avg_sq of {name}")
            same_bits(self.dg[name], self.g[name], f"{label}: the gradient of {name}")

    def records_now(self):
        return ar.records_of(self.host, self.base)

    def fresh_scene(self):
        """Scene.from_tensors of the reference's parameters (the groups that are not stepped: the base's)."""
        full = ar.cut(self.records_now(), 15)
        return self.pkg.Scene.from_tensors(**{name: device(a) for name, a in full.items()})

    def check_scene(self, label, before=None, mask=None):
        fresh = self.fresh_scene()
        same(self.scene.download_vertices(), fresh.download_vertices(), f"{label}: vertices")
        same(self.scene.download_cov3d(), fresh.download_cov3d(), f"{label}: cov3D")
        same(raw_blob(self.scene), raw_blob(fresh), f"{label}: the blob")
        fresh.close()
        if before is not None and mask is not None:
            off = np.asarray(mask) == 0
            same(self.scene.download_vertices()[off], before[0][off], f"{label}: vertices of unmasked Gaussians")
            same(self.scene.download_cov3d().reshape(len(off), -1)[off], before[1].reshape(len(off), -1)[off], f"{label}: cov3D of unmasked Gaussians")


def masks(n):
    """all; none; one Gaussian (the first, the last, one in the middle); alternating; one whole workgroup empty between two full
    ones (where the scene has three) -- without repeats."""
    out = {"all (NULL)": None, "all": np.ones(n, np.uint8), "none": np.zeros(n, np.uint8)}
    for label, at in (("the first", 0), ("the last", n - 1), ("one in the middle", n // 2)):
        m = np.zeros(n, np.uint8)
        m[at] = 1
        out[label] = m
    out["alternating"] = (np.arange(n) % 2).astype(np.uint8)
    if n >= 3 * B:
        m = np.ones(n, np.uint8)
        m[B:2 * B] = 0
        out["an empty workgroup between two full ones"] = m
    seen, unique = set(), {}
    for label, m in out.items():
        key = None if m is None else m.tobytes()
        if key not in seen:
            seen.add(key)
            unique[label] = m
    return unique


# ------------------------------------------------------------------------------------------------ bit-equality
@pytest.mark.parametrize("k", [0, 3, 8, 15])
@pytest.mark.parametrize("n", [1, B - 1, B, B + 1, 3 * B + 7])
def test_parameters_moments_gradients_and_the_scene_are_the_references_bit_for_bit(pkg, gpu, _sort_path, n, k):
    """After one step and after three, under every mask; gradients hold zeros, denormals and 1e+-30 (exp_avg_sq overflows to +inf
    in binary32 there, by the contract's store)."""
    once(_sort_path)
    base = zero_bands_beyond(records(pkg, n), k)
    for label, mask in masks(n).items():
        run = Run(pkg, base, k)
        before = (run.scene.download_vertices(), run.scene.download_cov3d())
        for t in (1, 2, 3):
            run.step(mask)
            if t in (1, 3):
                run.check_tensors(f"n={n} k={k} mask {label}, step {t}")
                run.check_scene(f"n={n} k={k} mask {label}, step {t}", before, mask)
        run.scene.close()


def test_slices_that_are_four_and_eight_byte_aligned_and_no_more(pkg, gpu, _sort_path):
    once(_sort_path)
    n = B + 1
    run = Run(pkg, records(pkg, n), 15, offset=True)
    mask = (np.arange(n) % 2).astype(np.uint8)
    for t in (1, 2, 3):
        run.step(mask)
        run.check_tensors(f"offset slices, step {t}")
        run.check_scene(f"offset slices, step {t}")


def test_without_zero_grads_the_gradients_keep_their_bits(pkg, gpu, _sort_path):
    once(_sort_path)
    n = B + 1
    run = Run(pkg, records(pkg, n), 15)
    run.step((np.arange(n) % 3 == 0).astype(np.uint8), zero_grads=False)
    run.check_tensors("zero_grads = False")
    assert all(np.count_nonzero(g) > g.size // 2 for g in run.g.values())


# ------------------------------------------------------------------------------------------------ groups absent
PLANES = dict(means=(0, 3), log_scales=(3, 6), quats=(6, 10), opacity_logits=(10, 11))


@pytest.mark.parametrize("groups", [("means",), ("opacity_logits",), ("sh_dc", "sh_rest")], ids=lambda g: "+".join(g))
def test_a_group_that_is_not_stepped_keeps_its_planes(pkg, gpu, _sort_path, groups):
    once(_sort_path)
    n = B + 44
    st = (n + 15) // 16 * 16
    run = Run(pkg, records(pkg, n), 15, groups=groups)
    was = raw_blob(run.scene)
    mask = (np.arange(n) % 2).astype(np.uint8)
    run.step(mask)
    run.check_tensors("+".join(groups))
    run.check_scene("+".join(groups))
    now = raw_blob(run.scene)
    for name, (lo, hi) in PLANES.items():
        kept = np.array_equal(now[lo * st:hi * st].view(np.uint32), was[lo * st:hi * st].view(np.uint32))
        assert kept == (name not in groups), name
    sh_was, sh_now = was[11 * st:].reshape(n, 48), now[11 * st:].reshape(n, 48)
    assert np.array_equal(sh_now.view(np.uint32), sh_was.view(np.uint32)) == ("sh_dc" not in groups)
    assert np.array_equal(sh_now[mask == 0].view(np.uint32), sh_was[mask == 0].view(np.uint32))


def test_an_opacity_only_step_takes_the_opacity_flag_behind_exp_mode_3_again(pkg, gpu, _sort_path):
    """The scene starts with ONE opacity above 1 (from vertices), so exp mode 3 runs as mode 2.  An opacity-only step rewrites
    every opacity from its logit -- one of them pushed to exactly 1.0f: logit 16 + 1 (lr 1, the first step moves by lr) -- and
    the flag must be taken again: the mode-3 frame afterwards is, bit for bit, the mode-3 frame of a scene built from the new
    parameters, and no longer the mode-2 frame."""
    n, at, pushed = 1200, 77, 300
    r = records(pkg, n).copy()
    r[pushed, 54] = 16.0
    verts = pkg.activate_records(r)
    verts[at, 7] = 2.0
    scene = pkg.Scene.from_vertices(verts)
    rend = pkg.Renderer(scene)
    u = pkg.camera_uniforms(pkg.make_camera(), W, H)
    rend.set_exp_mode(3)
    as3, _ = rend.render_host(u)
    rend.set_exp_mode(2)
    as2, _ = rend.render_host(u)
    assert np.array_equal(as3.view(np.uint32), as2.view(np.uint32))       # mode 3 ran as mode 2
    rend.synchronize()
    run = Run(pkg, r, 15, groups=("opacity_logits",), scene=scene, lr=1.0)
    g = dict(opacity_logits=np.full(n, -1e-3))
    g["opacity_logits"][::2] = 2e-3
    g["opacity_logits"][pushed] = -1e-3
    run.step(None, grads=g)
    run.check_tensors("opacity only")
    assert run.host["opacity_logits"][pushed] == np.float32(17.0)
    now = scene.download_vertices()
    assert now[pushed, 7] == np.float32(1.0) and now[:, 7].max() == np.float32(1.0)
    fresh = run.fresh_scene()
    same(now, fresh.download_vertices(), "opacity only: vertices")
    frames = {}
    for name, (s, rd) in dict(stepped=(scene, rend), fresh=(fresh, pkg.Renderer(fresh))).items():
        for mode in (3, 2):
            rd.set_exp_mode(mode)
            frames[name, mode], _ = rd.render_host(u)
    for mode in (3, 2):
        assert np.array_equal(frames["stepped", mode].view(np.uint32), frames["fresh", mode].view(np.uint32)), f"exp mode {mode}"
    assert not np.array_equal(frames["stepped", 3].view(np.uint32), frames["stepped", 2].view(np.uint32))   # v_exp_f32 is back


def test_sh_bands_beyond_k_keep_their_bits(pkg, gpu, _sort_path):
    """A scene loaded with 15 coefficients and stepped with K = 3 keeps coefficients 4 .. 15 (an update would zero them)."""
    once(_sort_path)
    n = B + 9
    base = records(pkg, n)
    scene = pkg.Scene.from_records(base)
    was = scene.download_vertices()
    run = Run(pkg, base, 3, scene=scene)
    run.step(None)
    run.check_tensors("K = 3 of 15")
    now = scene.download_vertices()
    sh_was, sh_now = was[:, 12:60], now[:, 12:60]
    assert np.array_equal(sh_now[:, 12:].view(np.uint32), sh_was[:, 12:].view(np.uint32)) and (sh_was[:, 12:] != 0).all(axis=0).any()
    assert (sh_now[:, :12] != sh_was[:, :12]).any(axis=0).all()
    same(now, ar.vertices_of(pkg, run.host, base), "K = 3 of 15: vertices")


# ------------------------------------------------------------------------------------------------ derived data
@pytest.mark.parametrize("variant", ["spatial copy", "quantised", "plain"])
def test_a_frame_after_the_step_is_the_frame_of_a_fresh_scene_and_renderer(pkg, gpu, _sort_path, monkeypatch, variant):
    """Stage by stage as tests/test_gpu_device_arrays.py compares two scenes: vertices, cov3D (in ITS order under a copy in spatial
    order), the blob, the alpha cuts of the visible Gaussians, the pixels -- after a step under the frame's visible mask."""
    if variant == "spatial copy":
        monkeypatch.setenv("GS_SPATIAL_MIN", "1")
    n = 1500
    run = Run(pkg, records(pkg, n), 15)
    if variant == "quantised":
        run.scene.quantize_sh()
    rend = pkg.Renderer(run.scene)
    stale = state(pkg, run.scene, rend=rend)
    rend.synchronize()
    mask = rend.visible_mask()
    assert np.array_equal(mask.cpu().numpy() != 0, stale["visible"]) and stale["visible"].sum() > 0
    lr = {name: 20 * v for name, v in LR.items()}                          # (a step large enough to move pixels)
    run.lr = lr
    rng = np.random.default_rng(8)
    run.step(mask.cpu().numpy(), grads={name: rng.standard_normal(a.shape) for name, a in run.host.items()})
    run.check_tensors(variant)
    fresh = run.fresh_scene()
    if variant == "quantised":
        fresh.quantize_sh()
        assert run.scene.sh_bits == 16
    want = state(pkg, fresh)
    got = state(pkg, run.scene, rend=rend)
    same_state(got, want, variant)
    assert not np.array_equal(got["image"], stale["image"])


# ------------------------------------------------------------------------------------------------ NaN
def test_a_nan_gradient_reaches_its_own_gaussian_and_no_other(pkg, gpu, _sort_path):
    once(_sort_path)
    n, at = B + 30, 200
    run = Run(pkg, records(pkg, n), 15)
    before = run.scene.download_vertices()
    grads = ar.random_gradients(run.host, seed=77)
    for g in grads.values():
        g[at] = np.nan
    mask = np.ones(n, np.uint8)
    mask[at + 1] = 0
    run.step(mask, grads=grads)
    run.check_tensors("NaN")
    others = np.arange(n) != at
    for name in run.host:
        for what, t in (("param", run.dev[name]), ("exp_avg", run.dm[name]), ("exp_avg_sq", run.dv[name])):
            got = t.cpu().numpy().reshape(n, -1)
            assert np.isnan(got[at]).all() and not np.isnan(got[others]).any(), (name, what)
    now = run.scene.download_vertices()
    planes = np.r_[0:3, 4:60]                                              # (slot 3 is the constant 1 of the vertex layout)
    assert np.isnan(now[at][planes]).all() and not np.isnan(now[others]).any()
    same(now[others], ar.vertices_of(pkg, run.host, run.base)[others], "NaN: the other Gaussians")
    same(now[at + 1], before[at + 1], "NaN: the unmasked neighbour")


# ------------------------------------------------------------------------------------------------ visible_mask
def test_visible_mask_is_the_tiles_tap_by_scene_id_and_accumulates(pkg, gpu, _sort_path, monkeypatch):
    n, w, h = 1500, 96, 64
    r = records(pkg, n)
    plain = pkg.Scene.from_records(r)
    monkeypatch.setenv("GS_SPATIAL_MIN", "1")
    spatial = pkg.Scene.from_records(r)
    monkeypatch.delenv("GS_SPATIAL_MIN")
    rgba = torch.zeros(h, w, 4, device="cuda")
    torch.cuda.synchronize()
    answers = {}
    for name, scene in (("plain", plain), ("spatial", spatial)):
        rend = pkg.Renderer(scene)
        with pytest.raises(pkg.binding.GsError, match="no frame rendered yet") as e:
            rend.visible_mask()
        assert e.value.code == GS_ERR_INVALID
        union = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
        union.zero_()
        seen = []
        for cam in ("C1", "C2"):
            rend.render(pkg.camera_uniforms(bc.camera(pkg, cam), w, h), rgba.data_ptr())
            rend.synchronize()
            tiles = rend.stage("tiles") != 0
            m = rend.visible_mask()
            assert m.dtype == torch.uint8 and tuple(m.shape) == (n,) and m.is_cuda
            assert np.array_equal(m.cpu().numpy(), tiles.astype(np.uint8)), (name, cam)
            assert rend.visible_mask(out=union, accumulate=True) is union
            seen.append(tiles)
        print(f"{name}: visible under C1 {int(seen[0].sum())}, under C2 {int(seen[1].sum())}, under either {int((seen[0] | seen[1]).sum())} of {n}")
        assert seen[0].sum() > 0 and seen[1].sum() > 0
        assert np.array_equal(union.cpu().numpy(), (seen[0] | seen[1]).astype(np.uint8)), name
        out = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
        rend.visible_mask(out=out)                                        # not accumulating: what was there is overwritten
        assert np.array_equal(out.cpu().numpy(), seen[1].astype(np.uint8))
        answers[name] = seen
        rend.close()
    for a, b in zip(answers["plain"], answers["spatial"]):                # by scene id, whatever order the frame read the scene in
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_of_the_header_leaves_parameters_moments_and_scene_untouched(pkg, gpu, _sort_path):
    once(_sort_path)
    n = 300
    run = Run(pkg, records(pkg, n), 15)
    rng = np.random.default_rng(4)
    for name, a in run.host.items():
        run.dg[name].copy_(torch.from_numpy(rng.standard_normal(a.shape)))
        run.dm[name].fill_(0.25)
        run.dv[name].fill_(0.5)
    tensors = [t for d in (run.dev, run.dg, run.dm, run.dv) for t in d.values()]
    was = [t.clone() for t in tensors]
    blob = raw_blob(run.scene)
    L = pkg.binding.lib()

    def struct():
        a = pkg.binding.AdamStep()
        for name in run.host:
            g = getattr(a, name)
            g.param, g.grad, g.exp_avg, g.exp_avg_sq = (d[name].data_ptr() for d in (run.dev, run.dg, run.dm, run.dv))
            g.lr = 1e-3
        a.sh_rest_coeffs = 15
        a.beta1, a.beta2, a.eps, a.bias_correction1, a.bias_correction2, a.zero_grads = 0.9, 0.999, 1e-15, 0.1, 0.001, 1
        return a

    torch.cuda.synchronize()
    for label, word, bend in REFUSALS:
        a = struct()
        bend(a)
        assert L.gs_scene_adam_step(run.scene._h, C.byref(a), None) == GS_ERR_INVALID, label
        assert word in L.gs_last_error().decode(), (label, L.gs_last_error().decode())
    assert L.gs_scene_adam_step(None, C.byref(struct()), None) == GS_ERR_INVALID
    assert L.gs_scene_adam_step(run.scene._h, None, None) == GS_ERR_INVALID
    assert L.gs_scene_adam_step(run.scene._h, C.byref(pkg.binding.AdamStep()), None) == GS_ERR_INVALID   # (beta, eps and the corrections of a zeroed struct)
    none = struct()
    for name in ar.NAMES:
        g = getattr(none, name)
        g.param = g.grad = g.exp_avg = g.exp_avg_sq = None
    assert L.gs_scene_adam_step(run.scene._h, C.byref(none), None) == 0                                  # no group at all: a successful no-op
    torch.cuda.synchronize()
    for t, old in zip(tensors, was):
        assert torch.equal(t.view(torch.uint8), old.view(torch.uint8))
    assert np.array_equal(raw_blob(run.scene).view(np.uint32), blob.view(np.uint32))
    assert int(blob.view(np.uint32).astype(np.uint64).sum()) == int(raw_blob(run.scene).view(np.uint32).astype(np.uint64).sum())
    assert L.gs_scene_adam_step(run.scene._h, C.byref(struct()), None) == 0                              # ... and the good struct does step
    assert not np.array_equal(raw_blob(run.scene).view(np.uint32), blob.view(np.uint32))


# ------------------------------------------------------------------------------------------------ end to end
def test_six_sparse_adam_steps_without_torchs_optimiser_lower_the_loss_every_time(pkg, gpu):
    """The loop of INTEGRATION.md 3k on the scene, camera, target and rate of the CPU check
    (tests/test_adam_step_api.py: adam_step_reference.GEOMETRY_LR, losses GEOMETRY_LOSSES there): render, the squared-error
    gradient grad_rgb = 2 (rgb - target) as float32, blend_backward, project_backward into gradients zeroed ONCE, pkg.Adam.step
    under the frame's visible mask.  Seven losses, six steps, falling at every step -- the assertion
    tests/test_gpu_backward_cameras.py makes for torch's Adam, and nothing tighter -- and after each step the scene is bit for bit
    Scene.from_tensors of the stepped parameters."""
    n, w, h = comp.RENDER_SCENE
    rec, target_rec = comp.geometry_records(pkg.synth)
    u = pkg.camera_uniforms(bc.camera(pkg, comp.GEOMETRY_CAMERA), w, h)
    rgba = torch.zeros(h, w, 4, device="cuda")
    torch.cuda.synchronize()
    target_scene = pkg.Scene.from_records(target_rec)
    target_rend = pkg.Renderer(target_scene)
    target_rend.render(u, rgba.data_ptr())
    target_rend.synchronize()
    target = rgba[..., :3].clone()
    target_rend.close()
    target_scene.close()
    params = {name: device(a) for name, a in ar.cut(rec).items()}
    scene = pkg.Scene.from_tensors(**params)
    rend = pkg.Renderer(scene)
    moving = {name: params[name] for name in ar.GEOMETRY_GROUPS}
    opt = pkg.Adam(scene, moving, lr=ar.GEOMETRY_LR)
    assert opt.eps == ar.EPS and opt.betas == ar.BETAS
    grads = {name: torch.zeros_like(t, dtype=torch.float64) for name, t in moving.items()}          # zeroed ONCE
    losses = []
    try:
        for step in range(comp.GEOMETRY_STEPS + 1):
            rend.render(u, rgba.data_ptr())
            rend.synchronize()
            diff = rgba[..., :3] - target
            losses.append(float((diff ** 2).sum().item()))
            if step == comp.GEOMETRY_STEPS:
                break
            sums = rend.blend_backward((2.0 * diff).contiguous(), colour=True, opacity=True, conic=True, uv=True)
            rend.project_backward(out=grads, **sums)
            assert all(g.abs().max().item() > 0 for g in grads.values())
            opt.step(grads, mask=rend.visible_mask())
            assert all(not g.any().item() for g in grads.values()), "a gradient row the step did not consume"
            fresh = pkg.Scene.from_tensors(**params)
            same(scene.download_vertices(), fresh.download_vertices(), f"after step {step + 1}: vertices")
            same(raw_blob(scene), raw_blob(fresh), f"after step {step + 1}: the blob")
            fresh.close()
        print(f"lr {ar.GEOMETRY_LR:g}: losses " + " ".join(f"{v:.6g}" for v in losses))
        assert opt.t == comp.GEOMETRY_STEPS and all(bool(m.any().item()) for m in opt.state["exp_avg"].values())
        assert losses[0] > 0 and all(b < a for a, b in zip(losses, losses[1:])), losses
    finally:
        rend.close()
        scene.close()
