"""Both backward passes as one: parameters -> record -> image.  Two statements of it, compared by
tests/test_backward_cameras_api.py, so that the seam between the halves -- the order of the conic's three numbers, whether
d_conic[1] means b or 2b, the order of uv, whether d_opacity is taken before or after the antialiased factor -- is checked by
something other than the two halves called one after the other:

  composed()            tests/project_backward_reference.py fed with the sums of tests/backward_reference.py: the yardsticks of
                        gs_project_backward and gs_blend_backward, chained as Renderer.differentiable_render chains the kernels;
  composed_autograd()   one float64 torch function from the six parameter tensors to rgb and alpha -- the record function of
                        tests/record_function_torch.py feeding the dense blend of tests/test_blend_backward_api.py -- differentiated
                        by torch.autograd.  Every decision of the frame is a constant taken from the oracle's frame and the binary32
                        walk: visibility, the lists, which pairs are skipped, clamped or broken, the clamps' branches, red's flow.
                        The record entering the blend is rec32.detach() + (F - F.detach()): its VALUE is the oracle's binary32 record
                        exactly, so the gradient is evaluated at the frame's values, and it flows through F.

The antialiased frame on the CPU: the oracle has no such mode; as tests/test_gpu_antialiased.py establishes, the antialiased frame
of scene S is the plain frame of the scene S' whose opacities are the compensated ones.  antialiased_frame() builds S' from the
reference's own forward value (opacity * comp rounded to binary32) and lets the oracle render it."""
import numpy as np

import backward_reference as bref
import project_backward_reference as pref
import record_function_torch as rft

INS = tuple(pref.INPUTS)
NAMES = tuple(pref.OUTPUTS)
RENDER_SCENE = (200, 64, 48)        # synth_records(200, seed=9, kind="A") at 64 x 48


def antialiased_frame(oracle, verts, u):
    """(S' vertices, oracle.stages(S', u)): the plain frame that is the antialiased frame of `verts`."""
    plain = oracle.stages(verts, u)
    vis = plain["tiles"] != 0
    fields = pref.unpack_vertices(verts)
    fwd = pref.backward(*fields, u, vis, plain["attr"]["color_radii"][:, 0] > 0, antialiased=True)["record"]["opacity"][0][:, 0]
    prime = verts.copy()
    prime["scale_opacity"][vis, 3] = fwd[vis].astype(np.float32)
    ref = oracle.stages(prime, u)
    assert np.array_equal(ref["tiles"], plain["tiles"])
    return prime, ref


def frame(oracle, verts, u, antialiased):
    """oracle.stages of the frame the renderer draws of `verts` in either mode."""
    return antialiased_frame(oracle, verts, u)[1] if antialiased else oracle.stages(verts, u)


def _project(verts, u, ref, g, antialiased, sh16=False, k=15):
    return pref.backward(*pref.unpack_vertices(verts, sh16=sh16), u, ref["tiles"] != 0, ref["attr"]["color_radii"][:, 0] > 0,
                         colour=g["colour"], opacity_grad=g["opacity"], conic=g["conic"], uv=g["uv"], antialiased=antialiased,
                         sh_rest_coeffs=k)


def composed(oracle, verts, u, ref, G, ga, antialiased=False, binary64=False, sh16=False, k=15, bend=None):
    """The reference gradients of sum(G rgb) + sum(ga alpha) with respect to the six parameter groups.  verts: the scene's own
    vertices (S, not S'); ref: frame(...).  binary64: the blend's sums from the binary64 replay of the binary32 walk's decisions
    (the exact derivative of a smooth function: what autograd is compared with) instead of the definition's binary32 walk (what
    the device is compared with).  bend: a function applied to the blend's sums before they enter the projection (the teeth).
    Returns (want = the projection's reference with its A and bounds, spread = the projection's magnitudes of the blend's own
    bounds, per output, blend = the blend's reference)."""
    w, h = int(u["width"][0]), int(u["height"][0])
    blend = bref.backward(oracle, ref, w, h, G, ga)
    if binary64:
        blend = bref.backward(oracle, ref, w, h, G, ga, dtype=np.float64, replay=blend["pairs"])
    g = {name: blend[name] for name in INS}
    if bend is not None:
        g = bend(g)
    want = _project(verts, u, ref, g, antialiased, sh16, k)
    spread = _project(verts, u, ref, {name: bref.bound(blend, name) for name in INS}, antialiased, sh16, k)["A"]
    return want, spread, blend


def composed_autograd(verts, u, ref, pairs, G, ga, antialiased=False, k=15):
    """torch.autograd's gradients of the one float64 function, in the six outputs' shapes."""
    import torch
    from test_blend_backward_api import _dense_loss
    w, h = int(u["width"][0]), int(u["height"][0])
    attr, n = ref["attr"], len(ref["tiles"])
    f = rft.forward(verts, u, ref["tiles"] != 0, attr["color_radii"][:, 0] > 0, antialiased, False)
    idx = torch.as_tensor(f["idx"].astype(np.int64))

    def at_frame(rec32, F):
        """[N][c] float64: the binary32 record's value, F's gradient (rows of culled Gaussians: the record's, constant)."""
        base = torch.tensor(np.asarray(rec32, np.float64))
        delta = F - F.detach()
        return base.index_add(0, idx, delta.reshape((len(idx),) + tuple(base.shape[1:])))
    conic = at_frame(attr["conic_opacity"][:, :3], f["conic"])
    opac = at_frame(attr["conic_opacity"][:, 3], f["opacity"])
    uv = at_frame(attr["uv"][:, :2], f["uv"])
    col = at_frame(attr["color_radii"][:, :3], f["rgb"])
    ga = np.zeros((h, w), np.float32) if ga is None else ga
    _dense_loss(conic, opac, uv, col, ref, w, h, pairs, G, ga).backward()
    return rft.gradients(f, n, k)


# ------------------------------------------------------------------------------------------------ descent on geometry
GEOMETRY_RATES = (1e-2, 3e-3, 1e-3, 3e-4)
GEOMETRY_LR = 3e-3          # the largest of GEOMETRY_RATES for which reference_descent falls at every step (asserted on the CPU)
GEOMETRY_STEPS = 6
GEOMETRY_CAMERA = "C1"


def geometry_records(synth):
    """(records the descent starts from, records the target is rendered from): RENDER_SCENE, and the same with its means,
    log-scales and quaternions perturbed."""
    n = RENDER_SCENE[0]
    rec = synth.synth_records(n, seed=9, kind="A")
    rng = np.random.default_rng(37)
    target = rec.copy()
    target[:, 0:3] += 0.02 * rng.standard_normal((n, 3)).astype(np.float32)
    target[:, 55:58] += 0.15 * rng.standard_normal((n, 3)).astype(np.float32)
    target[:, 58:62] += 0.15 * rng.standard_normal((n, 4)).astype(np.float32)
    return rec, target


def reference_descent(pkg, oracle, lr, steps=GEOMETRY_STEPS):
    """The losses sum((rgb - target)^2) before each of `steps` Adam steps and after the last, on the CPU: the oracle's frame, the
    gradient of composed() with grad_rgb = 2 (rgb - target) rounded to float32 as differentiable_render returns it, torch's Adam on
    the float32 means, log-scales and quaternions."""
    import torch
    import backward_cameras as bc
    n, w, h = RENDER_SCENE
    rec, target_rec = geometry_records(pkg.synth)
    u = oracle.camera_uniforms(bc.camera(oracle, GEOMETRY_CAMERA), w, h)
    target = oracle.stages(oracle.activate_records(target_rec), u)["image"][..., :3].astype(np.float32)
    rec = rec.copy()
    params = {"means": torch.tensor(rec[:, 0:3].copy()), "log_scales": torch.tensor(rec[:, 55:58].copy()), "quats": torch.tensor(rec[:, 58:62].copy())}
    opt = torch.optim.Adam(list(params.values()), lr=lr)
    losses = []
    for step in range(steps + 1):
        rec[:, 0:3], rec[:, 55:58], rec[:, 58:62] = params["means"].numpy(), params["log_scales"].numpy(), params["quats"].numpy()
        verts = oracle.activate_records(rec)
        ref = oracle.stages(verts, u)
        diff = ref["image"][..., :3].astype(np.float32) - target
        losses.append(float((diff.astype(np.float32) ** 2).sum()))
        if step == steps:
            break
        want, _, _ = composed(oracle, verts, u, ref, (2.0 * diff).astype(np.float32), None, k=0)
        opt.zero_grad()
        for name, p in params.items():
            p.grad = torch.tensor(want[name].astype(np.float32))
        opt.step()
    return losses
