"""gs_scene_adam_step restated in numpy: the yardstick of tests/test_adam_step_api.py (CPU) and tests/test_gpu_adam_step.py.

The function, as include/gs3d_hip.h writes it -- binary64 on exact conversions of the stored binary32 values, every operation
rounded on its own, in exactly this order:

    m' = (beta1 * m) + ((1 - beta1) * g)              (1 - beta1) and (1 - beta2) formed once, in binary64
    v' = (beta2 * v) + (((1 - beta2) * g) * g)
    d  = (sqrt(v') / sqrt(bias_correction2)) + eps    sqrt(bias_correction2) formed once
    p' = p - ((lr / bias_correction1) * (m' / d))     lr / bias_correction1 formed once, per group
    exp_avg <- fl32(m')    exp_avg_sq <- fl32(v')    param <- fl32(p')

numpy's float64 +, -, *, / and sqrt are IEEE operations, one rounding each, and it never fuses two of them: the arrays below ARE
the contract's bits.  The three roundings at the stores are .astype(np.float32) (`store`; np.float64 keeps the stores in binary64
for the comparison with torch.optim.Adam).  Only the rows of the mask are read or written.

The activation of the new parameters is not restated: it is the host path's (gs_activate_records), which the device-array ingest is
pinned to bit for bit (tests/test_gpu_device_arrays.py)."""
import numpy as np

NAMES = ("means", "log_scales", "quats", "opacity_logits", "sh_dc", "sh_rest")
COLUMNS = dict(means=slice(0, 3), sh_dc=slice(6, 9), sh_rest=slice(9, 54), opacity_logits=slice(54, 55), log_scales=slice(55, 58),
               quats=slice(58, 62))
WIDTH = dict(means=3, log_scales=3, quats=4, opacity_logits=1, sh_dc=3)
BETAS, EPS = (0.9, 0.999), 1e-15          # the defaults of the package's Adam


def bias_corrections(betas, t):
    """(1 - beta1^t, 1 - beta2^t) as Scene.adam_step forms them: Python floats."""
    return 1.0 - float(betas[0]) ** int(t), 1.0 - float(betas[1]) ** int(t)


def step(params, grads, exp_avg, exp_avg_sq, lr, betas=BETAS, eps=EPS, t=1, mask=None, zero_grads=True, store=np.float32):
    """One step IN PLACE on dicts of numpy arrays under NAMES (a name params lacks is not stepped): params and the moments of dtype
    `store`, grads float64, one row per Gaussian.  lr: a float or a dict per name.  mask: (n,) nonzero = step, None = every row."""
    beta1, beta2 = np.float64(betas[0]), np.float64(betas[1])
    bc1, bc2 = bias_corrections(betas, t)
    one_minus_beta1, one_minus_beta2 = np.float64(1.0) - beta1, np.float64(1.0) - beta2
    root_bc2 = np.sqrt(np.float64(bc2))
    eps = np.float64(eps)
    rows = slice(None) if mask is None else (np.asarray(mask) != 0)
    with np.errstate(all="ignore"):
        for name, p in params.items():
            assert p.dtype == store and exp_avg[name].dtype == store and exp_avg_sq[name].dtype == store and grads[name].dtype == np.float64
            size = np.float64(lr[name] if isinstance(lr, dict) else lr) / np.float64(bc1)
            g = grads[name][rows]
            m = (beta1 * exp_avg[name][rows].astype(np.float64)) + (one_minus_beta1 * g)
            v = (beta2 * exp_avg_sq[name][rows].astype(np.float64)) + ((one_minus_beta2 * g) * g)
            d = (np.sqrt(v) / root_bc2) + eps
            new = p[rows].astype(np.float64) - (size * (m / d))
            exp_avg[name][rows] = m.astype(store)
            exp_avg_sq[name][rows] = v.astype(store)
            p[rows] = new.astype(store)
            if zero_grads:
                grads[name][rows] = 0.0


def cut(records, k=15):
    """The six float32 arrays of (n, 62) PLY-domain records as a trainer holds them, sh_rest with its first k coefficients."""
    r = np.ascontiguousarray(records, np.float32)
    n = len(r)
    a = dict(means=r[:, 0:3], log_scales=r[:, 55:58], quats=r[:, 58:62], opacity_logits=r[:, 54], sh_dc=r[:, 6:9],
             sh_rest=r[:, 9:54].reshape(n, 3, 15).transpose(0, 2, 1)[:, :k, :])
    return {name: np.array(v, np.float32, order="C") for name, v in a.items()}


def records_of(params, base):
    """`base` (n, 62) with the columns of the groups in `params` replaced; SH coefficients beyond sh_rest's k keep base's."""
    r = np.array(base, np.float32, copy=True)
    n = len(r)
    for name, v in params.items():
        v = np.asarray(v, np.float32)
        if name == "sh_rest":
            planar = r[:, 9:54].reshape(n, 3, 15).copy()
            planar[:, :, :v.shape[1]] = v.transpose(0, 2, 1)
            r[:, 9:54] = planar.reshape(n, 45)
        else:
            r[:, COLUMNS[name]] = v.reshape(n, -1)
    return r


def vertices_of(pkg, params, base):
    """The (n, 60) vertices the scene holds after a step: the host path's activation of records_of(params, base)."""
    with np.errstate(all="ignore"):
        return pkg.activate_records(records_of(params, base))


def zeros_like(params, dtype):
    return {name: np.zeros(v.shape, dtype) for name, v in params.items()}


def random_gradients(params, seed, mask=None):
    """float64 gradients with the values a step must not trip over sprinkled in: exact zeros, denormals, 1e+30 and 1e-30."""
    rng = np.random.default_rng(seed)
    special = np.array([0.0, -0.0, 5e-324, -3e-310, 1e30, -1e30, 1e-30, -1e-30])
    out = {}
    for name, v in params.items():
        g = rng.standard_normal(v.shape) * 10.0 ** rng.integers(-6, 3, v.shape)
        pick = rng.random(v.shape) < 0.15
        g[pick] = special[rng.integers(0, len(special), int(pick.sum()))]
        out[name] = g
    return out


# ------------------------------------------------------------------------------------------------ descent on geometry, sparse
# The loop of tests/composed_reference.py: reference_descent with THIS module's step, under each frame's visibility, in place of
# torch's Adam.  The rate is composed_reference.GEOMETRY_LR if the loss falls at every step there (tests/test_adam_step_api.py
# asserts the choice on the CPU; tests/test_gpu_adam_step.py uses it).  The CPU run's seven losses at that rate are written beside it.
GEOMETRY_LR = 3e-3        # = composed_reference.GEOMETRY_LR: the sparse step falls at every step there too; its seven CPU losses:
GEOMETRY_LOSSES = (17.4541, 14.0704, 11.2633, 9.0736, 7.38947, 6.14226, 5.25778)   # (at 1e-2: ... 4.67932 -> 4.75464, a rise)
GEOMETRY_GROUPS = ("means", "log_scales", "quats")


def sparse_descent(pkg, oracle, lr, steps=None):
    """The losses sum((rgb - target)^2) before each Adam step and after the last, on the CPU: the oracle's frame, the gradient of
    composed() with grad_rgb = 2 (rgb - target) in float32, this module's step on the float32 means, log-scales and quaternions of
    the Gaussians that frame saw."""
    import backward_cameras as bc
    import composed_reference as comp
    steps = comp.GEOMETRY_STEPS if steps is None else steps
    n, w, h = comp.RENDER_SCENE
    rec, target_rec = comp.geometry_records(pkg.synth)
    u = oracle.camera_uniforms(bc.camera(oracle, comp.GEOMETRY_CAMERA), w, h)
    target = oracle.stages(oracle.activate_records(target_rec), u)["image"][..., :3].astype(np.float32)
    params = {name: v for name, v in cut(rec).items() if name in GEOMETRY_GROUPS}
    m, v = zeros_like(params, np.float32), zeros_like(params, np.float32)
    losses = []
    for t in range(steps + 1):
        verts = oracle.activate_records(records_of(params, rec))
        ref = oracle.stages(verts, u)
        diff = ref["image"][..., :3].astype(np.float32) - target
        losses.append(float((diff.astype(np.float32) ** 2).sum()))
        if t == steps:
            break
        want, _, _ = comp.composed(oracle, verts, u, ref, (2.0 * diff).astype(np.float32), None, k=0)
        grads = {name: np.array(want[name], np.float64) for name in params}
        step(params, grads, m, v, lr, t=t + 1, mask=ref["tiles"] != 0)
    return losses
