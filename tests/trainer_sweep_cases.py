"""The drawn cases of the trainer sweep (tests/test_gpu_trainer_sweep.py; tests/test_trainer_sweep_cases.py asserts on the CPU what
they cover).  The hand-built scenes of the last-frame passes -- contributions, feature_maps, lift_pixels, blend_backward,
project_backward, camera_backward, visible_mask, densify_stats, Scene.adam_step, densify -- are at most 72 x 64 and 1 500 Gaussians
under three cameras; here everything a case needs is drawn from np.random.default_rng(seed) alone: frames of 1 x 1 to 160 x 120 at
any pose within some 30 degrees of the default view and any field of view from 25 to 100 degrees, scenes of 1 to 900 Gaussians of
any splat size and opacity, and every mode switch a pass may meet.  WIDE is three further cases of 3 000 Gaussians at 256 x 144
(144 tiles).  A plain module: numpy only."""
import os

import numpy as np

SIZES = (1, 7, 63, 300, 900)
COEFFS = (0, 3, 8, 15)
CHANNELS = (1, 3, 4, 5, 15, 16, 17, 20)        # widths tests/test_gpu_feature_maps.py and tests/test_gpu_lift.py both run
MASKS = ("none", "half", "zero")
PRELOADS = (0.0, 1.5)
SWITCHES = ("sh16", "antialiased", "spatial", "one_pass", "tile_cull", "graph", "grad_alpha")
DEFAULT_SEEDS = 24
SEEDS = range(int(os.environ.get("GS_TRAINER_SWEEP_SEEDS", DEFAULT_SEEDS)))      # a soak: GS_TRAINER_SWEEP_SEEDS=200
WIDE_SIZE = (3000, 256, 144)


def _camera(rng):
    """As tests/test_gpu_fuzz.py draws it, a little closer in: within ~30 degrees of the default view, +-0.5 per axis, fov 25 .. 100."""
    q = rng.normal(size=4)
    q = q / np.linalg.norm(q) * 0.25 + np.array([1.0, 0, 0, 0])
    q /= np.linalg.norm(q)
    pos = rng.uniform(-0.5, 0.5, size=3)
    return tuple(float(v) for v in pos), tuple(float(v) for v in q), float(rng.uniform(25, 100))


def _draw(rng, name, seed, n=None, size=None):
    c = dict(name=name, seed=int(seed))
    drawn_n = int(rng.choice(SIZES))
    drawn_w, drawn_h = int(rng.integers(1, 161)), int(rng.integers(1, 121))
    c["n"] = drawn_n if n is None else n
    c["width"], c["height"] = (drawn_w, drawn_h) if size is None else size
    c["kind"] = str(rng.choice(["A", "T"]))
    c["log_scale_mean"] = float(rng.uniform(-4.5, -1.5))
    c["opacity_shift"] = float(rng.uniform(-3, 4))
    c["position"], c["rotation"], c["fov"] = _camera(rng)
    c["k"] = int(rng.choice(COEFFS))
    for switch in SWITCHES:
        c[switch] = bool(rng.integers(0, 2))
    c["exp_mode"] = int(rng.choice([2, 3]))
    c["in_flight"] = int(rng.choice([1, 3]))
    c["channels"] = int(rng.choice(CHANNELS))
    c["mask"] = str(rng.choice(MASKS))
    c["preload"] = float(rng.choice(PRELOADS))
    return c


def case(seed):
    """Everything one default case needs, from np.random.default_rng(seed) alone."""
    return _draw(np.random.default_rng(seed), f"seed {seed}", seed)


def _wide(i, **switches):
    """3 000 Gaussians at 256 x 144 under a drawn camera of its own; the switches are set, not drawn, so that the three differ."""
    c = _draw(np.random.default_rng(1000 + i), f"wide {i}", 1000 + i, n=WIDE_SIZE[0], size=WIDE_SIZE[1:])
    c["log_scale_mean"] = -3.5 + 0.2 * i          # (splats of a few pixels to a few tiles: the references stay near 10 s)
    c.update(switches)
    return c


WIDE = (_wide(0, kind="A", k=15, sh16=False, antialiased=False, spatial=True, one_pass=True, tile_cull=True, exp_mode=2, in_flight=1,
              graph=False, channels=5, mask="none", grad_alpha=True, preload=0.0),
        _wide(1, kind="T", k=3, sh16=True, antialiased=True, spatial=False, one_pass=False, tile_cull=False, exp_mode=3, in_flight=3,
              graph=True, channels=17, mask="half", grad_alpha=False, preload=1.5),
        _wide(2, kind="A", k=8, sh16=False, antialiased=True, spatial=True, one_pass=True, tile_cull=False, exp_mode=2, in_flight=3,
              graph=False, channels=3, mask="none", grad_alpha=True, preload=1.5))


def cases(seeds=None):
    """The sweep's list: the seeded cases, then WIDE."""
    return [case(s) for s in (SEEDS if seeds is None else seeds)] + list(WIDE)


def records(synth, c):
    """The (n, 62) PLY-domain records of a case: the synthetic scene of its kind and splat size, its opacity logits shifted, its SH
    coefficients beyond the case's K zero (what Scene.from_tensors makes of an sh_rest of K coefficients)."""
    rec = synth.synth_records(c["n"], seed=2000 + c["seed"], kind=c["kind"], log_scale_mean=c["log_scale_mean"])
    rec[:, 54] += np.float32(c["opacity_shift"])
    for ch in range(3):
        rec[:, 9 + 15 * ch + c["k"]:9 + 15 * (ch + 1)] = 0
    return rec


def camera(module, c):
    """The camera record of a case; module: the package (make_camera) or the oracle (default_camera)."""
    make = getattr(module, "make_camera", None) or module.default_camera
    return make(c["position"], c["rotation"], c["fov"])


def tiles_of(c):
    return ((c["width"] + 15) // 16) * ((c["height"] + 15) // 16)


def grads(c):
    """(grad_rgb (h, w, 3) float32, grad_alpha (h, w) float32 or None) of a case."""
    rng = np.random.default_rng(7000 + c["seed"])
    G = rng.standard_normal((c["height"], c["width"], 3)).astype(np.float32)
    ga = rng.standard_normal((c["height"], c["width"])).astype(np.float32)
    return G, (ga if c["grad_alpha"] else None)


def pixel_mask(c):
    """The (h, w) uint8 mask of contributions and lift_pixels: None, a random half (any nonzero value counts), or all zero."""
    if c["mask"] == "none":
        return None
    if c["mask"] == "zero":
        return np.zeros((c["height"], c["width"]), np.uint8)
    return (np.random.default_rng(8000 + c["seed"]).random((c["height"], c["width"])) < 0.5).astype(np.uint8) * 3


def gaussian_mask(c):
    """The (n,) uint8 mask of Scene.adam_step: None (every Gaussian), a random half, or all zero."""
    if c["mask"] == "none":
        return None
    if c["mask"] == "zero":
        return np.zeros(c["n"], np.uint8)
    return (np.random.default_rng(9000 + c["seed"]).random(c["n"]) < 0.5).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ ill-conditioned draws
def ill_conditioned(want):
    """The ONE exclusion of the sweep, for project_backward and camera_backward in antialiased frames: bool [n], true for a visible
    Gaussian whose det_raw = cov00 cov11 - cov01^2 -- the reference's binary64 value -- lies within rounding of zero by the
    reference's own error magnitude for that node, |det_raw| <= 2 k 2^-53 mag(det_raw) (k and mag as
    tests/project_backward_reference.py counts them; the factor 2 because the device's value and the reference's each lie within
    k 2^-53 mag of the exact one).  The sign of such a difference of rounding-sized products, and so whether comp is the constant
    0, is the association's to decide: the needle tests/test_backward_cameras_api.py leaves out by margin.  `want`:
    project_backward_reference.backward(..., antialiased=True); in a reference-mode frame nothing is excluded."""
    det, lim = want["det_raw"], want["det_raw_bound"]
    with np.errstate(invalid="ignore"):
        return np.asarray(want["visible"], bool) & (np.abs(det) <= 2.0 * lim)
