"""Named edge scenes for the float64 check (tests/float64_check.py): each is built so that ONE of the shaders' rules decides
an output many times -- the near cull, the Jacobian's frustum clamp, the eigenvalue floor, the alpha clamp and the T cut,
SH in every band under every orientation, needles, extreme frames, saturating boxes, equal-depth ties.

A case is a list of Frames (records, camera, W x H) plus the rule perturbations it is named after (`mutations`), each with
the least number of Gaussians / list entries / pixels that the float64 reference must decide differently under it: a case cannot quietly stop testing what it is named after.  A plain module (not a conftest): the CPU test
and the GPU test import it; it needs numpy and tests/ only."""
from dataclasses import dataclass

import numpy as np

import np_reference as npr

RECORD_FLOATS = 62


@dataclass
class Frame:
    label: str
    records: np.ndarray            # (n, 62) float32 PLY records
    position: tuple = (0.0, 0.0, 0.0)
    rotation: tuple = (1.0, 0.0, 0.0, 0.0)
    fov: float = 45.0
    width: int = 320
    height: int = 180
    sh16: bool = False             # compare against the coefficients rounded to binary16 (Scene.quantize_sh)
    max_explained: int = 0         # cap on image pixels explained by a decision within rounding (not by the continuous bound)

    def camera64(self):
        """The float64 camera of the binary32 camera the pipeline receives."""
        pos = tuple(float(np.float32(v)) for v in self.position)
        q = tuple(float(np.float32(v)) for v in self.rotation)
        return npr.camera(pos, q, float(np.float32(self.fov)), float(np.float32(0.1)), float(np.float32(1000.0)),
                          self.width, self.height)


@dataclass
class Case:
    name: str
    frames: list
    mutations: list                # [(rule perturbation this case is built to expose, its least exercise count), ...]


def _records(n, rng, sh_rest=0.1, logit=(-1.0, 3.0)):
    rec = np.zeros((n, RECORD_FLOATS), np.float32)
    rec[:, 6:9] = rng.uniform(-1.5, 1.5, (n, 3))
    rec[:, 9:54] = sh_rest * rng.normal(size=(n, 45))
    rec[:, 54] = rng.uniform(*logit, n)
    rec[:, 58] = 1.0
    return rec


def _tan(fov):
    return np.tan(np.radians(float(np.float32(fov))) / 2.0)


def _place(rec, ndc_x, ndc_y, tz, fov, w, h):
    """Positions (identity camera at the origin) whose view depth is tz and whose NDC is (ndc_x, ndc_y)."""
    tx = _tan(fov)
    ty = tx * h / w
    rec[:, 0] = ndc_x * tz * tx
    rec[:, 1] = -ndc_y * tz * ty
    rec[:, 2] = -tz


def _ndc(uv, size):
    return (2.0 * uv + 1.0) / size - 1.0


def _quat_axis(axis, deg):
    a = np.radians(deg) / 2.0
    v = np.asarray(axis, np.float64)
    v = v / np.linalg.norm(v)
    return (float(np.cos(a)), *(float(np.sin(a)) * v))


def _quat_mul(p, q):
    w1, x1, y1, z1 = p
    w2, x2, y2, z2 = q
    return (w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
            w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2)


def near_plane():
    """View depths straddling the near cut 0.2: a band 0.195 .. 0.205, and the binary32 neighbours of 0.2f (+-1..4 ULP)."""
    rng = np.random.default_rng(101)
    w, h, fov, n = 320, 180, 45.0, 3000
    rec = _records(n, rng)
    tz = rng.uniform(0.195, 0.205, n)
    ulps = np.arange(-4, 5)
    tz[:len(ulps) * 20] = np.repeat(np.float32(0.2).view(np.int32) + ulps, 20).astype(np.int32).view(np.float32)
    _place(rec, rng.uniform(-0.9, 0.9, n), rng.uniform(-0.9, 0.9, n), tz, fov, w, h)
    rec[:, 2] = -tz.astype(np.float32)
    rec[:, 55:58] = np.log(rng.uniform(0.0004, 0.002, (n, 1))) + rng.normal(0, 0.2, (n, 3))
    rec[:, 58:62] = rng.normal(size=(n, 4))
    return Case("near_plane", [Frame("near_plane", rec, fov=fov, width=w, height=h, max_explained=4)],
                mutations=[(dict(near=0.202), 20000)])


def frustum_clamp():
    """Centres beyond 1.3 tan(fov/2) on both axes and both signs, large enough that their footprints reach the screen."""
    rng = np.random.default_rng(102)
    w, h, fov, n = 320, 180, 60.0, 1600
    rec = _records(n, rng, logit=(-2.0, 1.0))
    tz = rng.uniform(1.0, 3.0, n)
    lim = 1.3
    r = rng.uniform(lim + 0.02, 1.7, n) * rng.choice([-1.0, 1.0], n)
    other = rng.uniform(-1.0, 1.0, n)
    xaxis = np.arange(n) % 2 == 0
    _place(rec, np.where(xaxis, r, other), np.where(xaxis, other, r), tz, fov, w, h)
    rec[:, 55:58] = np.log(tz[:, None] * rng.uniform(0.08, 0.2, (n, 1))) + rng.normal(0, 0.3, (n, 3))
    rec[:, 58:62] = rng.normal(size=(n, 4))
    return Case("frustum_clamp", [Frame("frustum_clamp", rec, fov=fov, width=w, height=h, max_explained=4)],
                mutations=[(dict(frustum=1.28), 20000)])


def radius_floor():
    """Small isotropic splats, so mid^2 - det ~ 0 < 0.1 and the floor sets lambda = mid + sqrt(0.1); sized so that
    3 sqrt(lambda) lies 0.01 below an integer (half of them) or 0.01 above one (the other half), and placed so that
    uv + r sits half a pixel past a tile border: a change of the floor or of the factor 3 moves the radius AND the box."""
    rng = np.random.default_rng(103)
    w, h, fov, n = 320, 176, 45.0, 2000
    rec = _records(n, rng)
    r = rng.integers(3, 7, n).astype(np.float64)                   # the radius: 3 .. 6
    below = np.arange(n) % 2 == 0
    target = np.where(below, r - 0.01, r - 1.0 + 0.01)              # 3 sqrt(lambda)
    tiles_x, tiles_y = rng.integers(1, w // 16, n), rng.integers(1, h // 16, n)
    uvx = 16.0 * tiles_x + 0.5 - r
    uvy = 16.0 * tiles_y - 8.0 + rng.uniform(-4, 4, n)
    tz = rng.uniform(2.0, 5.0, n)
    _place(rec, _ndc(uvx, w), _ndc(uvy, h), tz, fov, w, h)
    frame = Frame("radius_floor", rec, fov=fov, width=w, height=h, max_explained=4)
    cam = frame.camera64()
    lo, hi = np.full(n, -12.0), np.full(n, 0.0)                     # bisection on the log-scale for the target
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        rec[:, 55:58] = mid[:, None]
        pre = npr.preprocess(npr.activate(rec), cam)
        v = 3.0 * np.sqrt(pre["lam"])
        lo, hi = np.where(v < target, mid, lo), np.where(v < target, hi, mid)
    rec[:, 55:58] = (0.5 * (lo + hi))[:, None]
    return Case("radius_floor", [frame], mutations=[(dict(floor=0.12), 2000)])


def opaque_cores():
    """Dense stacks of nearly opaque splats (logit 5 .. 8: opacity 0.993 .. 0.9997): alpha is clamped at 0.99 around every
    centre and the transmittance falls through 1e-4 within a few entries."""
    rng = np.random.default_rng(104)
    w, h, fov = 320, 180, 45.0
    stacks, depth = 150, 12
    n = stacks * depth
    rec = _records(n, rng, logit=(5.0, 8.0))
    cx, cy = np.repeat(rng.uniform(-0.9, 0.9, stacks), depth), np.repeat(rng.uniform(-0.9, 0.9, stacks), depth)
    tz = rng.uniform(2.0, 6.0, n)
    _place(rec, cx + rng.normal(0, 0.01, n), cy + rng.normal(0, 0.01, n), tz, fov, w, h)
    rec[:, 55:58] = np.log(tz[:, None] * rng.uniform(0.006, 0.03, (n, 1))) + rng.normal(0, 0.2, (n, 3))
    rec[:, 58:62] = rng.normal(size=(n, 4))
    return Case("opaque_cores", [Frame("opaque_cores", rec, fov=fov, width=w, height=h, max_explained=8)],
                mutations=[(dict(alpha_max=0.995), 300)])


VIEW_SPHERE_POS = (0.1, 0.2, -0.3)


def _view_sphere_records(n, rng):
    rec = _records(n, rng, sh_rest=0.6)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rec[:, 0:3] = np.asarray(VIEW_SPHERE_POS) + d * rng.uniform(2.0, 4.0, (n, 1))
    rec[:, 6:9] = rng.normal(0.0, 1.0, (n, 3))
    rec[:, 55:58] = np.log(rng.uniform(0.01, 0.05, (n, 1))) + rng.normal(0, 0.3, (n, 3))
    rec[:, 58:62] = rng.normal(size=(n, 4))
    return rec


def view_sphere(sh16=False):
    """A shell around the camera with strong SH in every band (coefficients ~ N(0, 0.6), many colours negative in every
    channel), seen from seven orientations: forward, yawed 90/180/270, pitched +-90, and upside down (rolled 180)."""
    rng = np.random.default_rng(105)
    rec = _view_sphere_records(4000, rng)
    poses = {"forward": (1.0, 0.0, 0.0, 0.0), "yaw90": _quat_axis((0, 1, 0), 90), "yaw180": _quat_axis((0, 1, 0), 180),
             "yaw270": _quat_axis((0, 1, 0), 270), "pitch+90": _quat_axis((1, 0, 0), 90),
             "pitch-90": _quat_axis((1, 0, 0), -90),
             "upside_down": _quat_mul(_quat_axis((0, 1, 0), 30), _quat_axis((0, 0, 1), 180))}
    frames = [Frame(f"view_sphere/{k}", rec, position=VIEW_SPHERE_POS, rotation=q, fov=70.0, width=240, height=160,
                    sh16=sh16, max_explained=4) for k, q in poses.items()]
    return Case("view_sphere", frames, mutations=[(dict(clamp_channels=(0, 1, 2)), 50000)])


def needles():
    """Anisotropy 10^3 .. 10^4, random orientations: near-singular 2D covariances and a `power` of cancelling terms."""
    rng = np.random.default_rng(106)
    w, h, fov, n = 320, 180, 45.0, 1500
    rec = _records(n, rng, logit=(0.0, 4.0))
    tz = rng.uniform(2.0, 6.0, n)
    _place(rec, rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n), tz, fov, w, h)
    long_ = np.log(rng.uniform(0.1, 0.6, n))
    ratio = np.log(rng.uniform(1e3, 1e4, n))
    rec[:, 55] = long_
    rec[:, 56] = long_ - ratio
    rec[:, 57] = long_ - ratio + rng.normal(0, 0.3, n)
    rec[:, 58:62] = rng.normal(size=(n, 4))
    return Case("needles", [Frame("needles", rec, fov=fov, width=w, height=h, max_explained=12)],
                mutations=[(dict(dilation=0.29), 20000)])


def extreme_frames():
    """fov 5 and 150 degrees, a 3 x 900 and a 1500 x 5 frame; no size a multiple of 16."""
    frames = []
    for k, (fov, w, h) in enumerate([(5.0, 250, 130), (150.0, 250, 130), (45.0, 3, 900), (45.0, 1500, 5)]):
        rng = np.random.default_rng(107 + k)
        n = 2500
        rec = _records(n, rng)
        tz = rng.uniform(1.0, 8.0, n)
        _place(rec, rng.uniform(-1.2, 1.2, n), rng.uniform(-1.2, 1.2, n), tz, fov, w, h)
        px = 2.0 * _tan(fov) * tz / w                             # world size of a pixel at that depth
        rec[:, 55:58] = np.log(px[:, None] * rng.uniform(0.5, 8.0, (n, 1))) + rng.normal(0, 0.3, (n, 3))
        rec[:, 58:62] = rng.normal(size=(n, 4))
        frames.append(Frame(f"extreme/fov{fov:g}_{w}x{h}", rec, fov=fov, width=w, height=h, max_explained=4))
    return Case("extreme_frames", frames, mutations=[(dict(uv_offset=0.0), 30000)])


def huge_and_saturating():
    """Four sets, at the limits of the tile box's float -> int conversion (preprocess.comp:161-164 converts
    (uv -+ r [+ 15]) / 16; GLSL leaves int() of a value beyond int32 undefined, the pipeline saturates):
      * covering: splats far larger than the frame, nearly transparent;
      * huge: radius 4e9 .. 6e9 pixels (uv -+ r beyond 2^31) -- the converted arguments stay below 2^31, so these test the
        clamp to the grid, not saturation.  Arguments beyond 2^31 on BOTH sides of one axis would need r > 2^35 = 3.4e10,
        i.e. lambda > 1.3e20, where det = a c - b^2 overflows binary32: not a frame the pipeline can compute;
      * straddling: uv ~ 2^35 with r = 2e8: (uv - r) / 16 < 2^31 < (uv + r + 15) / 16 -- x0 converts to a value beyond the
        grid (clamped to its width), x1 saturates to INT32_MAX and clamps there too: an empty box.  A wrapping (or INT_MIN)
        conversion gives x1 = 0 < x0, whose uint32 tile count is not 0: the Gaussian would be kept;
      * far: centred 10^10 .. 10^11 pixels off screen, both arguments beyond 2^31 on one side: an empty box.
    The nearly transparent ones sit just above the alpha cut 1/255 (opacity 0.00393), so it decides every pixel they cover."""
    rng = np.random.default_rng(110)
    w, h, fov = 320, 180, 45.0
    sizes = dict(covering=24, huge=40, straddling=40, far=40)
    n = sum(sizes.values())
    edges = np.cumsum([0] + list(sizes.values()))
    c, s, t, f = (slice(edges[k], edges[k + 1]) for k in range(4))
    rec = _records(n, rng)
    tz = rng.uniform(1.0, 3.0, n)
    ndc_x, ndc_y = rng.uniform(-0.8, 0.8, n), rng.uniform(-0.8, 0.8, n)
    r_t = 2e8
    ndc_x[t] = _ndc(2.0 ** 35 + rng.uniform(-0.4, 0.4, sizes["straddling"]) * r_t, w)
    ndc_x[f] = rng.choice([-1.0, 1.0], sizes["far"]) * rng.uniform(1e8, 1e9, sizes["far"])
    _place(rec, ndc_x, ndc_y, tz, fov, w, h)
    rec[:, 58:62] = rng.normal(size=(n, 4))
    rec[c, 55:58] = np.log(tz[c, None] * rng.uniform(0.5, 3.0, (sizes["covering"], 1))) + rng.normal(0, 0.3, (sizes["covering"], 3))
    rec[c, 54] = rng.uniform(-3.0, -1.0, sizes["covering"])
    rec[s, 58:62] = (1.0, 0.0, 0.0, 0.0)
    # short of lambda ~ 1e19, where det = a c - b^2 overflows binary32
    rec[s, 55:58] = np.log(tz[s, None] * rng.uniform(3.2e6, 5.0e6, (sizes["huge"], 1)))
    rec[s, 54] = np.log(0.00393 / (1.0 - 0.00393))
    rec[t, 58:62] = (1.0, 0.0, 0.0, 0.0)
    focal = w / (2.0 * _tan(fov))
    rec[t, 55:58] = np.log(r_t / 3.0 * tz[t] / focal / 1.3)[:, None]   # 1.3: the frustum clamp's share of the Jacobian
    rec[f, 55:58] = np.log(rng.uniform(0.01, 0.1, (sizes["far"], 1)))
    return Case("huge_and_saturating", [Frame("huge_and_saturating", rec, fov=fov, width=w, height=h, max_explained=4)],
                mutations=[(dict(alpha_min=1.0 / 254.0), 20000), (dict(f2i="wrap"), 40)])


def depth_ties():
    """Groups of ten Gaussians at bit-identical view depth (identity camera: p_view.z = -z exactly), overlapping in the same
    tiles: the lists must hold each group in id order, and the ids of a group are interleaved with other groups'."""
    rng = np.random.default_rng(111)
    w, h, fov = 320, 180, 45.0
    groups, size = 300, 10
    n = groups * size
    rec = _records(n, rng)
    g = rng.permutation(np.arange(n) % groups)                      # group of each id: a group's ids are scattered
    tz = rng.uniform(2.0, 6.0, groups).astype(np.float32)[g]
    cx, cy = rng.uniform(-0.9, 0.9, groups)[g], rng.uniform(-0.9, 0.9, groups)[g]
    _place(rec, cx + rng.normal(0, 0.03, n), cy + rng.normal(0, 0.03, n), tz.astype(np.float64), fov, w, h)
    rec[:, 2] = -tz
    rec[:, 55:58] = np.log(tz[:, None] * rng.uniform(0.005, 0.02, (n, 1))) + rng.normal(0, 0.2, (n, 3))
    rec[:, 58:62] = rng.normal(size=(n, 4))
    return Case("depth_ties", [Frame("depth_ties", rec, fov=fov, width=w, height=h, max_explained=4)],
                mutations=[(dict(tie=-1), 30000)])


CASES = {f.__name__: f for f in (near_plane, frustum_clamp, radius_floor, opaque_cores, view_sphere, needles,
                                 extreme_frames, huge_and_saturating, depth_ties)}


def build(name):
    return CASES[name]()
