"""The images gs_photometric_loss is tested on, shared by tests/test_gpu_photometric_loss.py (the device against the reference) and
tests/test_photometric_loss_api.py (the reference against torch.autograd, binary80 and its mutations): built once, never changed.
The sizes are the smallest at which a tiled windowed kernel can go wrong: below the window's radius, the kernel's tile of
TILE x TILE pixels exactly, one more in either axis, odd sizes, and 70 x 90 = 5 x 6 workgroups, whose partial-sum row has an
interior."""
import numpy as np

TILE = 16   # kLossTile of gs_loss.hip
SIZES = ((1, 1), (1, 11), (5, 7), (6, 6), (11, 64), (TILE, TILE), (TILE + 1, TILE), (TILE, TILE + 1), (37, 53), (70, 90))   # (h, w)
CONDITIONING = ("equal", "const_0.5_0.5", "const_0.2_0.7", "step_edge", "wide_range", "spike")
_cache = {}


def uniform(h, w, stride=3, seed=0, lo=0.0, hi=1.0):
    rng = np.random.default_rng([h, w, stride, seed])
    return rng.uniform(lo, hi, (h, w, stride)).astype(np.float32)


def _build(name):
    if name.startswith("uniform_"):
        h, w = (int(v) for v in name[len("uniform_"):].split("x"))
        return uniform(h, w, seed=1), uniform(h, w, seed=2)
    h, w = 37, 53
    if name == "equal":
        x = uniform(h, w, seed=3)
        return x, x.copy()
    if name.startswith("const_"):
        a, b = (float(v) for v in name[len("const_"):].split("_"))
        return np.full((h, w, 3), a, np.float32), np.full((h, w, 3), b, np.float32)
    if name == "step_edge":      # the image's edge two pixels beside the target's, flat on both sides
        x, y = np.zeros((h, w, 3), np.float32), np.full((h, w, 3), 0.1, np.float32)
        x[:, 28:], y[:, 26:] = 1.0, 0.9
        return x, y
    if name == "wide_range":
        return uniform(h, w, seed=4, lo=-0.5, hi=2.0), uniform(h, w, seed=5)
    if name == "spike":
        x, y = uniform(h, w, seed=6), uniform(h, w, seed=7)
        x[20, 31, 1] = 1e4
        return x, y
    raise KeyError(name)


NAMES = tuple(f"uniform_{h}x{w}" for h, w in SIZES) + CONDITIONING


def images(name):
    """(image, target): float32 [H][W][3], read-only."""
    if name not in _cache:
        x, y = _build(name)
        x.setflags(write=False), y.setflags(write=False)
        _cache[name] = (x, y)
    return _cache[name]


def widen(a, fill):
    """[H][W][3] as the first three floats of a [H][W][4] image whose fourth float is `fill`."""
    out = np.full(a.shape[:2] + (4,), fill, np.float32)
    out[..., :3] = a
    return out
