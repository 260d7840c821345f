"""The images gs_photometric_loss is tested on, shared by tests/test_gpu_photometric_loss.py (the device against the reference) and
tests/test_photometric_loss_api.py (the reference against torch.autograd, binary80 and its mutations): built once, never changed.
The sizes are the smallest at which a tiled windowed kernel can go wrong: below the window's radius, the kernel's tile of
TILE x TILE pixels exactly, one more in either axis, odd sizes, and 70 x 90 = 5 x 6 workgroups, whose partial-sum row has an
interior.  REDUCTION_SIZES is a second list, for the GPU tests and the partition model alone: the sizes at which the kernels' SUMS
change regime (a lane of k_loss_finish takes a second row, k_loss_l1 reaches its cap and strides), which the per-name CPU tests
(torch.autograd and binary80 on every entry of NAMES) have no reason to pay for."""
import numpy as np

TILE = 16   # kLossTile of gs_loss.hip
SIZES = ((1, 1), (1, 11), (5, 7), (6, 6), (11, 64), (TILE, TILE), (TILE + 1, TILE), (TILE, TILE + 1), (37, 53), (70, 90))   # (h, w)
THREADS = 256        # kLossThreads: lanes of a workgroup, and of the one workgroup of k_loss_finish
L1_GROUPS = 2048     # kLossL1Groups: the cap on k_loss_l1's grid
FINISH_UNROLL = 8    # k_loss_finish adds its rows under #pragma unroll 8
MAX_EXTENT = 16384   # GS_PHOTO_LOSS_MAX_EXTENT
REDUCTION_LAMBDA = 0.2
# (h, w, lambda).  lambda > 0: rows = ceil(h / TILE) * ceil(w / TILE) partial-sum rows, one per tile (ssim_rows).
# lambda = 0: E = 3 h w elements, rows = min(ceil(E / THREADS), L1_GROUPS) (l1_rows).  tests/test_photometric_loss_api.py asserts
# every comment below from the constants above.
REDUCTION_SIZES = (
    (16, 4112, REDUCTION_LAMBDA),     # 257 rows: one lane of the finish takes a second row
    (272, 272, REDUCTION_LAMBDA),     # 17 x 17 = 289 rows: many tiles in both axes
    (1, 16384, REDUCTION_LAMBDA),     # 1024 rows: the extent, all-padding rows above and below
    (16384, 1, REDUCTION_LAMBDA),     # 1024 rows: the same in the other axis, gridDim.y = 1024
    (368, 1424, REDUCTION_LAMBDA),    # 23 x 89 = 2047 rows: lanes take 7 or 8 rows
    (17, 16384, REDUCTION_LAMBDA),    # 2048 rows: exactly 8 per lane, the unrolled body alone
    (48, 10928, REDUCTION_LAMBDA),    # 3 x 683 = 2049 rows: one lane takes a 9th row
    (33, 16384, REDUCTION_LAMBDA),    # 3072 rows: 12 per lane, unrolled body plus remainder; the last tile row holds one image row
    (160, 160, 0.0),                  # E = 76 800: 300 rows, every workgroup full
    (161, 160, 0.0),                  # E = 77 280: 302 rows, the last workgroup partly idle
    (126, 1387, 0.0),                 # E = 524 286: 2048 workgroups, no lane strides, two lanes idle
    (183, 955, 0.0),                  # E = 524 295: seven lanes take a second element
    (350, 1249, 0.0),                 # E = 1 311 450: lanes take 2 or 3 elements
)
CONDITIONING = ("equal", "const_0.5_0.5", "const_0.2_0.7", "step_edge", "wide_range", "spike")
_cache = {}


def uniform(h, w, stride=3, seed=0, lo=0.0, hi=1.0):
    rng = np.random.default_rng([h, w, stride, seed])
    return rng.uniform(lo, hi, (h, w, stride)).astype(np.float32)


def ssim_rows(h, w):
    """(tiles down, tiles across) of the lambda > 0 path: their product is the number of partial-sum rows."""
    return -(-h // TILE), -(-w // TILE)


def l1_rows(h, w):
    """Workgroups of k_loss_l1 (lambda = 0): one per THREADS elements, capped."""
    return min(-(-3 * h * w // THREADS), L1_GROUPS)


def dyadic(h, w, seed):
    """(image, target) whose values are integer multiples of 2^-8 in [0, 1], as float32.  Every |x - y| is a multiple of 2^-8 and
    every (x - y)^2 of 2^-16, and up to the largest listed size 2^8 sum |x - y| and 2^16 sum (x - y)^2 stay below 2^53: the two sums
    are exact in binary64 in any order and any association, so l1 and mse are ONE correctly rounded division by n (dyadic_exact)."""
    rng = np.random.default_rng([h, w, 256, seed])
    k = rng.integers(0, 257, (2, h, w, 3))
    return tuple((k[i] / 256.0).astype(np.float32) for i in range(2))


def dyadic_exact(x, y):
    """(l1, mse) of a dyadic pair from integer arithmetic: the sums in int64, one correctly rounded division each (Python's
    int / int rounds the exact quotient once)."""
    kx, ky = (np.rint(np.asarray(a, np.float64)[..., :3] * 256).astype(np.int64) for a in (x, y))
    assert np.array_equal(kx / 256.0, np.asarray(x, np.float64)[..., :3]) and np.array_equal(ky / 256.0, np.asarray(y, np.float64)[..., :3])
    d = np.abs(kx - ky)
    n = 3 * d.shape[0] * d.shape[1]
    return int(d.sum()) / (256 * n), int((d * d).sum()) / (65536 * n)


def _build(name):
    if name.startswith("uniform_"):
        h, w = (int(v) for v in name[len("uniform_"):].split("x"))
        return uniform(h, w, seed=1), uniform(h, w, seed=2)
    if name.startswith("dyadic_"):
        h, w = (int(v) for v in name[len("dyadic_"):].split("x"))
        return dyadic(h, w, seed=1)
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
