"""The export's inverse activation restated in numpy (gs_host_math.h: export_log_scale / export_opacity_logit /
deactivate_vertex; gs_scene.hip: k_scene_export): what tests/test_scene_export_api.py holds the host function to and,
through it, tests/test_gpu_scene_export.py the kernel.

binary64 elementwise numpy operations are IEEE, one rounding each and never fused, so the order written here is the order the
C++ states.  The activation inside the polish is NOT restated: it is the library's own gs_activate_records, which is older
than the export and pinned to the reference (tests/test_host_math_vs_ref.py).  Neighbours are taken with np.nextafter.
"""
import numpy as np

SQRT_HALF = float.fromhex("0x1.6a09e667f3bcdp-1")
LN2 = float.fromhex("0x1.62e42fefa39efp-1")
ORDER = (0, -1, +1, -2, +2, -3, +3, -4, +4)
ROTATION_BOUND = 8.0 * 2.0 ** -24  # |q' - q| <= ROTATION_BOUND |q| per component after a reload (test_scene_export_api.py derives it)


def log64(v):
    """log of positive, finite, normal binary64 values."""
    v = np.asarray(v, np.float64)
    m, e = np.frexp(v)  # m in [1/2, 1)
    small = m < SQRT_HALF
    m = np.where(small, 2.0 * m, m)
    e = np.where(small, e - 1, e)
    t = (m - 1.0) / (m + 1.0)
    w = t * t
    p = np.full_like(t, 1.0 / 17.0)
    for k in (15.0, 13.0, 11.0, 9.0, 7.0, 5.0, 3.0):
        p = p * w + 1.0 / k
    p = p * w + 1.0
    return e.astype(np.float64) * LN2 + (2.0 * t) * p


def neighbour(x, d):
    """The binary32 value |d| steps above (d > 0) or below x, as nextafter steps."""
    x = np.asarray(x, np.float32).copy()
    toward = np.float32(np.inf if d > 0 else -np.inf)
    for _ in range(abs(d)):
        x = np.nextafter(x, toward)
    return x


def _activated(pkg, column, slot, x):
    """Column `slot` of gs_activate_records of records whose column `column` is x."""
    r = np.zeros((len(x), 62), np.float32)
    r[:, 58] = 1.0
    r[:, column] = x
    with np.errstate(all="ignore"):
        return pkg.activate_records(r)[:, slot]


def polish(pkg, x0, stored, column, slot):
    x0 = np.asarray(x0, np.float32)
    best, best_err = x0.copy(), np.full(len(x0), np.inf)
    for d in ORDER:
        c = neighbour(x0, d)
        ok = np.isfinite(c)
        act = _activated(pkg, column, slot, np.where(ok, c, np.float32(0)))
        with np.errstate(all="ignore"):
            err = np.abs(act.astype(np.float64) - stored.astype(np.float64))
            take = ok & (err < best_err)  # strictly smaller: the first in ORDER keeps a tie; a NaN never compares smaller
        best, best_err = np.where(take, c, best), np.where(take, err, best_err)
    return best.astype(np.float32)


def log_scales(pkg, s):
    s = np.asarray(s, np.float32)
    out = np.full(s.shape, np.nan, np.float32)
    out[s == 0] = -np.inf
    out[s == np.inf] = np.inf
    with np.errstate(invalid="ignore"):
        reg = (s > 0) & np.isfinite(s)
    if reg.any():
        x0 = log64(s[reg].astype(np.float64)).astype(np.float32)
        out[reg] = polish(pkg, x0, s[reg], 55, 4)
    return out


def opacity_logits(pkg, o):
    o = np.asarray(o, np.float32)
    out = np.full(o.shape, np.nan, np.float32)
    out[o == 0] = -np.inf
    out[o == 1] = np.inf
    with np.errstate(invalid="ignore"):
        reg = (o > 0) & (o < 1)
    if reg.any():
        od = o[reg].astype(np.float64)
        x0 = log64(od / (1.0 - od)).astype(np.float32)
        out[reg] = polish(pkg, x0, o[reg], 54, 7)
    return out


def deactivate(pkg, vertices):
    """(n, 60) activated vertices -> (n, 62) PLY records."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 60)
    n = len(v)
    r = np.zeros((n, 62), np.float32)
    r[:, 0:3] = v[:, 0:3]
    sh = v[:, 12:60].reshape(n, 16, 3)
    r[:, 6:9] = sh[:, 0, :]
    r[:, 9:54] = sh[:, 1:, :].transpose(0, 2, 1).reshape(n, 45)  # interleaved RGB per coefficient -> 15 R, 15 G, 15 B
    r[:, 54] = opacity_logits(pkg, v[:, 7])
    r[:, 55:58] = log_scales(pkg, v[:, 4:7].reshape(-1)).reshape(n, 3)
    r[:, 58:62] = v[:, 8:12]
    return r


def same_bits(got, want, label):
    """Bitwise equal wherever `want` is not a NaN, a NaN where it is."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.isnan(got[nan]).all(), f"{label}: a NaN of the reference is a number here"
    bad = np.argwhere((got.view(np.uint32) != want.view(np.uint32)) & ~nan)
    assert len(bad) == 0, (f"{label}: {len(bad)} value(s) differ in their bits, first at {tuple(bad[0])}: "
                           f"{got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}")


def rotations_within_bound(got, want, label):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    worst = np.abs(got - want) - ROTATION_BOUND * np.abs(want)
    assert (worst <= 0).all(), f"{label}: a quaternion component moved by more than 8 * 2^-24 relative (row {np.argwhere(worst > 0)[0]})"
