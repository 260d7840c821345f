"""The contract of gs_knn_dist2 (include/gs3d_hip.h) restated in numpy: the brute force over all pairs in binary32, one explicit
rounding after every operation, and the point sets the CPU and GPU tests share.

    dx = fl(xi - xj) ...;  d2 = fl(fl(fl(dx dx) + fl(dy dy)) + fl(dz dz))   for every j != i by index
    best = the ke = min(k, n - 1) smallest, ascending; a candidate replaces a kept value only where d2 < kept, so +inf (an
           overflowed d2) and NaN are never kept: the slot stays +inf
    mean_dist2 = fl(fl(... fl(best[0] + best[1]) + ...) / (float)ke), +0.0 where ke == 0;  dist2 = best padded with +inf to k

Nothing here knows of Morton codes or boxes: that is the point."""
import numpy as np

F = np.float32
CHUNK = 512
BOX = 256          # GS_KNN_BOX
RADIX_TILE = 2048  # keys per tile of the radix passes


def knn_rows(points, rows, k):
    """(mean_dist2 [len(rows)], dist2 [len(rows)][k]) of the queries `rows` (indices into points) against ALL points."""
    p = np.ascontiguousarray(points, F).reshape(-1, 3)
    rows = np.asarray(rows, np.int64)
    n, ke = len(p), min(k, len(p) - 1)
    dist2 = np.full((len(rows), k), np.inf, F)
    mean = np.zeros(len(rows), F)
    if ke <= 0:
        return mean, dist2
    with np.errstate(over="ignore", invalid="ignore"):
        chunk = max(1, min(CHUNK, (1 << 23) // n))   # (a chunk's temporaries stay within some tens of megabytes)
        for c0 in range(0, len(rows), chunk):
            r = rows[c0:c0 + chunk]
            q = p[r]
            dx = (q[:, None, 0] - p[None, :, 0]).astype(F)
            dy = (q[:, None, 1] - p[None, :, 1]).astype(F)
            dz = (q[:, None, 2] - p[None, :, 2]).astype(F)
            xx, yy, zz = (dx * dx).astype(F), (dy * dy).astype(F), (dz * dz).astype(F)
            d2 = ((xx + yy).astype(F) + zz).astype(F)
            d2[np.arange(len(r)), r] = np.inf          # j != i, by index
            d2[np.isnan(d2)] = np.inf                  # never kept (cannot arise from finite coordinates)
            best = np.sort(np.partition(d2, ke - 1, axis=1)[:, :ke], axis=1).astype(F)
            dist2[c0:c0 + len(r), :ke] = best
            s = best[:, 0].copy()
            for i in range(1, ke):
                s = (s + best[:, i]).astype(F)
            mean[c0:c0 + len(r)] = (s / F(ke)).astype(F)
    return mean, dist2


def knn(points, k):
    """(mean_dist2 [n], dist2 [n][k]) of every point."""
    n = len(np.asarray(points).reshape(-1, 3))
    return knn_rows(points, np.arange(n), k)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def rounding_bound(k):
    """Relative bound between the binary32 restatement and the same quantity computed exactly on the same binary32 inputs, for
    results in the normal range.  u = 2^-24.  d2: each difference carries one rounding, (1 + e)^2 through its square, whose
    rounding adds one: 3 per term; the two sums add 2 more to the terms that pass through both: at most 5 roundings on any part,
    so d2 = exact (1 + t), |t| <= 5 u + O(u^2).  Order statistics are monotone: if every value moves by a relative t at most, so
    does the i-th smallest.  The running sum of k values rounds k - 1 times, the division once: k + 5 roundings, (k + 5) u.
    (The issue's (k + 6) u counts one more; the tests use twice THIS figure, 2 (k + 5) u, plus the second-order terms' 1e-12.)"""
    return 2.0 * (k + 5) * 2.0 ** -24 + 1e-12


# ---------------------------------------------------------------------------------------------------------------- point sets
SIZES = (1, 2, 3, 4, 9, BOX - 1, BOX, BOX + 1, 2 * BOX + 1, RADIX_TILE - 1, RADIX_TILE, RADIX_TILE + 1, 2 * RADIX_TILE + 1)


def uniform(n, seed=0):
    return np.random.default_rng(1000 + 7 * n + seed).uniform(-1.0, 1.0, (n, 3)).astype(F)


def lattice17():
    """The 17^3 integer lattice, 4913 points, x fastest: ties everywhere; a corner has exactly three neighbours at distance 1,
    every other point more, so every mean at k = 3 is exactly 1.0."""
    g = np.arange(17, dtype=F)
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1).astype(F)


def point_sets():
    """name -> float32 [n][3], n = 4097 (4913 for the lattices): the structured clouds of the GPU tests (k = 3), which the CPU simulation is held to first."""
    n = 4097
    rng = np.random.default_rng(77)
    sets = {}
    sets["coincident"] = np.tile(np.array([[0.25, -3.0, 7.5]], F), (n, 1))
    lat = lattice17()
    sets["lattice"] = lat
    sets["lattice_rounding"] = (lat * F(2.0 ** -10) + F(1024.0)).astype(F)
    sets["lattice_collapsed"] = (lat * F(2.0 ** -10) + F(1e6)).astype(F)   # spacing 2^-10 against an ulp of 2^-4: one point
    plane = uniform(n, 1)
    plane[:, 2] = F(0.5)
    sets["plane"] = plane
    line = uniform(n, 2)
    line[:, 1], line[:, 2] = F(-2.0), F(3.0)
    sets["line"] = line
    a = (rng.uniform(0.0, 1e-3, (n // 2, 3)) + np.array([-1.0, -1.0, -1.0])).astype(F)
    b = (rng.uniform(0.0, 1e-3, (n - 1 - n // 2, 3)) + np.array([1.0, 1.0, 1.0])).astype(F)
    sets["clusters_outlier"] = np.concatenate([a, b, np.array([[1.0, -1.0, 0.1]], F)]).astype(F)[rng.permutation(n)]
    mid = uniform(n, 3)
    side = rng.integers(0, 2, (n, 3)) * 2 - 1
    mid[: n // 2] = (side[: n // 2] * rng.uniform(0.0, 1e-6, (n // 2, 3))).astype(F)   # within 1e-6 of the mid-planes of [-1, 1]^3
    mid[0], mid[1] = F(-1.0), F(1.0)                                                    # (pin the box)
    sets["morton_discontinuity"] = mid
    sub = (rng.integers(0, 40, (n, 3)).astype(np.float64) * 2.0 ** -149).astype(F)      # subnormal coordinates and separations
    sets["subnormal"] = sub
    sets["subnormal_squares"] = (rng.integers(0, 40, (n, 3)).astype(np.float64) * 2.0 ** -70).astype(F)   # d2 = integers x 2^-140
    sets["large"] = (rng.uniform(-1.0, 1.0, (n, 3)) * 1e19).astype(F)                   # squares overflow: d2 = +inf
    return sets


def two_clusters(m=8, seed=5):
    """2 m BOX points: m BOX in each of two opposite corners, all three axes differing, each cluster's diameter far below the
    gap: any interleave separates them at the code's top bits and no box of BOX sorted points straddles them."""
    rng = np.random.default_rng(seed)
    a = (rng.uniform(0.0, 0.05, (m * BOX, 3)) + np.array([-1.0, -1.0, -1.0])).astype(F)
    b = (rng.uniform(-0.05, 0.0, (m * BOX, 3)) + np.array([1.0, 1.0, 1.0])).astype(F)
    return np.concatenate([a, b]).astype(F)[rng.permutation(2 * m * BOX)]
