"""gs_knn_dist2 (include/gs3d_hip.h) as far as a machine without a GPU can check it: the restatement (tests/knn_reference.py)
against a float64 tree and against exact arithmetic, the CPU simulation of the whole search (tests/native/knn_rules_sim.cpp over
csrc/gs_knn_rules.h: the text the kernels compile) against the restatement bit for bit, the lower bound against every member pair,
three mutations of the search that the point sets must catch, the ABI's shape, and every refusal of the C ABI and of the Python
wrappers (they come before a device is touched)."""
import ctypes as C
import functools
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import knn_reference as kr
from helpers import FakeTensor as _Fake, forbid_c

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "3dgs.cpp_amd", "csrc")
GS_ERR_INVALID = -1
F = np.float32


# ------------------------------------------------------------------------------------------------ the simulation
@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    """run(points, k, mutation=0) -> (bits of mean_dist2 [n], bits of dist2 [n][k], box_visits [boxes]) of the CPU simulation;
    run.bounds(cases [count][12]) -> (bits of box_box_bound, bits of point_box_bound)."""
    work = tmp_path_factory.mktemp("knn")
    exe = str(work / "knn_rules_sim")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off", "-I", CSRC,
                           os.path.join(ROOT, "tests", "native", "knn_rules_sim.cpp"), "-o", exe])
    path = str(work / "input.bin")

    def run(points, k, mutation=0):
        p = np.ascontiguousarray(points, F).reshape(-1, 3)
        p.tofile(path)
        words = subprocess.check_output([exe, "search", path, str(len(p)), str(k), str(mutation)]).split()
        n, kk, boxes = (int(w) for w in words[:3])
        assert (n, kk, boxes) == (len(p), k, (len(p) + kr.BOX - 1) // kr.BOX)
        a = np.array(words[3:], dtype=np.uint64).astype(np.uint32)
        assert len(a) == n * (k + 1) + boxes
        table = a[:n * (k + 1)].reshape(n, k + 1)
        return table[:, 0], table[:, 1:], a[n * (k + 1):]

    def bounds(cases):
        c = np.ascontiguousarray(cases, F).reshape(-1, 12)
        c.tofile(path)
        words = subprocess.check_output([exe, "bounds", path, str(len(c))]).split()
        a = np.array(words, dtype=np.uint64).astype(np.uint32).reshape(len(c), 2)
        return a[:, 0].copy().view(F), a[:, 1].copy().view(F)

    run.bounds = bounds
    return run


@functools.lru_cache(maxsize=None)
def _structured():
    return kr.point_sets()


@functools.lru_cache(maxsize=None)
def _restated(name, k):
    """The restatement of a named point set, computed once."""
    if name.startswith("uniform"):
        return kr.knn(kr.uniform(int(name[7:])), k)
    if name == "two_clusters":
        return kr.knn(kr.two_clusters(), k)
    return kr.knn(_structured()[name], k)


def _points(name):
    if name.startswith("uniform"):
        return kr.uniform(int(name[7:]))
    return kr.two_clusters() if name == "two_clusters" else _structured()[name]


STRUCTURED = ("coincident", "lattice", "lattice_rounding", "lattice_collapsed", "plane", "line", "clusters_outlier",
              "morton_discontinuity", "subnormal", "subnormal_squares", "large", "two_clusters")
CASES = [(f"uniform{n}", k) for n in kr.SIZES for k in (1, 3, 8)] + [(name, 3) for name in STRUCTURED]


def _same(sim_out, restated):
    return np.array_equal(sim_out[0], kr.bits(restated[0])) and np.array_equal(sim_out[1], kr.bits(restated[1]))


@pytest.mark.parametrize("name,k", CASES, ids=[f"{n}-k{k}" for n, k in CASES])
def test_the_simulated_search_gives_the_brute_forces_bits(sim, name, k):
    """Codes, stable sort, boxes, own box first, the walk with the workgroup's rejection and the lanes' own -- all of
    gs_knn_rules.h -- against the brute force: mean_dist2 and dist2 bit for bit.  (Fails without csrc/gs_knn_rules.h.)"""
    mean, dist2, visits = sim(_points(name), k)
    ref_mean, ref_dist2 = _restated(name, k)
    assert np.array_equal(mean, kr.bits(ref_mean))
    assert np.array_equal(dist2, kr.bits(ref_dist2))
    boxes = len(visits)
    assert visits.min() >= 1 and visits.max() <= boxes


def test_the_point_sets_are_what_their_names_say():
    sets = _structured()
    assert len(sets["lattice"]) == 17 ** 3 and all(len(p) == 4097 for n, p in sets.items() if not n.startswith("lattice"))
    assert np.all(_restated("coincident", 3)[0] == 0.0) and not np.signbit(_restated("coincident", 3)[0]).any()
    assert np.all(_restated("lattice", 3)[0] == 1.0)                          # a corner has exactly three neighbours at distance 1
    assert np.all(_restated("lattice_collapsed", 3)[0] == 0.0) and len(np.unique(sets["lattice_collapsed"], axis=0)) == 1
    assert len(np.unique(sets["lattice_rounding"], axis=0)) == 17 ** 3        # ... and here nothing collapsed
    assert np.ptp(sets["plane"][:, 2]) == 0 and np.ptp(sets["line"][:, 1]) == 0 and np.ptp(sets["line"][:, 2]) == 0
    tiny = np.finfo(F).tiny
    assert 0 < np.abs(sets["subnormal"]).max() < tiny
    d = _restated("subnormal_squares", 3)[1]
    assert ((d > 0) & (d < tiny)).any()                                        # subnormal distances are among the results
    with np.errstate(over="ignore"):
        p = sets["large"]
        far = ((p[0] - p[1:]) ** 2).sum(axis=1, dtype=F)
    assert np.isinf(far).any() and np.isfinite(_restated("large", 3)[0]).all()  # d2 overflows for far pairs, in the restatement too


def test_two_separated_clusters_keep_every_query_box_inside_its_own_cluster(sim):
    """THE REJECTION CONDITION.  Two clusters of m BOX points in opposite corners, all three axes differing: every code of one
    lies below every code of the other, so the sorted order holds m boxes of one and then m of the other.  After its own box a
    workgroup's radius is at most its cluster's diameter squared (3 * 0.05^2), below the gap squared between the clusters' boxes
    (3 * 1.9^2): every box of the other cluster is passed over, visits <= m, the sum <= 2 m^2 of the 4 m^2 pairs."""
    m = 8
    mean, dist2, visits = sim(kr.two_clusters(m), 3)
    assert _same((mean, dist2), _restated("two_clusters", 3))
    assert len(visits) == 2 * m and visits.max() <= m and visits.sum() <= 2 * m * m


# ------------------------------------------------------------------------------------------------ the restatement itself
def test_the_restatement_is_within_the_counted_roundings_of_a_float64_tree():
    """scipy's cKDTree in float64 on the same binary32 inputs.  THE BOUND (kr.rounding_bound): with u = 2^-24, a difference
    carries one rounding, its square that twice and one of its own (3 u), the two sums at most 2 more: |d2 - exact| <= 5 u exact.
    The i-th smallest of values that each moved by at most a relative t moved by at most t.  The running sum of k values rounds
    k - 1 times, the division once: (k + 5) u in all (the issue counts k + 6; the smaller figure is used), doubled for margin.
    The tree's own float64 arithmetic is 2^-29 of one u.  Coordinates of order one: nothing is subnormal."""
    from scipy.spatial import cKDTree
    for n, k in ((4097, 3), (2049, 8), (513, 1)):
        p = kr.uniform(n, seed=9)
        mean, dist2 = kr.knn(p, k)
        d, _ = cKDTree(p.astype(np.float64)).query(p.astype(np.float64), k=k + 1)
        exact = d[:, 1:].reshape(n, k) ** 2
        bound = kr.rounding_bound(k)
        assert np.all(np.abs(dist2.astype(np.float64) - exact) <= bound * exact)
        assert np.all(np.abs(mean.astype(np.float64) - exact.mean(axis=1)) <= bound * exact.mean(axis=1))


def _rne(x):
    """The binary32 nearest the Fraction x, ties to even, as a Fraction (no overflow in this test's range)."""
    if x == 0:
        return Fraction(0)
    s, a = (-1 if x < 0 else 1), abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    quantum = Fraction(2) ** (max(e, -126) - 23)
    q = a / quantum
    n = q.numerator // q.denominator
    rest = q - n
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and n % 2 == 1):
        n += 1
    return s * n * quantum


def test_the_restatement_is_exact_arithmetic_with_one_rounding_per_operation():
    """A dozen points, a scalar loop in fractions.Fraction, round-to-nearest-even after every operation, a selection by sorting:
    bit for bit.  Coordinates with full mantissas, a coincident pair and a pair one ulp apart."""
    rng = np.random.default_rng(12)
    p = (rng.uniform(-3.0, 3.0, (12, 3)) * np.array([1.0, 1e-3, 37.0])).astype(F)
    p[5] = p[2]
    p[7] = np.nextafter(p[3], F(9.0))
    for k in (1, 3, 8):
        mean, dist2 = kr.knn(p, k)
        for i in range(len(p)):
            cand = []
            for j in range(len(p)):
                if j == i:
                    continue
                d = [_rne(Fraction(float(p[i][a])) - Fraction(float(p[j][a]))) for a in range(3)]
                sq = [_rne(v * v) for v in d]
                cand.append(_rne(_rne(sq[0] + sq[1]) + sq[2]))
            best = sorted(cand)[:k]
            s = best[0]
            for v in best[1:]:
                s = _rne(s + v)
            assert [Fraction(float(v)) for v in dist2[i]] == best, (k, i)
            assert Fraction(float(mean[i])) == _rne(s / k), (k, i)
    # fewer neighbours than k: the mean over n - 1, +inf beyond; one point: +0.0
    mean, dist2 = kr.knn(p[:3], 8)
    assert np.isinf(dist2[:, 2:]).all() and np.isfinite(dist2[:, :2]).all()
    assert np.array_equal(mean, ((dist2[:, 0] + dist2[:, 1]).astype(F) / F(2)).astype(F))
    mean, dist2 = kr.knn(p[:1], 3)
    assert kr.bits(mean)[0] == 0 and np.isinf(dist2).all()


# ------------------------------------------------------------------------------------------------ the bound
def _d2(a, b):
    """The restatement's d2 between points a [..., 3] and b [..., 3], broadcast."""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        d = (a - b).astype(F)
        sq = (d * d).astype(F)
        return ((sq[..., 0] + sq[..., 1]).astype(F) + sq[..., 2]).astype(F)


def _hold(sim, A, B, label):
    """A, B: [cases][members][3].  The box bound of (box of A, box of B) is <= d2 of every member pair, and the point bound of
    (A's lowest corner as a point, box of B) is <= d2 of that point and every member of B."""
    A, B = np.ascontiguousarray(A, F), np.ascontiguousarray(B, F)
    lo_a, hi_a, lo_b, hi_b = A.min(axis=1), A.max(axis=1), B.min(axis=1), B.max(axis=1)
    box, point = sim.bounds(np.concatenate([lo_a, hi_a, lo_b, hi_b], axis=1))
    pairs = _d2(A[:, :, None, :], B[:, None, :, :]).reshape(len(A), -1)
    assert not np.isnan(box).any() and not np.isnan(point).any(), label
    assert np.all(box[:, None] <= pairs), label
    assert np.all(point[:, None] <= _d2(lo_a[:, None, :], B)), label
    assert np.all(box >= 0) and np.all(point >= 0), label
    return box


def test_the_bound_never_exceeds_the_distance_of_any_member_pair(sim):
    """10^5 random pairs of boxes over twelve decades of scale, separated, touching and overlapping; then the adversarial ones:
    a point on the box's face, gaps of one ulp, subnormal gaps, and coordinates near 2^10 against a box of spacing 2^-10, where
    fl(x - hi) rounds.  Every box carries its corners among its members, so the extreme pairs are there."""
    rng = np.random.default_rng(31)
    count, m = 100000, 4

    def members(centre, size):
        pts = centre[:, None, :] + rng.uniform(-1.0, 1.0, (len(centre), m, 3)) * size[:, None, None]
        return pts.astype(F)

    scale = 10.0 ** rng.uniform(-6, 6, count)
    centre_a = rng.uniform(-1.0, 1.0, (count, 3)) * scale[:, None]
    offset = rng.uniform(-1.0, 1.0, (count, 3)) * (scale * 10.0 ** rng.uniform(-4, 1, count))[:, None]
    offset[rng.random((count, 3)) < 0.3] = 0.0   # axes on which the boxes meet
    A, B = members(centre_a, scale * 10.0 ** rng.uniform(-5, 0, count)), members(centre_a + offset, scale * 10.0 ** rng.uniform(-5, 0, count))
    box = _hold(sim, A, B, "random")
    assert (box > 0).mean() > 0.2 and (box == 0).mean() > 0.05   # both kinds occur

    def corners(lo, hi):
        """[cases][8 corners + the two given][3]"""
        sel = np.array([[(c >> a) & 1 for a in range(3)] for c in range(8)], bool)
        return np.where(sel[None, :, :], hi[:, None, :], lo[:, None, :]).astype(F)

    cases = 2000
    lo = rng.uniform(-2.0, 2.0, (cases, 3)).astype(F)
    hi = (lo + rng.uniform(0.0, 1.0, (cases, 3)).astype(F)).astype(F)
    # a point on the face, and one ulp off it
    on_face = corners(hi, hi)
    box = _hold(sim, on_face, corners(lo, hi), "face")
    assert np.all(box == 0)
    above = np.nextafter(hi, F(np.inf))
    box = _hold(sim, corners(lo, hi), corners(above, (above + F(1.0)).astype(F)), "one ulp")
    assert np.all(box > 0)
    # subnormal gaps: A ends at 0, B begins a few subnormal steps above
    zero = np.zeros((cases, 3), F)
    step = (rng.integers(1, 5, (cases, 3)) * 2.0 ** -149).astype(F)
    box = _hold(sim, corners((zero - step).astype(F), zero), corners(step, (step + step).astype(F)), "subnormal")
    assert np.all(box == 0) and step.min() > 0   # (the squares underflow: 0 is the bound, and d2, too)
    # near 2^10 against spacing 2^-10: the differences round
    fine = (rng.integers(0, 1 << 20, (cases, 3)) * 2.0 ** -30).astype(F)
    big = (1024.0 + rng.integers(0, 1 << 13, (cases, 3)) * 2.0 ** -13).astype(F)
    box = _hold(sim, corners(fine, (fine + F(2.0 ** -10)).astype(F)), corners(big, (big + F(2.0 ** -10)).astype(F)), "2^10")
    assert np.all(box > 1e6)
    _hold(sim, corners(big, (big + F(2.0 ** -10)).astype(F)), corners(fine, (fine + F(2.0 ** -10)).astype(F)), "2^10 reversed")


# ------------------------------------------------------------------------------------------------ mutations
@pytest.mark.parametrize("mutation,name,what", [(1, f"uniform{kr.BOX + 1}", "rejecting before k values are kept: the last box's one lane has none after its own box"),
                                                (2, "uniform4097", "a bound from the boxes' centres exceeds the distance of members near the faces"),
                                                (3, "coincident", "passing over by position loses the coincident points at other indices")])
def test_a_mutated_search_is_caught_by_the_point_sets(sim, mutation, name, what):
    assert _same(sim(_points(name), 3), _restated(name, 3))
    assert not _same(sim(_points(name), 3, mutation), _restated(name, 3)), what


# ------------------------------------------------------------------------------------------------ the ABI's shape
def test_the_symbols_are_declared_listed_and_exported(pkg):
    with open(os.path.join(ROOT, "include", "gs3d_hip.h")) as f:
        header = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    L, b = pkg.binding.lib(), pkg.binding
    assert re.search(r"\bint\s+gs_knn_dist2\s*\(", header) and re.search(r"\buint64_t\s+gs_knn_scratch_bytes\s*\(", header)
    for name in ("gs_knn_dist2", "gs_knn_scratch_bytes"):
        assert name in b.SYMBOLS and hasattr(L, name)
    assert "gs_knn.hip" in b.KERNEL_SOURCES and "gs_knn_rules.h" in b.KERNEL_SOURCES
    with open(os.path.join(CSRC, "Makefile")) as f:
        text = f.read()
    assert re.search(r"^KERNELS\s*:=.*\bgs_knn\.hip\b", text, flags=re.M) and re.search(r"^HDRS\s*:=.*\bgs_knn_rules\.h\b", text, flags=re.M)
    assert int(re.search(r"#define\s+GS_KNN_MAX_K\s+(\d+)", header).group(1)) == b.KNN_MAX_K == 8
    assert int(re.search(r"#define\s+GS_KNN_BOX\s+(\d+)u", header).group(1)) == b.KNN_BOX == kr.BOX
    assert pkg.knn_dist2 is b.knn_dist2 and pkg.init_from_points is b.init_from_points


def _scratch_bytes(L, n):
    L.gs_knn_scratch_bytes.restype, L.gs_knn_scratch_bytes.argtypes = C.c_uint64, [C.c_uint64]
    return int(L.gs_knn_scratch_bytes(C.c_uint64(n)))


def test_the_scratch_grows_with_the_points_and_is_nothing_for_none(pkg):
    L = pkg.binding.lib()
    assert _scratch_bytes(L, 0) == 0
    sizes = [_scratch_bytes(L, n) for n in (1, 255, 256, 257, 4097, 1 << 20)]
    assert sizes == sorted(sizes) and sizes[0] > 0
    # 16 (sorted) + 16 (two key and two id arrays) bytes per point, the boxes, the radix tables: below 40 bytes per point at 1 M
    assert 32 * (1 << 20) <= sizes[-1] <= 40 * (1 << 20)


# ------------------------------------------------------------------------------------------------ refusals
def test_the_c_entry_refuses_before_any_device_is_touched(pkg):
    """Each call is wrong in ONE way and is refused with GS_ERR_INVALID and a message that names the fault; device 1 << 20 does
    not exist, so a call that got as far as selecting it complains of the device instead."""
    L = pkg.binding.lib()
    call = L.gs_knn_dist2
    n = 1000
    need = _scratch_bytes(L, n)
    good = dict(points=4096, n=n, k=3, mean=8192, dist2=16384, visits=32768, scratch=65536, bytes=need)

    def rc(**change):
        a = dict(good, **change)
        ptr = lambda v: C.c_void_p(v) if v else None
        return call(ptr(a["points"]), C.c_uint64(a["n"]), C.c_int(a["k"]), ptr(a["mean"]), ptr(a["dist2"]), ptr(a["visits"]),
                    ptr(a["scratch"]), C.c_uint64(a["bytes"]), C.c_int(1 << 20), None)

    refusals = [(dict(points=0), "points"), (dict(n=1 << 31), "2^31"), (dict(n=(1 << 31) + 5, bytes=1 << 40), "2^31"),
                (dict(k=0), "k"), (dict(k=9), "k"), (dict(k=-1), "k"),
                (dict(mean=0, dist2=0, visits=0), "output"), (dict(scratch=0), "scratch"), (dict(bytes=need - 1), "scratch"),
                (dict(bytes=0), "scratch"), (dict(points=4098), "points"), (dict(mean=8194), "mean_dist2"), (dict(dist2=16385), "dist2"),
                (dict(visits=32770), "box_visits"), (dict(scratch=65537), "scratch")]
    for change, word in refusals:
        assert rc(**change) == GS_ERR_INVALID, change
        assert word in L.gs_last_error().decode(), (change, L.gs_last_error().decode())
    # n == 0: success, nothing launched, nothing touched -- with no points, no scratch, and a device that does not exist
    assert rc(n=0, points=0, scratch=0, bytes=0) == 0
    assert rc(n=0, points=0, scratch=0, bytes=0, k=0) == GS_ERR_INVALID
    # one output is enough; a well-formed call goes on to the device, which is not there: that is what it then complains of
    for change in (dict(mean=0, dist2=0), dict()):
        assert rc(**change) != 0 and "device" in L.gs_last_error().decode().lower(), change


def test_the_wrappers_refuse_what_is_not_a_point_cloud_before_c_is_reached(pkg, monkeypatch):
    forbid_c(pkg, monkeypatch)
    good = _Fake((100, 3))
    for fn in (pkg.knn_dist2, pkg.init_from_points):
        with pytest.raises(TypeError, match="device tensor"):
            fn(np.zeros((100, 3), F))
        with pytest.raises(TypeError, match="dtype"):
            fn(_Fake((100, 3), dtype="torch.float64"))
        with pytest.raises(ValueError, match="shape"):
            fn(_Fake((100, 4)))
        with pytest.raises(ValueError, match="shape"):
            fn(_Fake((100, 3, 3)))
        with pytest.raises(ValueError, match="contiguous"):
            fn(_Fake((100, 3), contiguous=False))
        with pytest.raises(ValueError, match="CPU"):
            fn(_Fake((100, 3), device="cpu"))
    for k in (0, 9, -3):
        with pytest.raises(ValueError, match="outside"):
            pkg.knn_dist2(good, k=k)
    for k in (3.0, "3", True, None):
        with pytest.raises(TypeError, match="int"):
            pkg.knn_dist2(good, k=k)
    with pytest.raises(ValueError, match="nothing asked"):
        pkg.knn_dist2(good, mean=False)
    with pytest.raises(ValueError, match="sh_degree"):
        pkg.init_from_points(good, sh_degree=4)
    for opacity in (0.0, 1.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="opacity"):
            pkg.init_from_points(good, opacity=opacity)
    with pytest.raises(ValueError, match="min_dist2"):
        pkg.init_from_points(good, min_dist2=0.0)
    with pytest.raises(ValueError, match="rows"):
        pkg.init_from_points(good, colours=_Fake((99, 3)))
    with pytest.raises(ValueError, match="shape"):
        pkg.init_from_points(good, colours=_Fake((100, 4)))
    with pytest.raises(ValueError, match="device"):
        pkg.init_from_points(good, colours=_Fake((100, 3), device="cuda:1"))
    # ... and a well-formed call goes on to C
    with pytest.raises(AssertionError, match="C library was reached"):
        pkg.knn_dist2(good)
