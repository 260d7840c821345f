"""gs_knn_dist2 on the device (pkg.knn_dist2, pkg.init_from_points): mean_dist2 and dist2 bit for bit against the brute force
restated in numpy (tests/knn_reference.py) at every size where the kernels take another path and on the structured clouds,
box_visits against the CPU simulation of the search (tests/native/knn_rules_sim.cpp) and against the derived condition on two
separated clusters, and the first lines of a trainer's loop end to end."""
import functools
import math

import numpy as np
import pytest
import torch  # at collection, before the package loads its library: both must bind the same HIP runtime

import knn_reference as kr
from test_gpu_lift import _queue_filler
from test_knn_api import STRUCTURED, _points, _restated, sim  # noqa: F401  (sim: the fixture that builds the simulation)

pytestmark = pytest.mark.gpu
F = np.float32


def device(a):
    return torch.as_tensor(np.ascontiguousarray(a, F)).cuda()


def run(pkg, points, k, **want):
    out = pkg.knn_dist2(device(points), k=k, **want)
    return {name: t.cpu().numpy() for name, t in out.items()}


def same_bits(got, want, label):
    got, want = np.ascontiguousarray(got, F).view(np.uint32), np.ascontiguousarray(want, F).view(np.uint32)
    assert got.shape == want.shape, label
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{label}: {len(bad)} value(s) differ, first at {tuple(bad[0])}: {got[tuple(bad[0])]:#010x} against {want[tuple(bad[0])]:#010x}"


def check(pkg, name, k):
    got = run(pkg, _points(name), k, mean=True, dist2=True, visits=True)
    want_mean, want_dist2 = _restated(name, k)
    same_bits(got["mean_dist2"], want_mean, f"{name}, k = {k}: mean_dist2")
    same_bits(got["dist2"], want_dist2, f"{name}, k = {k}: dist2")
    boxes = (len(want_mean) + kr.BOX - 1) // kr.BOX
    assert got["box_visits"].shape == (boxes,) and got["box_visits"].min() >= 1 and got["box_visits"].max() <= boxes
    return got


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("n", kr.SIZES)
def test_uniform_points_at_every_edge_of_a_box_and_of_a_radix_tile(pkg, gpu, n, k):
    """n below, at and above one box (one workgroup, the masked lanes of the last box), one radix tile, two; n <= k: fewer
    neighbours than asked for (+inf beyond, the mean over n - 1), one point: +0.0."""
    check(pkg, f"uniform{n}", k)


@pytest.mark.parametrize("name", [s for s in STRUCTURED if s != "two_clusters"])
def test_the_structured_clouds(pkg, gpu, name):
    """All points coincident (every value +0.0; nothing is passed over), the 17^3 lattice (ties everywhere; every mean exactly 1.0),
    the same scaled by 2^-10 at 1024 (differences that round) and at 10^6 (binary32 collapses it onto one point), a plane and a
    line (axes without extent), two clusters and an outlier whose neighbours sit in far boxes, points astride the bounding
    box's mid-planes (neighbours far apart in Morton order), subnormal coordinates and subnormal squares, coordinates of 10^19
    (d2 overflows for far pairs).  k = 3."""
    got = check(pkg, name, 3)
    if name in ("coincident", "lattice_collapsed"):
        assert np.all(got["mean_dist2"].view(np.uint32) == 0) and np.all(got["box_visits"] == len(got["box_visits"]))
    if name == "lattice":
        assert np.all(got["mean_dist2"] == 1.0)


def test_two_separated_clusters_keep_every_workgroup_inside_its_own_cluster(pkg, gpu, sim):  # noqa: F811
    """THE REJECTION CONDITION, on the device (its derivation: test_knn_api's test of the same name): box_visits[b] <= m, the
    sum <= 2 m^2 of the 4 m^2 box pairs -- and they are the simulation's, box by box."""
    m = 8
    got = check(pkg, "two_clusters", 3)
    assert len(got["box_visits"]) == 2 * m and got["box_visits"].max() <= m and got["box_visits"].sum() <= 2 * m * m
    assert np.array_equal(got["box_visits"].view(np.uint32), sim(kr.two_clusters(m), 3)[2])


@pytest.mark.parametrize("name,k", [("uniform4097", 8), ("clusters_outlier", 3), ("morton_discontinuity", 3), ("lattice", 3)])
def test_the_boxes_staged_are_the_simulations(pkg, gpu, sim, name, k):  # noqa: F811
    """The kernel decides GS_KNN_BOX walk positions per turn and tests the survivors again; the simulation walks one by one.  The
    radius only falls, so both stage the same boxes: box_visits are equal, box by box."""
    got = run(pkg, _points(name), k, mean=False, visits=True)
    assert set(got) == {"box_visits"}
    assert np.array_equal(got["box_visits"].view(np.uint32), sim(_points(name), k)[2])


def test_two_calls_give_the_same_bits_and_the_points_keep_theirs(pkg, gpu):
    p = device(kr.uniform(4097, seed=4))
    was = p.clone()
    a = pkg.knn_dist2(p, k=8, mean=True, dist2=True, visits=True)
    b = pkg.knn_dist2(p, k=8, mean=True, dist2=True, visits=True)
    assert set(a) == set(b) == {"mean_dist2", "dist2", "box_visits"}
    for name in a:
        assert torch.equal(a[name].view(torch.uint8), b[name].view(torch.uint8)), name
    assert torch.equal(p.view(torch.uint8), was.view(torch.uint8))
    assert a["mean_dist2"].dtype == torch.float32 and a["dist2"].shape == (4097, 8) and a["box_visits"].dtype == torch.int32


def test_points_that_a_queued_torch_kernel_is_still_writing(pkg, gpu):
    """The tensor protocol's wait: the points hold NaN when the call is made and get their values from a copy queued on torch's
    stream behind milliseconds of other work."""
    final = device(kr.uniform(2049))
    p = torch.full_like(final, float("nan"))
    torch.cuda.synchronize()
    keep = _queue_filler()
    p.copy_(final, non_blocking=True)
    out = pkg.knn_dist2(p, k=3, dist2=True)
    want_mean, want_dist2 = _restated("uniform2049", 3)
    same_bits(out["mean_dist2"].cpu().numpy(), want_mean, "mean_dist2")
    same_bits(out["dist2"].cpu().numpy(), want_dist2, "dist2")
    del keep


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_a_coordinate_that_is_not_finite_is_refused_and_nothing_is_launched(pkg, gpu, monkeypatch, bad):
    p = kr.uniform(513)
    p[300, 1] = bad
    t = device(p)

    class Refusing:
        def __getattr__(self, name):
            if name == "gs_knn_dist2":
                def called(*args):
                    raise AssertionError("gs_knn_dist2 was called")
                return called
            return getattr(real, name)
    real = pkg.binding.lib()
    monkeypatch.setattr(pkg.binding, "lib", lambda: Refusing())
    with pytest.raises(ValueError, match="NaN or infinite"):
        pkg.knn_dist2(t)
    with pytest.raises(ValueError, match="NaN or infinite"):
        pkg.init_from_points(t)


def test_no_points_is_no_work(pkg, gpu):
    out = pkg.knn_dist2(torch.zeros((0, 3), dtype=torch.float32, device="cuda"), k=3, dist2=True, visits=True)
    assert out["mean_dist2"].shape == (0,) and out["dist2"].shape == (0, 3) and out["box_visits"].shape == (0,)


def _ulps(a, b):
    """Distance in binary32 patterns between two arrays of finite floats of one sign."""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def test_init_from_points_makes_the_model_the_loop_starts_from(pkg, gpu):
    """the six tensors' shapes and dtypes; log_scales = the recipe on the restatement's mean_dist2 within 2 ulp
    (torch's float32 sqrt is correctly rounded, its log within 1 ulp; the 2 is the issue's); the other tensors exactly; the scene
    renders with a non-empty visible mask for a cloud in front of the camera, and one Adam step on it runs."""
    n, k = 1500, 3
    rec = pkg.synth.synth_records(n, seed=2, kind="S")
    xyz = np.ascontiguousarray(rec[:, :3], F)
    xyz[7] = xyz[3]                                   # a coincident pair: k = 3 still leaves a positive mean; the clamp below is for a triple
    xyz[11], xyz[12], xyz[13] = xyz[10], xyz[10], xyz[10]   # four coincident points: mean_dist2 = 0, the clamp at min_dist2 decides
    rgb = np.random.default_rng(3).uniform(0.0, 1.0, (n, 3)).astype(F)
    params = pkg.init_from_points(device(xyz), device(rgb), k=k, opacity=0.1, sh_degree=3)
    assert tuple(params) == pkg.binding.PARAMETER_NAMES
    shapes = pkg.binding._parameter_shapes(n, 15)
    for name, t in params.items():
        assert tuple(t.shape) == shapes[name] and t.dtype == torch.float32 and t.is_cuda and t.is_contiguous(), name
    mean, _ = kr.knn(xyz, k)
    assert np.all(mean[10:14] == 0.0)
    want = np.log(np.sqrt(np.maximum(mean, F(1e-7)).astype(F)).astype(F).astype(np.float64)).astype(F)
    got = params["log_scales"].cpu().numpy()
    assert np.array_equal(got[:, 0], got[:, 1]) and np.array_equal(got[:, 0], got[:, 2])
    assert _ulps(got[:, 0], want).max() <= 2
    same_bits(params["means"].cpu().numpy(), xyz, "means")
    assert np.array_equal(params["quats"].cpu().numpy(), np.tile(np.array([1, 0, 0, 0], F), (n, 1)))
    assert np.all(params["opacity_logits"].cpu().numpy() == F(math.log(0.1 / 0.9)))
    dc = params["sh_dc"].cpu().numpy()
    assert np.abs(dc - (rgb.astype(np.float64) - 0.5) / 0.28209479177387814).max() <= 4 * 2.0 ** -24 * 1.8
    assert not params["sh_rest"].any()
    for degree, coeffs in ((0, 0), (1, 3), (2, 8)):
        p2 = pkg.init_from_points(device(xyz[:50]), sh_degree=degree)
        assert tuple(p2["sh_rest"].shape) == (50, coeffs, 3) and not p2["sh_dc"].any()
    # the first lines of the loop
    scene = pkg.Scene.from_tensors(**params)
    rend = pkg.Renderer(scene)
    opt = pkg.Adam(scene, params, lr=1e-3)
    try:
        rend.render_host(pkg.camera_uniforms(pkg.make_camera(), 96, 64))
        mask = rend.visible_mask()
        assert int(mask.sum()) > 0
        grads = {name: torch.ones_like(t, dtype=torch.float64) for name, t in opt.params.items()}
        before = params["means"].clone()
        opt.step(grads, mask=mask)
        torch.cuda.synchronize()
        moved = (params["means"] != before).any(dim=1)
        assert opt.t == 1 and bool(moved.any()) and bool((moved <= mask.bool()).all())
    finally:
        rend.close()
        scene.close()


@functools.lru_cache(maxsize=None)
def _soak(n, k, samples):
    """The soak's cloud and its two references, computed once: (xyz, exact float64 dist2 of a tree, the sampled rows, the
    restatement's mean_dist2 and dist2 of those rows against all points)."""
    from scipy.spatial import cKDTree
    xyz = np.ascontiguousarray(_soak.synth.synth_records(n, seed=1, kind="T")[:, :3], F)
    p64 = xyz.astype(np.float64)
    d, _ = cKDTree(p64).query(p64, k=k + 1, workers=-1)
    rows = np.random.default_rng(8).choice(n, samples, replace=False)
    return (xyz, d[:, 1:] ** 2, rows) + kr.knn_rows(xyz, rows, k)


def test_a_clustered_cloud_of_200_000_points(pkg, gpu):
    """THE SOAK: synth.py's T statistics (80 % of the points in 96 blobs), k = 3.  Every value against scipy's float64 tree within
    the counted roundings (kr.rounding_bound), and 2 000 sampled queries bit for bit against the restatement run on those rows
    against all points."""
    n, k = 200000, 3
    _soak.synth = pkg.synth
    xyz, exact, rows, want_mean, want_dist2 = _soak(n, k, 2000)
    got = run(pkg, xyz, k, mean=True, dist2=True, visits=True)
    bound = kr.rounding_bound(k)
    assert np.all(np.abs(got["dist2"].astype(np.float64) - exact) <= bound * exact)
    assert np.all(np.abs(got["mean_dist2"].astype(np.float64) - exact.mean(axis=1)) <= bound * exact.mean(axis=1))
    same_bits(got["mean_dist2"][rows], want_mean, "sampled mean_dist2")
    same_bits(got["dist2"][rows], want_dist2, "sampled dist2")
    boxes = len(got["box_visits"])
    print(f"box pairs staged: {int(got['box_visits'].sum())} of {boxes * boxes} ({got['box_visits'].sum() / boxes ** 2:.4f})")
