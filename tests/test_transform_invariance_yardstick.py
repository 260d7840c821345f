"""The budget of the GPU test of gs_scene_transform's invariance (tests/test_gpu_scene_transform.py), pinned on the reference
alone: a scene moved by a similarity and seen through the camera moved with it shows the same frame -- up to binary32 rounding,
since positions, scales, rotations and SH coefficients of the moved scene are rounded once more.  Here the float64 transform of
the vertices (tests/transform_reference.py), rounded to binary32, is rendered by the oracle with the transformed camera
(gs_transform_camera) and compared with the original frame.  No kernel of the library runs.

The caps for the device are mean |d| <= 2e-4 and at most 2 % of the pixels beyond 1e-3 (threshold flips of the radius' ceil, the
1/255 cut and the T break move single pixels by up to alpha T rgb).  This test asserts that the reference itself stays within
HALF of each cap on the inputs the GPU test uses.

Measured (synth kind "A", seed 3, 128 x 96, rotation (0.61, -0.33, 0.52, 0.49), translation (0.7, -1.3, 0.45)):
    n     scale   visible (both)   mean |d|   pixels beyond 1e-3   max |d|
    1200  1.0     1131             3.5e-7     0                    3.8e-6
    1200  1.7     1131             2.8e-7     0                    3.9e-6
    1200  0.4     1131             4.5e-7     0                    6.3e-6
    5000  1.0     4716             3.6e-7     0                    4.2e-4
    5000  1.7     4716             2.8e-7     0                    4.2e-4
    5000  0.4     4716             4.4e-7     0                    4.2e-4
With the SH left unrotated: mean |d| 4.0e-2 (n = 1200) and 4.6e-2 (n = 5000), 79 % and 87 % of the pixels beyond 1e-3.
"""
import functools

import numpy as np
import pytest

import transform_reference as tr


@functools.lru_cache(maxsize=None)
def original(n):
    """(vertices, camera, frame, visible count) of the untransformed scene, computed once per size."""
    import __graft_entry__ as entry
    pkg, oracle = entry.load_package(), entry.load_oracle()
    verts = oracle.activate_records(pkg.synth.synth_records(n, seed=3, kind="A"))
    cam = oracle.default_camera(position=tr.CAMERA["position"], rotation=tr.unit(tr.CAMERA["rotation"]))
    ref = oracle.stages(verts, oracle.camera_uniforms(cam, tr.W, tr.H))
    ref["image"].setflags(write=False)
    return verts, cam, ref["image"], int((ref["tiles"] != 0).sum())


def moved_frame(pkg, oracle, verts64, cam, scale):
    v32 = np.ascontiguousarray(verts64.astype(np.float32)).view(oracle.VERTEX_DT).reshape(-1)
    cam2 = pkg.transform_camera(cam, tr.ROTATION, tr.TRANSLATION, scale)
    got = oracle.stages(v32, oracle.camera_uniforms(cam2, tr.W, tr.H))
    return got["image"], int((got["tiles"] != 0).sum())


@pytest.mark.parametrize("scale", tr.SCALES)
@pytest.mark.parametrize("n", [1200, 5000])
def test_the_reference_frame_is_invariant_within_half_the_devices_caps(pkg, oracle, n, scale):
    verts, cam, image, visible = original(n)
    assert visible > n // 2 and image[..., :3].max() > 0.1
    v64 = tr.transform_vertices(verts, tr.ROTATION, tr.TRANSLATION, scale)
    got, visible2 = moved_frame(pkg, oracle, v64, cam, scale)
    mean, beyond, worst = tr.frame_difference(got, image)
    print(f"n={n} s={scale}: visible {visible} / {visible2}, mean |d| {mean:.3g}, beyond 1e-3: {beyond * 100:.2f} %, max |d| {worst:.3g}")
    assert visible2 == visible
    assert mean <= tr.CAP_MEAN / 2 and beyond <= tr.CAP_FRACTION / 2


@pytest.mark.parametrize("n", [1200, 5000])
def test_unrotated_sh_is_far_outside_the_caps(pkg, oracle, n):
    """What the caps must catch: everything moved but the SH bands."""
    verts, cam, image, _ = original(n)
    v64 = tr.transform_vertices(verts, tr.ROTATION, tr.TRANSLATION, 1.7)
    v64[:, 12:60] = np.asarray(verts).view(np.float32).reshape(-1, 60)[:, 12:60]
    got, _ = moved_frame(pkg, oracle, v64, cam, 1.7)
    mean, beyond, _ = tr.frame_difference(got, image)
    print(f"n={n}: SH left alone: mean |d| {mean:.3g}, beyond 1e-3: {beyond * 100:.1f} %")
    assert mean > 10 * tr.CAP_MEAN and beyond > 10 * tr.CAP_FRACTION
