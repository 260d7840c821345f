"""gs_scene_transform / gs_transform_sh_matrices / gs_transform_camera (include/gs3d_hip.h) as far as a machine without a GPU can
check them: the symbols, every refusal (they come before a device is selected), and the host arithmetic of
3dgs.cpp_amd/csrc/gs_sh_rotation.h -- the SH band matrices against a float64 restatement by least squares
(tests/transform_reference.py, whose basis is first shown to be the renderer's), their algebra, and the transformed camera.
"""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import np_reference as ref64
import transform_reference as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gs_scene_transform", "gs_transform_sh_matrices", "gs_transform_camera")
GS_ERR_INVALID = -1


def test_the_three_symbols_are_declared_listed_and_exported(pkg):
    with open(os.path.join(ROOT, "include", "gs3d_hip.h")) as f:
        header = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    L = pkg.binding.lib()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), f"{name} is not declared in include/gs3d_hip.h"
        assert name in pkg.binding.SYMBOLS
        assert hasattr(L, name), f"{name} is not exported by libgs3d_hip.so"
    assert "gs_transform;" in header
    assert C.sizeof(pkg.binding.Transform) == 32
    for name in ("transform_camera", "sh_rotation_matrices"):
        assert callable(getattr(pkg, name))
    assert callable(pkg.Scene.transform)


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def _refused(pkg, rc, word=None):
    assert rc == GS_ERR_INVALID, rc
    msg = pkg.binding.lib().gs_last_error().decode()
    assert msg.strip(), "GS_ERR_INVALID without a message"
    if word:
        assert word in msg, (word, msg)
    return msg


def _bad_transforms(pkg):
    make = pkg.binding._transform
    inf, nan = float("inf"), float("nan")
    for s in (0.0, -0.0, -1.0, inf, -inf, nan):
        yield make((1, 0, 0, 0), (0, 0, 0), s), "scale"
    for k in range(3):
        for bad in (inf, -inf, nan):
            t = [0.0, 0.0, 0.0]
            t[k] = bad
            yield make((1, 0, 0, 0), t, 1.0), "translation"
    for k in range(4):
        for bad in (inf, nan):
            q = [1.0, 0.0, 0.0, 0.0]
            q[k] = bad
            yield make(q, (0, 0, 0), 1.0), "quaternion"
    yield make((0, 0, 0, 0), (0, 0, 0), 1.0), "zero norm"
    yield make((0, -0.0, 0, 0), (1, 2, 3), 2.0), "zero norm"


def test_every_entry_refuses_a_bad_transform_before_it_selects_a_device(pkg):
    """On a machine without a device anything that reached one would come back as GS_ERR_DEVICE (-3), not -1."""
    L = pkg.binding.lib()
    out, cam, cam_out = np.zeros(83, np.float32), pkg.make_camera(), pkg.make_camera()
    good = pkg.binding._transform((1, 0, 0, 0), (0, 0, 0), 1.0)
    fake_scene = C.c_void_p(0)
    _refused(pkg, L.gs_scene_transform(fake_scene, None, C.c_uint64(0), C.c_uint64(1), None), "null")
    _refused(pkg, L.gs_scene_transform(None, C.byref(good), C.c_uint64(0), C.c_uint64(1), None), "null")
    _refused(pkg, L.gs_scene_transform(None, C.byref(good), C.c_uint64(0), C.c_uint64(0), None), "null")
    _refused(pkg, L.gs_transform_sh_matrices(None, pkg.binding._p(out)), "null")
    _refused(pkg, L.gs_transform_sh_matrices(C.byref(good), None), "null")
    _refused(pkg, L.gs_transform_camera(None, pkg.binding._p(cam), pkg.binding._p(cam_out)), "null")
    _refused(pkg, L.gs_transform_camera(C.byref(good), None, pkg.binding._p(cam_out)), "null")
    _refused(pkg, L.gs_transform_camera(C.byref(good), pkg.binding._p(cam), None), "null")
    cases = list(_bad_transforms(pkg))
    assert len(cases) == 6 + 9 + 8 + 2
    for t, word in cases:
        _refused(pkg, L.gs_scene_transform(None, C.byref(t), C.c_uint64(0), C.c_uint64(1), None), word)
        _refused(pkg, L.gs_transform_sh_matrices(C.byref(t), pkg.binding._p(out)), word)
        _refused(pkg, L.gs_transform_camera(C.byref(t), pkg.binding._p(cam), pkg.binding._p(cam_out)), word)
    assert not out.any()
    # the Python layer passes the same refusals on
    with pytest.raises(pkg.binding.GsError, match="scale") as e:
        pkg.transform_camera(cam, scale=0.0)
    assert e.value.code == GS_ERR_INVALID
    with pytest.raises(pkg.binding.GsError, match="zero norm"):
        pkg.sh_rotation_matrices((0, 0, 0, 0))


# ---- the basis is the renderer's ----------------------------------------------------------------------------------------------
def check_the_restated_basis_is_the_renderers(pkg, oracle):
    """The colour of a few Gaussians from the restatement's basis, against np_reference.preprocess (float64, the same functions with
    binary64 constants: they differ from the kernel's binary32 ones by <= 2^-25 relative, 6e-8 of the terms' sum) and against
    the oracle's preprocess (binary32: a few 1e-7 of rounding on 16 terms)."""
    n = 40
    rec = pkg.synth.synth_records(n, seed=5, kind="A")
    scene = ref64.activate(rec)
    cam = ref64.camera((0.3, -0.2, 0.1), (1, 0, 0, 0), 45.0, 0.1, 1000.0, 128, 96)
    want = ref64.preprocess(scene, cam, rules=dict(clamp_channels=()))["rgb"]  # no clamp: the whole function, both signs
    d = scene["pos"] - cam["cam"]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    got = ref64.SH_C0 * scene["sh"][:, 0] + tr.colour(scene["sh"], d) + 0.5
    terms = np.abs(scene["sh"]).sum(axis=1).max() * 3.0  # |basis| < 3
    assert np.abs(got - want).max() <= 1e-7 * terms, np.abs(got - want).max()
    verts = oracle.activate_records(rec)
    u = oracle.camera_uniforms(oracle.default_camera(position=(0.3, -0.2, 0.1)), 128, 96)
    attr, tiles = oracle.preprocess(verts, oracle.cov3d(verts), u)
    vis = tiles != 0
    assert vis.sum() >= n // 2
    rgb32 = attr["color_radii"][vis, :3].astype(np.float64)
    clamped = got.copy()
    clamped[:, 0] = np.maximum(clamped[:, 0], 0.0)
    assert np.abs(clamped[vis] - rgb32).max() <= 32 * 2.0 ** -24 * terms, np.abs(clamped[vis] - rgb32).max()
    assert np.abs(got - 0.5).max() > 0.05  # the bands carry colour in these scenes


# ---- the matrices ------------------------------------------------------------------------------------------------------------
def _rotations():
    """The identity, the 24 rotations that permute the axes (the cube's group, the identity among them), 200 random ones."""
    qs = [np.array([1.0, 0.0, 0.0, 0.0])]
    h = np.sqrt(0.5)
    cube = []
    for q in itertools.chain(
            ([1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]),
            ([h * a, h * b, 0, 0] for a in (1,) for b in (1, -1)), ([h, 0, h * b, 0] for b in (1, -1)), ([h, 0, 0, h * b] for b in (1, -1)),
            ([0, h, h * b, 0] for b in (1, -1)), ([0, h, 0, h * b] for b in (1, -1)), ([0, 0, h, h * b] for b in (1, -1)),
            ([0.5, 0.5 * a, 0.5 * b, 0.5 * c] for a in (1, -1) for b in (1, -1) for c in (1, -1))):
        cube.append(np.array(q, np.float64))
    assert len(cube) == 24
    for q in cube:  # each is a signed permutation matrix, all different
        R = tr.rotation_matrix(q)
        assert np.allclose(np.abs(R).sum(axis=0), 1) and np.allclose(np.sort(np.abs(R).ravel())[-3:], 1)
    assert len({tuple(np.round(tr.rotation_matrix(q)).astype(int).ravel()) for q in cube}) == 24
    rng = np.random.default_rng(77)
    rand = [q * rng.choice([1e-3, 1.0, 50.0]) for q in rng.normal(size=(200, 4))]  # the quaternion's length must not matter
    return qs + cube + rand


def _matrices(pkg, q):
    """(the library's three matrices as float64, R in float64 of the binary32 quaternion the library was given)."""
    q32 = np.asarray(q, np.float32)
    return [m.astype(np.float64) for m in pkg.sh_rotation_matrices(q32)], tr.rotation_matrix(q32.astype(np.float64))


def test_the_matrices_equal_the_float64_restatement_whose_basis_is_the_renderers(pkg, oracle):
    """First the restatement's basis against np_reference and the oracle, then the matrices against the restatement.
    2^-23 per entry: one rounding to binary32 of an entry of magnitude <= 1 is 2^-25; the rest is room for the two
    least-squares solutions (64 fixed directions in the library, 500 random ones here), both exact to ~1e-15."""
    check_the_restated_basis_is_the_renderers(pkg, oracle)
    worst = 0.0
    for q in _rotations():
        got, R = _matrices(pkg, q)
        for g, w in zip(got, tr.sh_matrices(R)):
            assert g.shape == w.shape
            worst = max(worst, np.abs(g - w).max())
    print(f"max |M - float64 restatement| = {worst:.3g}")
    assert worst <= 2.0 ** -23


def test_the_matrices_are_orthogonal_compose_and_rotate_the_function(pkg):
    rots = _rotations()
    d = tr.directions(1000, seed=9)
    rng = np.random.default_rng(4)
    worst = dict(orthogonality=0.0, composition=0.0, function=0.0)
    for i, q in enumerate(rots):
        Ms, R = _matrices(pkg, q)
        q2 = rots[(7 * i + 3) % len(rots)]
        Ms2, R2 = _matrices(pkg, q2)
        prod = tr.quat_mul(tr.unit(np.asarray(q, np.float32).astype(np.float64)), tr.unit(np.asarray(q2, np.float32).astype(np.float64)))
        Ms12, R12 = _matrices(pkg, prod)
        assert np.abs(R12 - R @ R2).max() < 1e-6
        for l, (M, M2, M12) in enumerate(zip(Ms, Ms2, Ms12), start=1):
            m = 2 * l + 1
            worst["orthogonality"] = max(worst["orthogonality"], np.abs(M @ M.T - np.eye(m)).max())
            worst["composition"] = max(worst["composition"], np.abs(M @ M2 - M12).max())
            c = rng.normal(size=m)
            f_rotated = tr.basis(l, d) @ (M @ c)      # f'(d)
            f_there = tr.basis(l, d @ R) @ c          # f(R^T d)
            worst["function"] = max(worst["function"], np.abs(f_rotated - f_there).max() / np.abs(c).sum())
    print(worst)
    assert worst["orthogonality"] <= 1e-6 and worst["composition"] <= 1e-6 and worst["function"] <= 1e-5


def test_the_identity_gives_exact_identity_matrices(pkg):
    for q in ((1, 0, 0, 0), (-1, 0, 0, 0), (1e-20, 0, 0, 0), (3e19, 0, 0, 0)):
        for l, M in enumerate(pkg.sh_rotation_matrices(q), start=1):
            assert np.array_equal(M, np.eye(2 * l + 1, dtype=np.float32)), (q, l, M)
    # a rotation about an axis has the zeros of its block structure, exactly: band 1 is R itself in the order (-y, z, -x)
    M1 = pkg.sh_rotation_matrices((np.sqrt(0.5), 0, 0, np.sqrt(0.5)))[0]  # a quarter turn about z
    assert np.count_nonzero(M1) == 3 and M1[1, 1] == 1.0


# ---- the camera --------------------------------------------------------------------------------------------------------------
def test_the_transformed_camera_sees_the_transformed_world_as_before(pkg):
    """NDC of s R x + t through the new camera's uniforms = NDC of x through the old one's; view depth times s.  1e-5 relative (to
    the magnitude of the clip coordinates: binary32 uniforms built from binary32 camera members)."""
    rng = np.random.default_rng(21)
    x = np.concatenate([rng.uniform(-1.5, 1.5, size=(200, 2)), -rng.uniform(3, 9, size=(200, 1))], axis=1)  # in front of the cameras below (they look down -z)
    worst = 0.0
    for k in range(40):
        q, t, s = rng.normal(size=4), rng.uniform(-4, 4, size=3), float(rng.choice([1.0, 1.7, 0.4, 12.0]))
        cq = tr.unit(np.array([1.0, 0, 0, 0]) + 0.08 * rng.normal(size=4))
        cam = pkg.make_camera(position=rng.uniform(-0.5, 0.5, size=3), rotation=cq, fov=float(rng.uniform(30, 70)))
        cam2 = pkg.transform_camera(cam, q, t, s)
        pos, rot, near, far = tr.transform_camera(cam, q, t, s)
        assert np.abs(cam2["position"][0] - pos).max() <= 1e-6 * (1 + np.abs(pos).max())
        assert np.abs(cam2["rotation"][0] - rot).max() <= 1e-6
        assert cam2["fov"][0] == cam["fov"][0]
        assert abs(cam2["near_plane"][0] / near - 1) <= 1e-6 and abs(cam2["far_plane"][0] / far - 1) <= 1e-6
        qf, tf, sf = tr.params32(q, t, s)
        moved = sf * (x @ tr.rotation_matrix(qf).T) + tf
        u, u2 = pkg.camera_uniforms(cam, 128, 96), pkg.camera_uniforms(cam2, 128, 96)

        def project(u_, pts):
            P = u_["proj_mat"][0].astype(np.float64).reshape(4, 4).T  # column-major
            V = u_["view_mat"][0].astype(np.float64).reshape(4, 4).T
            ph = np.concatenate([pts, np.ones((len(pts), 1))], axis=1)
            clip, view = ph @ P.T, ph @ V.T
            return clip[:, :3] / clip[:, 3:4], view[:, 2]
        ndc, depth = project(u, x)
        ndc2, depth2 = project(u2, moved)
        assert (depth > 0.5).all()
        worst = max(worst, np.abs(ndc2 - ndc).max() / max(1.0, np.abs(ndc).max()), np.abs(depth2 / (sf * depth) - 1).max())
        assert u2["tan_fovx"][0] == u["tan_fovx"][0] and u2["tan_fovy"][0] == u["tan_fovy"][0]
    print(f"worst relative difference {worst:.3g}")
    assert worst <= 1e-5


# ---- the header on its own, under the sanitizers --------------------------------------------------------------------------------
def test_the_header_alone_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """tests/native/sh_rotation_sim.cpp is a program of its own: host code only, nothing of it is loaded into Python."""
    exe = str(tmp_path / "sh_rotation_sim")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",  # the runtimes inside the program: it runs in any environment as it is
                           "-I", os.path.join(ROOT, "3dgs.cpp_amd", "csrc"), os.path.join(ROOT, "tests", "native", "sh_rotation_sim.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith("ok"), run.stdout
