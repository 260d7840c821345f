"""The cameras of the backward passes' tests, defined once (tests/test_backward_cameras_api.py, tests/test_gpu_backward_cameras.py).

`default` is the camera every earlier test of gs_blend_backward, gs_project_backward and Renderer.differentiable_render looks
through: at the origin, identity rotation, fov 45.  Its view matrix is diag(1, -1, -1, 1) -- a symmetric rotation block, no
translation -- and its camera_position is (0, 0, 0), so a transposed view matrix, a view direction taken from p instead of
p - camera_position and any slip in the translation column leave every bit unchanged under it.  C1 and C2 are moved and rotated
about all three axes: the rotation block of their view matrices is asymmetric by 0.38 and more.  They are mild enough that the
synthetic scenes stay in view (a harsher camera leaves scene A ten visible Gaussians).  A plain module: numpy only."""
import numpy as np


def _unit(q):
    q = np.asarray(q, np.float64)
    return tuple(float(v) for v in q / np.linalg.norm(q))


CAMERAS = {
    "default": dict(position=(0.0, 0.0, 0.0), rotation=(1.0, 0.0, 0.0, 0.0), fov=45.0),
    "C1": dict(position=(0.1, 0.05, -0.3), rotation=_unit((0.95, -0.1, 0.15, 0.2)), fov=60.0),
    "C2": dict(position=(-0.2, 0.1, 0.1), rotation=_unit((0.97, 0.1, 0.1, -0.15)), fov=35.0),
}
MOVED = ("C1", "C2")
# the branch scene is moved together with its camera (the default one): C1's rotation and a translation
BRANCH_MOVE = dict(rotation=CAMERAS["C1"]["rotation"], translation=(0.4, -0.25, 0.6), scale=1.0)


def camera(module, name):
    """The CAMERA_DT record of camera `name`; module: the package or the oracle (make_camera / default_camera)."""
    make = getattr(module, "make_camera", None) or module.default_camera
    return make(**CAMERAS[name])


def view_block(u):
    """The 3 x 3 rotation block of a uniforms record's view matrix as [row][column], float64."""
    u = u[0] if getattr(u, "shape", ()) else u
    return np.asarray(u["view_mat"], np.float64).reshape(4, 4).T[:3, :3]


def assert_conditions(u, visible, binds, label=""):
    """What a moved camera must give a frame for the tests to mean anything: at least a quarter of the scene visible, a clamp that
    binds on each axis, a view rotation asymmetric by more than 0.1, a camera away from the origin."""
    u0 = u[0] if getattr(u, "shape", ()) else u
    V = view_block(u)
    assert np.abs(V - V.T).max() > 0.1, (label, V)
    assert np.abs(np.asarray(u0["camera_position"], np.float64).reshape(-1)[:3]).max() > 0, label
    assert 4 * int(np.sum(visible)) >= len(visible), (label, int(np.sum(visible)), len(visible))
    assert np.asarray(binds)[:, 0].any() and np.asarray(binds)[:, 1].any(), (label, np.asarray(binds).sum(axis=0))
