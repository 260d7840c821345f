"""float64 restatement of gs_scene_transform (include/gs3d_hip.h) for the tests: the rotation of a quaternion, the SH band
matrices by least squares over many directions, the transform of activated vertices, the transformed camera.  numpy only.

The basis is the one sh_to_rgb (gs_preprocess.hip) evaluates: its order, its signs, and its constants AS THE KERNEL HOLDS THEM
(binary32).  tests/test_scene_transform_api.py compares it with np_reference.preprocess's colour, so that it is the renderer's.
"""
import numpy as np

_C1 = float(np.float32(0.4886025119029199))
_C2 = [float(np.float32(v)) for v in (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)]
_C3 = [float(np.float32(v)) for v in (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154,
                                      -0.4570457994644658, 1.445305721320277, -0.5900435899266435)]
BANDS = {1: slice(1, 4), 2: slice(4, 9), 3: slice(9, 16)}  # coefficient indices j of band l (the DC term is j = 0)


def basis(l, d):
    """(K, 2l+1): the functions the coefficients of band l are multiplied with, at the unit directions d (K, 3)."""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    if l == 1:
        Y = [-_C1 * y, _C1 * z, -_C1 * x]
    elif l == 2:
        Y = [_C2[0] * x * y, _C2[1] * y * z, _C2[2] * (2 * z * z - x * x - y * y), _C2[3] * z * x, _C2[4] * (x * x - y * y)]
    else:
        Y = [_C3[0] * (3 * x * x - y * y) * y, _C3[1] * x * y * z, _C3[2] * (4 * z * z - x * x - y * y) * y,
             _C3[3] * z * (2 * z * z - 3 * x * x - 3 * y * y), _C3[4] * x * (4 * z * z - x * x - y * y), _C3[5] * (x * x - y * y) * z,
             _C3[6] * x * (x * x - 3 * y * y)]
    return np.stack(Y, axis=1)


def colour(sh, d):
    """sh (n, 16, 3) float64, d (n, 3) unit: the colour before the + 0.5 and the clamp, bands 1..3 only (no DC)."""
    out = np.zeros((len(sh), 3))
    for l, js in BANDS.items():
        out += np.einsum("nj,njc->nc", basis(l, d), sh[:, js, :])
    return out


def directions(k, seed=0):
    v = np.random.default_rng(seed).normal(size=(k, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def unit(q):
    q = np.asarray(q, np.float64)
    return q / np.linalg.norm(q)


def rotation_matrix(q):
    """R of the quaternion (w, x, y, z), normalised here."""
    w, x, y, z = unit(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def quat_mul(a, b):
    """Hamilton product a (x) b; a (4,), b (..., 4); w x y z."""
    aw, ax, ay, az = a
    bw, bx, by, bz = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], axis=-1)


def quat_conj(q):
    return np.asarray(q, np.float64) * np.array([1.0, -1.0, -1.0, -1.0])


def sh_matrices(R, k=500):
    """[M_1, M_2, M_3] of the rotation matrix R: least squares of Y(d) M = Y(R^T d) over k random directions (float64)."""
    d = directions(k, seed=12345)
    return [np.linalg.lstsq(basis(l, d), basis(l, d @ R), rcond=None)[0] for l in (1, 2, 3)]  # rows of d @ R are (R^T d)^T


def params32(rotation, translation, scale):
    """The transform as the C ABI receives it: binary32 members, read back as float64."""
    return (np.asarray(rotation, np.float32).astype(np.float64), np.asarray(translation, np.float32).astype(np.float64),
            float(np.float32(scale)))


def transform_vertices(verts, rotation, translation, scale, first=0, count=None):
    """float64 (n, 60) vertices with [first, first + count) moved, from (n, 60) vertices (position4 scale3 opacity rotation4 sh48)."""
    q, t, s = params32(rotation, translation, scale)
    v = np.array(np.asarray(verts).view(np.float32).reshape(-1, 60), np.float64)
    count = len(v) - first if count is None else count
    sel = slice(first, first + count)
    R = rotation_matrix(q)
    v[sel, 0:3] = s * (v[sel, 0:3] @ R.T) + t
    v[sel, 4:7] *= s
    r = quat_mul(unit(q), v[sel, 8:12])
    v[sel, 8:12] = r / np.linalg.norm(r, axis=1, keepdims=True)
    sh = v[sel, 12:60].reshape(-1, 16, 3)
    for M, js in zip(sh_matrices(R), BANDS.values()):
        sh[:, js, :] = np.einsum("ij,njc->nic", M, sh[:, js, :])
    v[sel, 12:60] = sh.reshape(-1, 48)
    return v


def transform_camera(cam, rotation, translation, scale):
    """(position, rotation, near, far) in float64 of the camera that sees the moved scene as `cam` (a CAMERA_DT record) saw it."""
    q, t, s = params32(rotation, translation, scale)
    R = rotation_matrix(q)
    return (s * R @ cam["position"][0].astype(np.float64) + t, quat_mul(unit(q), cam["rotation"][0].astype(np.float64)),
            s * float(cam["near_plane"][0]), s * float(cam["far_plane"][0]))


def inverse(rotation, translation, scale):
    """(rotation, translation, scale) of the inverse similarity, float64."""
    q, t, s = params32(rotation, translation, scale)
    R = rotation_matrix(q)
    return quat_conj(unit(q)), -(R.T @ t) / s, 1.0 / s


def compose(second, first):
    """The similarity `first` followed by `second`, each (rotation, translation, scale); float64."""
    q2, t2, s2 = params32(*second)
    q1, t1, s1 = params32(*first)
    return quat_mul(unit(q2), unit(q1)), s2 * rotation_matrix(q2) @ t1 + t2, s1 * s2


# the yardstick's inputs (tests/test_transform_invariance_yardstick.py, tests/test_gpu_scene_transform.py)
W, H = 128, 96
ROTATION = (0.61, -0.33, 0.52, 0.49)   # generic: no axis, no small angle
TRANSLATION = (0.7, -1.3, 0.45)
SCALES = (1.0, 1.7, 0.4)
CAMERA = dict(position=(0.15, -0.1, 0.2), rotation=(0.9950, 0.0600, -0.0700, 0.0400))  # a little off the default
CAP_MEAN, CAP_FRACTION, BEYOND = 2e-4, 0.02, 1e-3  # the device's caps: mean |d|, share of pixels beyond BEYOND


def frame_difference(img, ref):
    """(mean |d|, share of pixels beyond BEYOND, max |d|) of the RGB planes of two frames."""
    d = np.abs(np.asarray(img, np.float64)[..., :3] - np.asarray(ref, np.float64)[..., :3])
    return float(d.mean()), float((d.max(axis=2) > BEYOND).mean()), float(d.max())
