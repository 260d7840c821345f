"""The export (gs_deactivate_vertices, gs_write_ply, gs_scene_to_device_arrays, gs_scene_download_records, gs_scene_save_ply)
as far as a machine without a GPU can check it: the host's inverse activation against its numpy restatement
(tests/export_reference.py), the round trip through the activation, the PLY writer, and every argument check that must fail
before a device is selected.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import export_reference as ref
from helpers import FakeTensor as _Fake, forbid_c

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gs_deactivate_vertices", "gs_write_ply", "gs_scene_to_device_arrays", "gs_scene_download_records", "gs_scene_save_ply")
GS_ERR_INVALID, GS_ERR_IO = -1, -2
PROPERTIES = (["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"] + [f"f_rest_{k}" for k in range(45)] + ["opacity"]
              + [f"scale_{k}" for k in range(3)] + [f"rot_{k}" for k in range(4)])


def test_the_symbols_are_declared_listed_and_exported(pkg):
    with open(os.path.join(ROOT, "include", "gs3d_hip.h")) as f:
        header = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    L = pkg.binding.lib()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), f"{name} is not declared in include/gs3d_hip.h"
        assert name in pkg.binding.SYMBOLS
        assert hasattr(L, name), f"{name} is not exported by libgs3d_hip.so"
    assert "gs_device_arrays_out;" in header


# ---- the host function against the numpy restatement -------------------------------------------------------------------------
def _f(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


def edge_values():
    one, zero, inf = np.float32(1), np.float32(0), np.float32(np.inf)
    tiny = np.float32(np.finfo(np.float32).tiny)
    vals = [0.0, -0.0, np.inf, -np.inf, np.nan, -1.0, -1e-30, -1e-45, 1.0, 0.5, 2.0, 3.4028235e38, 1e-45, 2e-45, 1e-40, 1e-39,
            tiny, np.nextafter(tiny, zero), np.nextafter(tiny, one),                        # subnormal / normal boundary
            np.nextafter(zero, one), np.nextafter(zero, -one),                              # just inside / outside [0, 1] at 0
            np.nextafter(one, zero), np.nextafter(one, inf), np.nextafter(np.nextafter(one, zero), zero),  # .. at 1
            np.nextafter(np.float32(0.5), zero), np.nextafter(np.float32(0.5), one), 1.0 / 255.0, 0.99]
    return np.array(vals, np.float32)


def all_values():
    """Every edge, subnormals, 2^k for k = -149 .. 127, 2e5 patterns spread over all exponents (both signs, NaNs among them),
    and 1e5 patterns spread over the exponents of (0, 1)."""
    rng = np.random.default_rng(20)
    powers = np.ldexp(np.float32(1), np.arange(-149, 128)).astype(np.float32)
    subnormals = _f(rng.integers(1, 0x00800000, 2000, dtype=np.uint32))
    spread = _f(rng.integers(0, 1 << 32, 200_000, dtype=np.uint64).astype(np.uint32))
    unit = _f(rng.integers(0, 0x3F800000 + 1, 100_000, dtype=np.uint32))
    return np.concatenate([edge_values(), powers, subnormals, spread, unit]).astype(np.float32)


def vertices_of(values):
    """(n, 60) vertices whose three scales and opacity run through `values` (each value meets every one of the four slots)."""
    n = len(values)
    rng = np.random.default_rng(21)
    v = rng.standard_normal((n, 60)).astype(np.float32)
    v[:, 3] = 1.0
    for k, slot in enumerate((4, 5, 6, 7)):
        v[:, slot] = np.roll(values, k)
    return v


def test_the_host_inverse_equals_the_numpy_restatement(pkg):
    v = vertices_of(all_values())
    got = pkg.deactivate_vertices(v)
    want = ref.deactivate(pkg, v)
    ref.same_bits(got, want, "gs_deactivate_vertices against tests/export_reference.py")
    # the cases are what they claim to be
    assert np.isnan(want[:, 54:58]).any() and np.isposinf(want[:, 54:58]).any() and np.isneginf(want[:, 54:58]).any()
    assert (want[:, 3:6] == 0).all()


def test_edges_export_as_the_rule_states(pkg):
    e = edge_values()
    r = pkg.deactivate_vertices(vertices_of(e))
    scale, logit = r[:, 55], r[:, 54]
    for s, x in zip(e, scale):
        if s == 0:
            assert x == -np.inf
        elif s == np.inf:
            assert x == np.inf
        elif not s > 0:
            assert np.isnan(x)
        else:
            assert np.isfinite(x)
    for o, x in zip(np.roll(e, 3), logit):  # (vertices_of: slot 7 holds the values rolled by three)
        if o == 0:
            assert x == -np.inf
        elif o == 1:
            assert x == np.inf
        elif not 0 < o < 1:
            assert np.isnan(x)
        else:
            assert np.isfinite(x)


def test_log64_stays_within_its_stated_distance_of_libm(pkg):
    """1.5e-14 absolute over [e^-103, e^88] (the restatement; the host function equals it bit for bit, above)."""
    x = np.exp(np.random.default_rng(22).uniform(-103, 88, 400_000))
    assert np.abs(ref.log64(x) - np.log(x)).max() <= 1.5e-14


# ---- the round trip on images of the activation ------------------------------------------------------------------------------
def image_records(n=150_000):
    """Records with log-scales uniform in [-30, 20] plus a dense band in [-3, 3], logits in [-40, 17]."""
    rng = np.random.default_rng(23)
    r = rng.standard_normal((n, 62)).astype(np.float32)
    r[:, 3:6] = 0
    scales = rng.uniform(-30, 20, (n, 3))
    scales[n // 2:] = rng.uniform(-3, 3, (n - n // 2, 3))
    r[:, 55:58] = scales.astype(np.float32)
    r[:, 54] = rng.uniform(-40, 17, n).astype(np.float32)
    return r


def test_an_image_of_the_activation_reactivates_to_its_own_bits(pkg):
    """activate(deactivate(activate(r))) == activate(r), bit for bit in positions, scales, opacity and SH; no case left out.

    ROTATIONS are not bit for bit.  With u = 2^-24 (binary32's unit roundoff), a normalisation computes
    q_k = fl(r_k * fl(1 / fl(sqrt(dot)))), dot = fl(fl(fl(x x) + fl(y y)) + fl(fl(z z) + fl(w w))): every term of the dot
    product passes three roundings (its product, its pair's sum, the final sum), so dot = |r|^2 (1 + d), |d| <= 3 u, which the
    square root halves to 1.5 u; the square root, the reciprocal and the product add one rounding each.  The STORED quaternion
    therefore has |q| = 1 + a, |a| <= 4.5 u to first order.  The reload normalises it again: q'_k = q_k (1 + b) / (1 + a) with
    b bounded the same way, and near 1 the bound on b tightens -- the dot product's terms sum to 1 and lie below it (half-ulp
    u / 2 and less), and of sqrt(dot') and its reciprocal one lies below 1 -- to about 3.9 u.  If every rounding took its
    extreme with the same sign the two would add to a little over 8 u; they cannot (the extremes of the pair sums and of the
    final sum, of the square root and of the reciprocal exclude each other), and the bound asserted is 8 u |q_k| per
    component.  Measured on 4e6 quaternions: <= 4.8 u, 36 % of rows change at all.
    """
    r = image_records()
    v = pkg.activate_records(r)
    back = pkg.deactivate_vertices(v)
    again = pkg.activate_records(back)
    keep = [k for k in range(60) if not 8 <= k < 12]
    ref.same_bits(again[:, keep], v[:, keep], "activate(deactivate(activate(r)))")
    ref.rotations_within_bound(again[:, 8:12], v[:, 8:12], "reloaded rotations")
    ref.same_bits(back[:, 58:62], v[:, 8:12], "the rotation is exported as stored")
    ref.same_bits(back[:, 0:3], r[:, 0:3], "positions")
    ref.same_bits(back[:, 6:54], r[:, 6:54], "the SH reorder is activate_record's, inverted")
    moved = (again[:, 8:12] != v[:, 8:12]).any(axis=1).mean()
    print(f"rows whose rotation changed on reload: {100 * moved:.1f} %, worst "
          f"{(np.abs(again[:, 8:12].astype(np.float64) - v[:, 8:12]) / np.abs(v[:, 8:12])).max() * 2 ** 24:.2f} x 2^-24")


def test_a_value_that_is_no_image_gets_the_nearest_image(pkg):
    """A transformed scale (an image times a factor) and subnormals: the export's activation is at least as close to the stored
    value as the activation of either neighbour of the export."""
    rng = np.random.default_rng(24)
    s = (np.exp(rng.uniform(-12, 3, 20_000)) * 1.2345).astype(np.float32)
    s = np.concatenate([s, _f(rng.integers(1, 0x00800000, 2000, dtype=np.uint32))])
    x = ref.log_scales(pkg, s)
    ref.same_bits(pkg.deactivate_vertices(vertices_of(s))[:, 55], x, "log-scales")
    err = lambda c: np.abs(ref._activated(pkg, 55, 4, c).astype(np.float64) - s.astype(np.float64))  # noqa: E731
    assert (err(x) <= err(ref.neighbour(x, 1))).all() and (err(x) <= err(ref.neighbour(x, -1))).all()


# ---- the PLY writer ----------------------------------------------------------------------------------------------------------
def header_of(path):
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    return data[:end].decode("ascii"), len(data)


@pytest.mark.parametrize("n", [0, 1, 777])
def test_write_ply_then_read_ply_is_bit_identical(pkg, tmp_path, n):
    r = pkg.synth.synth_records(n, seed=5, kind="A") if n else np.zeros((0, 62), np.float32)
    if n:
        r[0, 3:6] = [np.nan, np.inf, -0.0]  # records are bytes to the writer
    path = tmp_path / "out.ply"
    pkg.write_ply(path, r)
    header, size = header_of(path)
    lines = header.split("\n")
    # exactly the layout gs_ply.cpp's parse_ply_header calls `standard`: 62 float properties under the reference's names, in its order
    assert lines[:3] == ["ply", "format binary_little_endian 1.0", f"element vertex {n}"]
    assert lines[3:-2] == [f"property float {name}" for name in PROPERTIES] and lines[-2:] == ["end_header", ""]
    assert size == len(header) + 248 * n
    back = pkg.read_ply(path)
    assert back.shape == (n, 62) and np.array_equal(back.view(np.uint32), r.view(np.uint32))


def test_write_ply_to_an_unwritable_path_is_an_io_error_and_leaves_no_file(pkg, tmp_path):
    r = pkg.synth.synth_records(10, seed=5, kind="A")
    L = pkg.binding.lib()
    for bad in (tmp_path / "no_such_directory" / "out.ply", tmp_path):  # a missing directory; a directory
        rc = L.gs_write_ply(os.fsencode(bad), r.ctypes.data_as(C.c_void_p), C.c_uint64(len(r)))
        assert rc == GS_ERR_IO, rc
        assert L.gs_last_error().decode().strip()
        assert not os.path.isfile(bad)
    if os.path.exists("/dev/full"):  # the header is buffered, the records are not: the write itself fails
        big = pkg.synth.synth_records(20_000, seed=5, kind="A")
        link = tmp_path / "full.ply"
        os.symlink("/dev/full", link)
        rc = L.gs_write_ply(os.fsencode(link), big.ctypes.data_as(C.c_void_p), C.c_uint64(len(big)))
        assert rc == GS_ERR_IO and not os.path.lexists(link)


# ---- argument checks that must fail before a device is selected --------------------------------------------------------------
def _refused(pkg, rc):
    assert rc == GS_ERR_INVALID, rc
    msg = pkg.binding.lib().gs_last_error().decode()
    assert msg.strip(), "GS_ERR_INVALID without a message"
    return msg


def _out_arrays(pkg, n=4, k=15, **override):
    """A gs_device_arrays_out over host memory (never dereferenced: every call below must fail before a device is touched)."""
    keep = dict(means=np.zeros((n, 3), np.float32), log_scales=np.zeros((n, 3), np.float32), quats=np.zeros((n, 4), np.float32),
                opacity_logits=np.zeros(n, np.float32), sh_dc=np.zeros((n, 3), np.float32), sh_rest=np.zeros((n, max(k, 1), 3), np.float32))
    a = pkg.binding.DeviceArrays()
    for name, arr in keep.items():
        setattr(a, name, arr.ctypes.data)
    a.sh_rest_coeffs = k
    for name, v in override.items():
        setattr(a, name, v)
    return a, keep


def test_the_device_entry_points_refuse_bad_arguments_before_they_select_a_device(pkg):
    L = pkg.binding.lib()
    a, keep = _out_arrays(pkg)
    to_arrays = lambda s, arrays, first=0, count=1: L.gs_scene_to_device_arrays(  # noqa: E731
        s, C.byref(arrays) if arrays is not None else None, C.c_uint64(first), C.c_uint64(count), None)
    _refused(pkg, to_arrays(None, a))       # no scene
    _refused(pkg, to_arrays(None, None))    # no arrays
    for k in (1, 2, 4, 7, 9, 14, 16, 45, 0xFFFFFFFF):
        assert "sh_rest_coeffs" in _refused(pkg, to_arrays(None, _out_arrays(pkg, sh_rest_coeffs=k)[0]))
    for name in ("means", "log_scales", "quats", "opacity_logits", "sh_dc", "sh_rest"):
        for off in (1, 2, 3):
            b, keep_b = _out_arrays(pkg)
            setattr(b, name, getattr(b, name) + off)
            assert name in _refused(pkg, to_arrays(None, b)) and "aligned" in L.gs_last_error().decode()
    out = np.zeros((1, 62), np.float32)
    _refused(pkg, L.gs_scene_download_records(None, C.c_uint64(0), C.c_uint64(1), out.ctypes.data_as(C.c_void_p)))
    _refused(pkg, L.gs_scene_save_ply(None, b"/nonexistent/out.ply"))
    _refused(pkg, L.gs_write_ply(None, out.ctypes.data_as(C.c_void_p), C.c_uint64(1)))
    _refused(pkg, L.gs_write_ply(b"/nonexistent/out.ply", None, C.c_uint64(1)))
    _refused(pkg, L.gs_deactivate_vertices(None, C.c_uint64(1), out.ctypes.data_as(C.c_void_p)))
    assert L.gs_deactivate_vertices(None, C.c_uint64(0), None) == 0
    del keep


def test_to_tensors_checks_out_before_it_reaches_c(pkg, monkeypatch):
    forbid_c(pkg, monkeypatch)
    scene = pkg.Scene(None)
    n = 8
    with pytest.raises(TypeError, match="float32"):
        scene.to_tensors(0, n, out=dict(means=_Fake((n, 3), dtype="float64")))
    with pytest.raises(ValueError, match="contiguous"):
        scene.to_tensors(0, n, out=dict(means=_Fake((n, 3), contiguous=False)))
    with pytest.raises(ValueError, match="shape"):
        scene.to_tensors(0, n, out=dict(quats=_Fake((n, 3))))
    with pytest.raises(ValueError, match="shape"):
        scene.to_tensors(0, n, out=dict(sh_rest=_Fake((n, 14, 3))))
    with pytest.raises(ValueError, match="device"):
        scene.to_tensors(0, n, out=dict(means=_Fake((n, 3), device="cuda:1")))
    with pytest.raises(ValueError, match="rows"):
        scene.to_tensors(0, n, out=dict(means=_Fake((n, 3)), quats=_Fake((n + 1, 4))))
    with pytest.raises(ValueError, match="rows"):
        scene.to_tensors(0, n, out=dict(means=_Fake((n + 1, 3))))
    with pytest.raises(TypeError, match="unknown"):
        scene.to_tensors(0, n, out=dict(positions=_Fake((n, 3))))
    with pytest.raises(ValueError, match="sh_degree"):
        scene.to_tensors(0, n, sh_degree=4)
    with pytest.raises(AssertionError, match="reached"):  # ... and a good `out` does go on to C
        scene.to_tensors(0, n, out=dict(means=_Fake((n, 3)), sh_rest=_Fake((n, 8, 3))))
