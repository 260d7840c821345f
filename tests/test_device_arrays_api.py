"""The device-array way into a scene (gs_scene_from_device_arrays / gs_scene_update_from_device_arrays), as far as a machine
without a GPU can check it: the symbols, every argument check of the C ABI (they run before a device is selected), the checks
Scene.from_tensors makes before it calls C, and -- on the CPU -- the premise of the ingest kernel's exp(): the device's
operation sequence equals this machine's libm expf on EVERY binary32 from +0 up to glibc's overflow bound.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from helpers import FakeTensor as _Fake, forbid_c

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gs_scene_from_device_arrays", "gs_scene_update_from_device_arrays", "gs_debug_activation_expf_scan")
GS_ERR_INVALID = -1
OVERFLOW_BITS = 0x42B17218  # the first binary32 above 0x1.62e42ep6f: glibc's expf returns +inf from here on


def test_the_three_symbols_are_declared_listed_and_exported(pkg):
    with open(os.path.join(ROOT, "include", "gs3d_hip.h")) as f:
        header = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    L = pkg.binding.lib()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), f"{name} is not declared in include/gs3d_hip.h"
        assert name in pkg.binding.SYMBOLS
        assert hasattr(L, name), f"{name} is not exported by libgs3d_hip.so"
    assert "gs_device_arrays;" in header


def _arrays(pkg, n=4, k=15, **override):
    """A gs_device_arrays over host memory (never dereferenced: every call below must fail before a device is touched)."""
    keep = dict(means=np.zeros((n, 3), np.float32), log_scales=np.zeros((n, 3), np.float32), quats=np.zeros((n, 4), np.float32),
                opacity_logits=np.zeros(n, np.float32), sh_dc=np.zeros((n, 3), np.float32), sh_rest=np.zeros((n, max(k, 1), 3), np.float32))
    a = pkg.binding.DeviceArrays()
    for name, arr in keep.items():
        setattr(a, name, arr.ctypes.data)
    a.sh_rest_coeffs = k
    for name, v in override.items():
        setattr(a, name, v)
    return a, keep


def _refused(pkg, rc):
    assert rc == GS_ERR_INVALID, rc
    msg = pkg.binding.lib().gs_last_error().decode()
    assert msg.strip(), "GS_ERR_INVALID without a message"
    return msg


def _build(pkg, a, n, out=True):
    h = C.c_void_p()
    return pkg.binding.lib().gs_scene_from_device_arrays(C.byref(a) if a is not None else None, C.c_uint64(n), C.c_int(0), None,
                                                         C.byref(h) if out else None)


def _update(pkg, scene, a, first, count):
    return pkg.binding.lib().gs_scene_update_from_device_arrays(scene, C.byref(a) if a is not None else None, C.c_uint64(first),
                                                                C.c_uint64(count), None)


def test_build_refuses_bad_arguments_before_it_selects_a_device(pkg):
    a, keep = _arrays(pkg)
    _refused(pkg, _build(pkg, None, 4))
    _refused(pkg, _build(pkg, a, 4, out=False))
    assert "2^31" in _refused(pkg, _build(pkg, a, 1 << 31))
    assert "2^31" in _refused(pkg, _build(pkg, a, (1 << 64) - 1))
    for k in (1, 2, 4, 7, 9, 14, 16, 45, 0xFFFFFFFF):
        assert "sh_rest_coeffs" in _refused(pkg, _build(pkg, _arrays(pkg, k=15, sh_rest_coeffs=k)[0], 4))
    for name in ("means", "log_scales", "quats", "opacity_logits", "sh_dc", "sh_rest"):
        b, keep_b = _arrays(pkg, **{name: None})
        assert name in _refused(pkg, _build(pkg, b, 4)), name
        for off in (1, 2, 3):
            b, keep_b = _arrays(pkg)
            setattr(b, name, getattr(b, name) + off)
            assert name in _refused(pkg, _build(pkg, b, 4)) and "aligned" in pkg.binding.lib().gs_last_error().decode()
    del keep


def test_update_refuses_bad_arguments_before_it_selects_a_device(pkg):
    a, keep = _arrays(pkg)
    _refused(pkg, _update(pkg, None, a, 0, 1))       # no scene
    _refused(pkg, _update(pkg, None, None, 0, 1))    # no arrays
    assert "sh_rest_coeffs" in _refused(pkg, _update(pkg, None, _arrays(pkg, sh_rest_coeffs=5)[0], 0, 1))
    b, keep_b = _arrays(pkg)
    b.quats += 2
    assert "quats" in _refused(pkg, _update(pkg, None, b, 0, 1))
    del keep, keep_b


def test_from_tensors_rejects_what_the_abi_cannot_take_without_reaching_c(pkg, monkeypatch):
    torch = pytest.importorskip("torch")
    forbid_c(pkg, monkeypatch)
    n = 8
    good = dict(means=_Fake((n, 3)), log_scales=_Fake((n, 3)), quats=_Fake((n, 4)), opacity_logits=_Fake((n, 1)), sh_dc=_Fake((n, 1, 3)),
                sh_rest=_Fake((n, 15, 3)))

    def build(**change):
        return pkg.Scene.from_tensors(**dict(good, **change))

    with pytest.raises(ValueError, match="CPU"):
        build(means=torch.zeros(n, 3))
    with pytest.raises(TypeError, match="float32"):
        build(means=torch.zeros(n, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="contiguous"):
        build(means=torch.zeros(3, n).T)
    with pytest.raises(ValueError, match="shape"):
        build(means=torch.zeros(n, 4))
    with pytest.raises(ValueError, match="shape"):
        build(sh_rest=_Fake((n, 14, 3)))
    with pytest.raises(ValueError, match="shape"):
        build(sh_rest=_Fake((n, 3, 15)))
    with pytest.raises(ValueError, match="rows"):
        build(quats=_Fake((n + 1, 4)))
    with pytest.raises(ValueError, match="device"):
        build(quats=_Fake((n, 4), device="cuda:1"))
    with pytest.raises(TypeError):
        build(means=np.zeros((n, 3), np.float32))  # host memory: no data_ptr
    with pytest.raises(TypeError, match="required"):
        build(sh_dc=None)
    with pytest.raises(AssertionError, match="reached"):  # ... and a good set of tensors does go on to C
        build()
    scene = pkg.Scene(None)
    with pytest.raises(ValueError, match="CPU"):
        scene.update_from_tensors(0, means=torch.zeros(n, 3))
    with pytest.raises(ValueError, match="rows"):
        scene.update_from_tensors(0, means=_Fake((n, 3)), opacity_logits=_Fake((n - 1,)))


def test_the_devices_exp_sequence_is_libm_on_every_binary32_from_zero_to_the_overflow_bound(oracle):
    """gs_expf_libm's operation sequence (the oracle's gso_expf_device restates it) was pinned on x <= 0 only.  The ingest
    kernel feeds it positive arguments (log-scales, -logits): it needs no other polynomial form up to glibc's overflow bound,
    and does need the explicit overflow branch above it."""
    bad, first = oracle.expf_device_mismatches(0, OVERFLOW_BITS + 1)
    assert bad == 0, (bad, hex(first))
    # without the branch the sequence is NOT libm further up (2^k leaves binary64's exponent range): from x = 710.4 on
    bad_above, first_above = oracle.expf_device_mismatches(OVERFLOW_BITS + 1, 0x7F800000 - OVERFLOW_BITS)
    assert bad_above > 0 and first_above > OVERFLOW_BITS, (bad_above, hex(first_above))
