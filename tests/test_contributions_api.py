"""gs_accumulate_contributions / Renderer.contributions without a GPU: the yardstick the GPU tests compare with
(tests/contribution_reference.py) is pinned to the oracle's image bit for bit, its outputs are consistent with the lists, and the
entry point and its Python wrapper refuse what they must before anything touches a device."""
import ctypes as C

import numpy as np
import pytest

import contribution_reference as cref
from helpers import assert_images_identical, FakeTensor as _Fake, forbid_c, hand_made_renderer, oracle_frame

SCENES = {"A": (600, 80, 48), "T": (1500, 64, 64)}   # synth_records(n, seed=5, kind): n, width, height


@pytest.fixture(scope="module", params=sorted(SCENES))
def walked(request, pkg, oracle):
    n, w, h = SCENES[request.param]
    rec = pkg.synth.synth_records(n, seed=5, kind=request.param)
    _, _, ref = oracle_frame(oracle, rec, w, h)
    return request.param, w, h, ref, cref.contributions(oracle, ref, w, h)


def test_the_reference_walk_accumulates_the_oracles_image(walked):
    kind, w, h, ref, got = walked
    assert got["image"].shape == ref["image"].shape
    assert_images_identical(got["image"], ref["image"], label=f"contribution reference, kind {kind}")


def test_the_reference_outputs_agree_with_each_other_and_with_the_lists(walked):
    kind, w, h, ref, got = walked
    assert got["blended"] > 10000 and int(got["pixels"].sum(dtype=np.uint64)) == got["blended"]
    touched = got["pixels"] != 0
    assert touched.sum() > 300 and np.array_equal(touched, got["weight"] != 0)
    # 6 <= q < 2^24 per blended pixel
    assert (got["weight"][touched] >= 6 * got["pixels"][touched].astype(np.uint64)).all()
    assert (got["weight"][touched] < (got["pixels"][touched].astype(np.uint64) << np.uint64(24))).all()
    b = ref["boundaries"].astype(np.int64)
    tx = (w + 15) // 16
    picked = 0
    for y in range(h):
        for x in range(w):
            top = got["top_id"][y, x]
            if top == cref.NONE:
                continue
            t = (y // 16) * tx + x // 16
            assert top in ref["sorted_payload"][b[2 * t]:b[2 * t + 1]], (x, y, int(top))
            assert got["pixels"][top] > 0
            picked += 1
    assert picked > w * h // 4
    # a pixel has a top id exactly where something was blended: where the image is not black (the synthetic colours are > 0)
    assert np.array_equal(got["top_id"] != cref.NONE, ref["image"][..., :3].max(axis=2) > 0)


def test_a_mask_and_its_complement_split_the_reference(pkg, oracle):
    n, w, h = SCENES["A"]
    _, _, ref = oracle_frame(oracle, pkg.synth.synth_records(n, seed=5, kind="A"), w, h)
    whole = cref.contributions(oracle, ref, w, h)
    mask = np.zeros((h, w), np.uint8)
    mask[5:29, 11:43] = 1
    a, b = cref.contributions(oracle, ref, w, h, mask), cref.contributions(oracle, ref, w, h, 1 - mask)
    assert 0 < a["blended"] < whole["blended"]
    for k in ("weight", "pixels"):
        np.testing.assert_array_equal(a[k] + b[k], whole[k])
    np.testing.assert_array_equal(np.where(mask != 0, a["top_id"], b["top_id"]), whole["top_id"])
    assert (a["top_id"][mask == 0] == cref.NONE).all()
    assert_images_identical(a["image"], ref["image"], label="the mask gates what is recorded, not the walk")


def test_null_arguments_are_refused_without_a_device(pkg):
    L = pkg.binding.lib()
    c = pkg.binding.Contributions()
    assert L.gs_accumulate_contributions(None, C.byref(c)) == -1          # GS_ERR_INVALID
    assert L.gs_accumulate_contributions(None, None) == -1
    assert L.gs_accumulate_contributions(C.c_void_p(8), None) == -1       # (r is not dereferenced before c is checked)
    assert b"null" in L.gs_last_error()


def test_the_wrapper_checks_its_tensors_before_it_reaches_c(pkg, monkeypatch):
    forbid_c(pkg, monkeypatch)
    rend = hand_made_renderer(pkg, frame_hw=(48, 80))
    good = dict(weight=_Fake((100,), "torch.int64"), pixels=_Fake((100,), "torch.int32"), top_id=_Fake((48, 80), "torch.int32"),
                mask=_Fake((48, 80), "torch.uint8"))
    with pytest.raises(AssertionError, match="C library was reached"):   # everything in order: the call goes through to C
        rend.contributions(**good)
    with pytest.raises(AssertionError, match="C library was reached"):
        rend.contributions(**dict(good, mask=_Fake((48, 80), "torch.bool")))
    bad = [("weight", _Fake((100,), "torch.float32"), TypeError), ("weight", _Fake((100,), "torch.int32"), TypeError),
           ("pixels", _Fake((100,), "torch.int64"), TypeError), ("top_id", _Fake((48, 80), "torch.float32"), TypeError),
           ("mask", _Fake((48, 80), "torch.int32"), TypeError), ("weight", np.zeros(100, np.int64), TypeError),
           ("weight", _Fake((99,), "torch.int64"), ValueError), ("weight", _Fake((100, 1), "torch.int64"), ValueError),
           ("pixels", _Fake((101,), "torch.int32"), ValueError), ("top_id", _Fake((80, 48), "torch.int32"), ValueError),
           ("top_id", _Fake((48 * 80,), "torch.int32"), ValueError), ("mask", _Fake((48, 81), "torch.uint8"), ValueError),
           ("pixels", _Fake((100,), "torch.int32", contiguous=False), ValueError),
           ("top_id", _Fake((48, 80), "torch.int32", contiguous=False), ValueError),
           ("weight", _Fake((100,), "torch.int64", device="cpu"), ValueError),
           ("mask", _Fake((48, 80), "torch.uint8", device="cuda:1"), ValueError)]
    for name, tensor, error in bad:
        with pytest.raises(error, match=name):
            rend.contributions(**dict(good, **{name: tensor}))
