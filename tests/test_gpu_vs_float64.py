"""The HIP path against the float64 restatement (np_reference.py) on the named edge scenes of float64_cases.py, with the same
checker as the oracle's CPU test (float64_check.assert_matches_float64): every stage tap, the image in exp mode 2 and in the
library's default mode 3, and the BGRA8 frame -- and, for view_sphere and opaque_cores, the frames again from binary16 SH
storage against the binary16 float64 inputs.  HIP == oracle bit for bit on each frame as well, which tells a kernel bug
apart from a disagreement between the oracle and float64.  Needs tests/ and numpy only."""
import dataclasses

import numpy as np
import pytest

import float64_cases as fc
import float64_check as chk
from helpers import assert_images_identical, compare_stages, oracle_frame

pytestmark = pytest.mark.gpu

SH16_CASES = ("view_sphere", "opaque_cores")


def _check_frame(pkg, oracle, scene, fr, verts_sh16=False):
    cam = dict(position=fr.position, rotation=fr.rotation, fov=fr.fov)
    rec = fr.records
    verts, u_ref, ref = oracle_frame(oracle, rec, fr.width, fr.height, oracle.default_camera(**cam))
    if verts_sh16:
        verts["sh"] = verts["sh"].astype(np.float16).astype(np.float32)
        ref = oracle.stages(verts, u_ref)
    rend = pkg.Renderer(scene)
    try:
        return _check_render(pkg, oracle, rend, fr, cam, u_ref, ref)
    finally:
        rend.close()


def _check_render(pkg, oracle, rend, fr, cam, u_ref, ref):
    u = pkg.camera_uniforms(pkg.make_camera(**cam), fr.width, fr.height)
    assert u.tobytes() == u_ref.tobytes()
    img, bgra = rend.render_host(u, want_rgba=True, want_bgra=True)
    # HIP == oracle, bit for bit -- its verdict is reported with the float64 check's, so that a failure says which side moved
    try:
        compare_stages(pkg, rend, u, ref)
        assert_images_identical(img, ref["image"], label=f"{fr.label}: HIP vs oracle")
        np.testing.assert_array_equal(bgra, oracle.pack_bgra8(ref["image"]))
        vs_oracle = None
    except AssertionError as e:
        vs_oracle = e
    # HIP against float64: every tap, the exp mode 2 image, the BGRA8 frame
    out = chk.outputs_from_hip(rend, u, img, bgra)
    try:
        rep = chk.assert_matches_float64(out, fr, label=f"{fr.label} (HIP, exp mode 2)")
    except chk.Mismatch as e:
        raise chk.Mismatch(f"{e}\n  HIP vs oracle: {'bit-identical' if vs_oracle is None else f'differ too: {vs_oracle}'}") from None
    if vs_oracle is not None:
        raise AssertionError(f"{fr.label}: HIP agrees with float64 but not with the oracle bit for bit: {vs_oracle}")
    # the library's default blend, exp mode 3
    rend.set_exp_mode(3)
    try:
        img3, _ = rend.render_host(u)
    finally:
        rend.set_exp_mode(2)
    rep3 = chk.assert_matches_float64(dict(out, image=img3, bgra=None), fr, label=f"{fr.label} (HIP, exp mode 3)")
    return rep, rep3


@pytest.mark.parametrize("name", list(fc.CASES))
def test_hip_matches_float64(pkg, oracle, gpu, name):
    case = fc.build(name)
    frames = [(fr, False) for fr in case.frames]
    if name in SH16_CASES:
        frames += [(dataclasses.replace(fr, label=fr.label + " (binary16 SH)", sh16=True), True) for fr in case.frames]
    scenes = {}
    try:
        for fr, sh16 in frames:
            key = (id(fr.records), sh16)
            if key not in scenes:
                scenes[key] = pkg.Scene.from_records(fr.records, device=0)
                if sh16:
                    scenes[key].quantize_sh()
            rep, rep3 = _check_frame(pkg, oracle, scenes[key], fr, verts_sh16=sh16)
            print(f"{fr.label}: explained pixels mode 2 {rep['explained_pixels']}, mode 3 {rep3['explained_pixels']} (cap "
                  f"{fr.max_explained}); explained radius/box/visibility {rep['radius_explained']}/{rep['box_explained']}/"
                  f"{rep['visibility_explained']}; BGRA8 steps {rep['bgra_explained']}")
    finally:
        for s in scenes.values():
            s.close()
