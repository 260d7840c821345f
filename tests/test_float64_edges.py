"""The C oracle (and the reference's shader text, where oracle/_ref is built) against the float64 restatement on the named
edge scenes of float64_cases.py -- and the check's own power: every perturbation of a shader rule in MUTATIONS, applied to
the float64 reference, must make the check fail on at least one case.  (The GPU side: tests/test_gpu_vs_float64.py.)"""
import dataclasses

import numpy as np
import pytest

import float64_cases as fc
import float64_check as chk
import np_reference as npr

# rule perturbations the check must notice: name -> rules override.  The last four passed the single-scene check of
# test_oracle_vs_numpy.py unnoticed.
MUTATIONS = {
    "near 0.2 -> 0.198": dict(near=0.198),
    "near 0.2 -> 0.202": dict(near=0.202),
    "frustum 1.3 -> 1.28": dict(frustum=1.28),
    "dilation 0.3 -> 0.29": dict(dilation=0.29),
    "floor 0.1 -> 0": dict(floor=0.0),
    "floor 0.1 -> 0.12": dict(floor=0.12),
    "radius 3 -> 2.98": dict(radius=2.98),
    "tile +15 -> +16": dict(tile_round=16),
    "uv -1 -> 0": dict(uv_offset=0.0),
    "alpha max 0.99 -> 0.995": dict(alpha_max=0.995),
    "alpha max 0.99 -> 0.985": dict(alpha_max=0.985),
    "alpha min 1/255 -> 1/254": dict(alpha_min=1.0 / 254.0),
    "T cut x0.5": dict(T_cut=0.5e-4),
    "T cut x2": dict(T_cut=2e-4),
    "clamp red only -> all channels": dict(clamp_channels=(0, 1, 2)),
    "clamp red only -> none": dict(clamp_channels=()),
    "ties id ascending -> descending": dict(tie=-1),
    "int() beyond int32: saturate -> wrap": dict(f2i="wrap"),
    "near 0.2 -> 0.1": dict(near=0.1),
    "near 0.2 -> 0.5": dict(near=0.5),
    "alpha max 0.99 -> 0.999": dict(alpha_max=0.999),
}


def frame_stages(o, fr, stages=None):
    verts = o.activate_records(fr.records)
    if fr.sh16:
        verts["sh"] = verts["sh"].astype(np.float16).astype(np.float32)
    u = o.camera_uniforms(o.default_camera(fr.position, fr.rotation, fr.fov), fr.width, fr.height)
    return (stages or o.stages)(verts, u)


@pytest.fixture(scope="module")
def cases():
    return {name: fc.build(name) for name in fc.CASES}


@pytest.fixture(scope="module")
def oracle_outputs(oracle, cases):
    out = {}
    for case in cases.values():
        for fr in case.frames:
            st = frame_stages(oracle, fr)
            o = chk.outputs_from_oracle(oracle, st)
            o["bgra"] = oracle.pack_bgra8(st["image"])
            out[fr.label] = o
    return out


@pytest.mark.parametrize("name", list(fc.CASES))
def test_oracle_matches_float64(cases, oracle_outputs, name):
    case = cases[name]
    for fr in case.frames:
        rep = chk.assert_matches_float64(oracle_outputs[fr.label], fr)
        worst = ", ".join(f"{k} {v:.2f}" for k, v in rep["worst_bound_ratio"].items())
        print(f"{fr.label}: explained pixels {rep['explained_pixels']} (cap {fr.max_explained}), explained radius/box/visibility "
              f"{rep['radius_explained']}/{rep['box_explained']}/{rep['visibility_explained']}, BGRA8 steps {rep['bgra_explained']}, "
              f"worst error / bound: {worst}")
    for mutation, least in case.mutations:
        total = dict(gaussians=0, entries=0, pixels=0)
        for fr in case.frames:
            ex = chk.exercise(fr, mutation)
            for k in total:
                total[k] += ex[k]
        n = sum(total.values())
        print(f"{name}: exercise count under {mutation}: {total} = {n} (at least {least})")
        assert n >= least, f"{name} no longer exercises {mutation}: {total}"


@pytest.mark.parametrize("name", list(fc.CASES))
def test_reference_text_matches_float64(pkg, oracle, cases, name):
    import __graft_entry__ as entry
    ref = entry.load_ref()
    if not ref.available():
        pytest.skip("oracle/_ref is not built and the reference tree is not mounted")
    for fr in cases[name].frames:
        fr = defined_for_glsl(fr)
        st = frame_stages(oracle, fr, ref.stages)
        chk.assert_matches_float64(chk.outputs_from_oracle(oracle, st), fr)


def defined_for_glsl(fr):
    """The frame without the Gaussians whose tile box converts a value beyond int32 to int: GLSL leaves that undefined, and
    the reference text compiled for the CPU gives INT_MIN there (a straddling box then counts ~2^32 tiles).  The pipeline and
    the oracle saturate; test_oracle_matches_float64 and the GPU test check them on these Gaussians."""
    pre = npr.preprocess(npr.activate(fr.records, fr.sh16), fr.camera64())
    keep = ~(np.abs(npr.box_args(pre["uv"], pre["radius"])) >= 2.0 ** 31 * 0.99).any(axis=1)
    return fr if keep.all() else dataclasses.replace(fr, records=fr.records[keep])


def test_every_rule_perturbation_is_caught(cases, oracle_outputs):
    """The check has teeth: the oracle's frames, checked against the float64 reference with one rule perturbed, fail on at
    least one case -- for every perturbation (a rule of the shaders the edge cases would not notice being wrong in the
    oracle and the stand-ins alike would pass here)."""
    missed, caught = [], {}
    for label, rules in MUTATIONS.items():
        # the case a rule is named after first, then the rest
        order = sorted(cases.values(), key=lambda c: not any(set(rules) & set(m) for m, _ in c.mutations))
        for case in order:
            for fr in case.frames:
                try:
                    chk.assert_matches_float64(oracle_outputs[fr.label], fr, rules=rules)
                except chk.Mismatch as e:
                    caught[label] = (fr.label, str(e).split(":")[1].strip()[:70])
                    break
            if label in caught:
                break
        else:
            missed.append(label)
    for label, (where, what) in caught.items():
        print(f"caught  {label:34s} on {where:28s} {what}")
    assert not missed, f"perturbations the float64 check does not notice: {missed}"


def test_bgra8_quantisation_against_the_oracles_conversion(oracle):
    """np_reference.bgra8 (float64) against gso_pack_bgra8 (the reference's UNORM conversion restated): equal everywhere but
    where binary32's x * 255 rounds onto a half-integer that float64 does not see as one."""
    rng = np.random.default_rng(7)
    k = np.arange(256, dtype=np.float64)
    vals = np.concatenate([rng.uniform(-0.2, 1.2, 40000), k / 255.0, (k + 0.5) / 255.0,
                           np.nextafter(((k + 0.5) / 255.0).astype(np.float32), np.float32(2)).astype(np.float64),
                           np.nextafter(((k + 0.5) / 255.0).astype(np.float32), np.float32(-2)).astype(np.float64),
                           [0.0, -0.0, 1.0, -1e30, 1e30, np.inf, -np.inf, np.nan]])
    vals = vals[: len(vals) // 4 * 4].astype(np.float32)
    rgba = vals.reshape(-1, 1, 4)
    got = oracle.pack_bgra8(rgba)
    want = npr.bgra8(rgba.astype(np.float64))
    tie = npr.bgra8_tie(rgba.astype(np.float64), 2.0 ** -23)
    assert np.array_equal(got[~tie], want[~tie])
    assert np.abs(got.astype(int) - want.astype(int)).max() <= 1
    assert want[..., 2].max() == 255 and want.min() == 0
