"""What every wrapper of binding.py that takes tensors answers to one bad tensor, without a GPU: from one good call per wrapper,
built from fake tensors, every tensor argument is replaced in turn by each single-fault variant of itself, and the exception's
class and text are compared with tests/golden/binding_refusals.json.  The table is generated, not written out: a check that is
fixed in one wrapper and missed in another, or a message that moves, shows here.

`python tests/test_binding_refusals.py` writes the fixture anew from the binding as it stands."""
import json
import os

import numpy as np
import pytest

from helpers import FakeTensor, forbid_c, hand_made_renderer

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "binding_refusals.json")
N, H, W, K, CHANNELS = 100, 40, 72, 15, 5
F32, F64 = "torch.float32", "torch.float64"
PARAMETERS = dict(means=(N, 3), log_scales=(N, 3), quats=(N, 4), opacity_logits=(N,), sh_dc=(N, 3), sh_rest=(N, K, 3))
RECORD = dict(colour=((N, 3), F64), opacity=((N,), F64), conic=((N, 3), F64), uv=((N, 2), F64))


def _parameters(dtype, prefix=""):
    return {prefix + name: (shape, dtype) for name, shape in PARAMETERS.items()}


# wrapper -> (the object it is a method of, the method, arguments that are no tensors, {argument: (shape, dtype)}); an argument
# "d.k" is the member k of the dict argument d
WRAPPERS = {
    "contributions": ("renderer", "contributions", {}, dict(weight=((N,), "torch.int64"), pixels=((N,), "torch.int32"),
                                                            top_id=((H, W), "torch.int32"), mask=((H, W), "torch.uint8"))),
    "feature_maps": ("renderer", "feature_maps", {}, dict(features=((N, CHANNELS), F32), out=((H, W, CHANNELS), F32), alpha=((H, W), F32),
                                                          depth=((H, W), F32), median_depth=((H, W), F32))),
    "lift_pixels": ("renderer", "lift_pixels", {}, dict(values=((H, W, CHANNELS), F32), out=((N, CHANNELS), F64), weight=((N,), F64),
                                                        mask=((H, W), "torch.uint8"))),
    "blend_backward": ("renderer", "blend_backward", {}, dict(grad_rgb=((H, W, 3), F32), grad_alpha=((H, W), F32), **RECORD)),
    "project_backward": ("renderer", "project_backward", {}, dict(RECORD, **_parameters(F64, "out."))),
    "camera_backward": ("renderer", "camera_backward", {}, dict(RECORD, view_mat=((16,), F64), proj_mat=((16,), F64),
                                                                camera_position=((3,), F64))),
    "photometric_loss": ("renderer", "photometric_loss", {}, dict(image=((H, W, 4), F32), target=((H, W, 3), F32), grad=((H, W, 3), F32),
                                                                  terms=((4,), F64))),
    "visible_mask": ("renderer", "visible_mask", {}, dict(out=((N,), "torch.uint8"))),
    "Scene.adam_step": ("scene", "adam_step", dict(lr=1e-3), dict(_parameters(F32, "params."), **_parameters(F64, "grads."),
                                                                   **_parameters(F32, "exp_avg."), **_parameters(F32, "exp_avg_sq."),
                                                                   mask=((N,), "torch.uint8"))),
    "Scene.to_tensors": ("scene", "to_tensors", {}, _parameters(F32, "out.")),
    "Scene.update_from_tensors": ("scene", "update_from_tensors", dict(first=0), _parameters(F32)),
}


def _faults(shape, dtype):
    """(label, tensor) of every single-fault variant of FakeTensor(shape, dtype)."""
    yield "not a tensor", np.zeros(shape)
    yield "dtype", FakeTensor(shape, "torch.float16")
    yield "rank + 1", FakeTensor(shape + (2,), dtype)
    yield "rank - 1", FakeTensor(shape[:-1], dtype)
    for axis in range(len(shape)):
        yield f"extent {axis}", FakeTensor(shape[:axis] + (shape[axis] + 1,) + shape[axis + 1:], dtype)
    yield "not contiguous", FakeTensor(shape, dtype, contiguous=False)
    yield "cpu", FakeTensor(shape, dtype, device="cpu")
    yield "device 1", FakeTensor(shape, dtype, device="cuda:1")


def _case_ids(wrapper):
    return [f"{wrapper}/{arg}/{label}" for arg, (shape, dtype) in WRAPPERS[wrapper][3].items() for label, _ in _faults(shape, dtype)]


def _answer(pkg, wrapper, tensors):
    """(exception class name, str(exception)) of the wrapper called with `tensors`; ("", "") if it returns."""
    owner, method, plain, _ = WRAPPERS[wrapper]
    rend = hand_made_renderer(pkg, n=N, frame_hw=(H, W))
    kwargs = dict(plain)
    for arg, t in tensors.items():
        outer, _, member = arg.partition(".")
        if member:
            kwargs.setdefault(outer, {})[member] = t
        else:
            kwargs[outer] = t
    try:
        getattr(rend if owner == "renderer" else rend.scene, method)(**kwargs)
    except Exception as e:  # noqa: BLE001 -- whatever is raised is what is recorded
        return [type(e).__name__, str(e)]
    return ["", ""]


def _answers(pkg, wrapper):
    """{case id: answer} of `wrapper`, and the answer to its good call."""
    spec = WRAPPERS[wrapper][3]
    good = {arg: FakeTensor(shape, dtype) for arg, (shape, dtype) in spec.items()}
    got = {}
    for arg, (shape, dtype) in spec.items():
        for label, bad in _faults(shape, dtype):
            got[f"{wrapper}/{arg}/{label}"] = _answer(pkg, wrapper, dict(good, **{arg: bad}))
    return got, _answer(pkg, wrapper, good)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("wrapper", sorted(WRAPPERS))
def test_every_single_fault_is_answered_as_recorded(pkg, monkeypatch, golden, wrapper):
    forbid_c(pkg, monkeypatch)
    got, good = _answers(pkg, wrapper)
    assert good == ["AssertionError", "the C library was reached"]      # the call the faults are bent from is a good one
    assert got and list(got) == _case_ids(wrapper)
    for case, answer in got.items():
        assert case in golden, f"{case}: not in the recorded table"
        assert answer == golden[case], case


def test_the_table_is_whole(golden):
    """Every wrapper, every tensor argument, every fault: a table that shrank quietly -- a wrapper dropped, a fault no longer
    generated -- is not the recorded one."""
    cases = [case for wrapper in WRAPPERS for case in _case_ids(wrapper)]
    assert len(cases) == len(set(cases)) > 0
    assert sorted(cases) == sorted(golden)
    assert len(WRAPPERS) == 11 and all(len(WRAPPERS[w][3]) > 0 for w in WRAPPERS)
    refused = [case for case, (kind, text) in golden.items() if kind in ("TypeError", "ValueError")]
    assert len(refused) > len(cases) // 2                               # (the recording is of refusals, not of a stub that raises)


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import __graft_entry__ as entry
    package, table = entry.load_package(), {}
    with pytest.MonkeyPatch.context() as patch:
        forbid_c(package, patch)
        for name in WRAPPERS:
            table.update(_answers(package, name)[0])
    with open(GOLDEN, "w") as f:
        json.dump(table, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(table)} cases -> {GOLDEN}")
