"""gs_accumulate_densify_stats, gs_densify_plan and gs_densify_apply on the device, bit for bit against their restatement
(tests/densify_reference.py, formulation (a)); pkg.Adam.densify and reset_opacity end to end on the loop of INTEGRATION.md 3l."""
import ctypes as C
import math

import numpy as np
import pytest
import torch  # at collection, before the package loads its library: both must bind the same HIP runtime

import adam_step_reference as ar
import backward_cameras as bc
import composed_reference as comp
import densify_reference as dr
from test_adam_step_api import LR
from test_densify_api import INPUT_REFUSALS, OUTPUT_REFUSALS
from test_gpu_adam_step import device, records, same_bits
from test_gpu_device_arrays import once, raw_blob, same

pytestmark = pytest.mark.gpu

B = dr.BLOCK                 # k_densify_apply's parents per workgroup (gs_densify.hip: GS_DENSIFY_BLOCK)
T = dr.PARTITION             # the plan's partition: parents per workgroup of its scan (GS_DENSIFY_PARTITION)
GS_ERR_INVALID = -1


def upload(sc, offset=False):
    params = {k: device(v, offset=offset) for k, v in sc["params"].items()}
    state = dict(exp_avg={k: device(v, offset=offset) for k, v in sc["moments"]["exp_avg"].items()},
                 exp_avg_sq={k: device(v, offset=offset) for k, v in sc["moments"]["exp_avg_sq"].items()})
    stats = dict(grad_sum=device(sc["stats"]["grad_sum"], offset=offset), count=device(sc["stats"]["count"].view(np.int32), offset=offset),
                 max_radius=device(sc["stats"]["max_radius"], offset=offset))
    return params, state, stats, device(sc["noise"], offset=offset)


class Model:
    """What densify reads of a scene: its device and its Gaussian count (the scene itself is not touched)."""

    def __init__(self, n):
        self.device, self.num_vertices = 0, n


def check(pkg, sc, label, offset=False):
    """pkg.densify of the scene dict `sc` against formulation (a): the counts, both offset arrays, every parameter and moment; and the
    inputs keep their bits.  Returns (the reference's plan, the new parameters on the device)."""
    n = len(sc["params"]["means"])
    params, state, stats, noise = upload(sc, offset)
    inputs = list(params.values()) + list(state["exp_avg"].values()) + list(state["exp_avg_sq"].values()) + list(stats.values()) + [noise]
    was = [t.clone() for t in inputs]
    new, new_state, info = pkg.densify(Model(n), params, sc["rule"], stats, state, noise=noise)
    want, want_m, _, p = dr.densify(pkg, sc["params"], sc["moments"], sc["stats"], sc["rule"], sc["noise"])
    assert (info["n_out"], info["n_noise"]) == (p["n_out"], p["n_noise"]), (label, info["n_out"], info["n_noise"], p["n_out"], p["n_noise"])
    assert np.array_equal(info["row_offset"].cpu().numpy().view(np.uint32), p["row_offset"]), f"{label}: row_offset"
    assert np.array_equal(info["noise_offset"].cpu().numpy().view(np.uint32), p["noise_offset"]), f"{label}: noise_offset"
    assert info["parents_split"] == int(p["noisy"].sum()) and info["parents_removed"] == int((p["rows"] == 0).sum())
    assert info["parents_cloned"] == int(((p["rows"] == 2) & ~p["split"]).sum()) and info["parents_single"] == int((p["rows"] == 1).sum())
    assert set(new) == set(want) and set(new_state["exp_avg"]) == set(want_m["exp_avg"]) == set(new_state["exp_avg_sq"])
    for name in want:
        assert tuple(new[name].shape) == want[name].shape, (label, name)
        same_bits(new[name], want[name], f"{label}: {name}")
        for what in ("exp_avg", "exp_avg_sq"):
            if name in want_m[what]:
                same_bits(new_state[what][name], want_m[what][name], f"{label}: {what} of {name}")
    for t, old in zip(inputs, was):
        assert torch.equal(t.view(torch.uint8), old.view(torch.uint8)), f"{label}: an input changed"
    return p, new


# ------------------------------------------------------------------------------------------------ plan + apply
@pytest.mark.parametrize("n", [1, B - 1, B, B + 1, 3 * B + 7])
def test_plan_and_apply_are_the_references_bit_for_bit(pkg, gpu, _sort_path, n):
    once(_sort_path)
    for k in (0, 3, 8, 15):
        p, _ = check(pkg, dr.scene(pkg, n, seed=10 + k, k=k), f"n {n} k {k}")
        assert n < 3 * B or (p["n_noise"] > 0 and p["copy_only"].any() and set(p["rows"].tolist()) == {0, 1, 2})


@pytest.mark.parametrize("n", [T - 1, T, T + 1, T * B + T + 1], ids=["T-1", "T", "T+1", "every level"])
def test_the_scan_at_its_partition_edges_and_with_a_carry_between_the_turns_of_its_second_level(pkg, gpu, _sort_path, n):
    """T = GS_DENSIFY_PARTITION = 2048 parents per workgroup of the first and third level; the second level scans the partitions'
    sums 256 at a time with a carry, so T * 256 + T + 1 parents need 258 partitions: two turns, the carry, and a last partition of
    one parent."""
    once(_sort_path)
    k = 0 if n > 4 * T else 3
    p, _ = check(pkg, dr.scene(pkg, n, seed=21, k=k, with_moments=("means", "opacity_logits")), f"n {n}")
    assert p["n_out"] > n // 2 and p["n_noise"] > 0


def patterns(n):
    keep, clone, split = (np.full(n, c) for c in range(3))
    none = np.zeros(n, int)
    runs = np.concatenate([np.full(B + 9, 0), np.full(2 * B - 6, 2), np.full(n - 3 * B - 3, 1)])       # (pruned keeps, splits, clones)
    runs_pruned = np.concatenate([np.ones(B + 9, int), np.zeros(n - B - 9, int)])
    rng = np.random.default_rng(6)
    return {"all pruned": (rng.integers(0, 3, n), np.ones(n, int)), "all kept": (keep, none), "all cloned": (clone, none), "all split": (split, none),
            "alternating": (np.arange(n) % 3, (np.arange(n) % 2) * ((np.arange(n) // 2) % 4)),
            "runs longer than a workgroup": (runs, runs_pruned), "a random mix": (None, None)}


@pytest.mark.parametrize("pattern", list(patterns(3 * B + 7)))
def test_class_patterns_from_no_row_to_two_rows_per_parent(pkg, gpu, _sort_path, pattern):
    once(_sort_path)
    n = 3 * B + 7
    classes, pruned = patterns(n)[pattern]
    sc = dr.scene(pkg, n, seed=31, k=3, classes=classes, pruned=pruned)
    p, new = check(pkg, sc, pattern)
    if pattern == "all pruned":
        assert p["n_out"] == 0 and all(t.shape[0] == 0 for t in new.values())
    elif pattern == "all kept":
        assert p["n_out"] == n and all(np.array_equal(new[k].cpu().numpy().view(np.uint32), v.view(np.uint32)) for k, v in sc["params"].items())
    elif pattern == "all cloned":
        assert p["n_out"] == 2 * n and p["n_noise"] == 0
    elif pattern == "all split":
        assert p["n_out"] == 2 * n and p["n_noise"] == n
    elif pattern == "runs longer than a workgroup":
        tiles = [p["row_offset"][min(g + B, n)] - p["row_offset"][g] for g in range(0, n, B)]
        assert tiles[0] == 0 and tiles[2] == 2 * B, tiles      # a workgroup of the apply with no output row, one with 2 BLOCK


@pytest.mark.parametrize("radius, world", [(0.0, 0.0), (20.0, 0.0), (0.0, 0.5), (-1.0, -1.0)], ids=["off", "radius", "world", "negative = off"])
def test_each_prune_rule_on_and_off_absent_moment_pairs_and_slices_aligned_to_four_bytes_only(pkg, gpu, _sort_path, radius, world):
    once(_sort_path)
    r = dr.rule(max_screen_radius=radius, max_world_scale=world)
    sc = dr.scene(pkg, 2 * B + 3, seed=41, k=8, r=r, with_moments=("log_scales", "sh_rest", "quats"))
    p, _ = check(pkg, sc, f"radius {radius} world {world}", offset=True)
    assert p["copy_only"].any() == (radius > 0)
    params, _, stats, noise = upload(sc)
    _, none, _ = pkg.densify(Model(2 * B + 3), params, r, stats, None, noise=noise)      # no state at all
    assert none is None


def test_rows_exactly_on_a_threshold_and_a_nan_in_one_parent(pkg, gpu, _sort_path):
    once(_sort_path)
    sc, want, _ = dr.tie_scene(pkg)
    p, _ = check(pkg, sc, "ties")
    assert np.array_equal(p["rows"], want)
    sc = dr.scene(pkg, 2 * B, seed=8, k=3)
    victim = int(np.nonzero(dr.plan(pkg, sc["params"], sc["stats"], sc["rule"])["noisy"])[0][5])
    sc["params"]["means"][victim, 1] = np.nan
    sc["params"]["log_scales"][victim + 1, 0] = np.nan
    sc["stats"]["grad_sum"][victim + 2] = np.nan
    sc["moments"]["exp_avg"]["quats"][victim + 3, 2] = np.nan
    check(pkg, sc, "a NaN")            # (the reference's own test shows that its NaN stays in its parent's rows)


def test_the_result_is_the_same_bits_from_call_to_call_and_torchs_noise_is_drawn_when_none_is_given(pkg, gpu, _sort_path):
    once(_sort_path)
    sc = dr.scene(pkg, 3 * B, seed=12, k=3)
    params, state, stats, noise = upload(sc)
    a, am, _ = pkg.densify(Model(3 * B), params, sc["rule"], stats, state, noise=noise)
    b, bm, _ = pkg.densify(Model(3 * B), params, sc["rule"], stats, state, noise=noise)
    assert all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a)
    assert all(torch.equal(am[w][k].view(torch.int32), bm[w][k].view(torch.int32)) for w in am for k in am[w])
    torch.manual_seed(5)
    c, _, info = pkg.densify(Model(3 * B), params, sc["rule"], stats, state)
    torch.manual_seed(5)
    drawn = torch.randn((info["n_noise"], 2, 3), dtype=torch.float32, device="cuda")
    sc["noise"] = drawn.cpu().numpy()
    want = dr.densify(pkg, sc["params"], sc["moments"], sc["stats"], sc["rule"], sc["noise"])[0]
    same_bits(c["means"], want["means"], "torch.randn's draws")


# ------------------------------------------------------------------------------------------------ the statistic
def test_the_statistic_over_frames_of_two_cameras_and_two_sizes(pkg, gpu, _sort_path):
    n = 900
    scene = pkg.Scene.from_records(records(pkg, n))
    rend = pkg.Renderer(scene)
    stats = pkg.densify_stats_zeros(scene)
    assert stats["grad_sum"].dtype == torch.float64 and stats["count"].dtype == torch.int32 and stats["max_radius"].dtype == torch.float32
    assert all(tuple(t.shape) == (n,) and not t.any().item() for t in stats.values())
    with pytest.raises(pkg.binding.GsError, match="no frame rendered yet") as e:
        rend.densify_stats(torch.zeros(n, 2, dtype=torch.float64, device="cuda"), stats)
    assert e.value.code == GS_ERR_INVALID
    stats["grad_sum"].fill_(0.5), stats["count"].fill_(3), stats["max_radius"].fill_(2.0)      # what an invisible row must keep
    want = dict(grad_sum=np.full(n, 0.5), count=np.full(n, 3, np.uint32), max_radius=np.full(n, 2.0, np.float32))
    rng = np.random.default_rng(3)
    seen = np.zeros(n, int)
    for cam, (w, h) in (("C1", (64, 48)), ("C2", (64, 48)), ("C1", (40, 64))):
        rgba = torch.zeros(h, w, 4, device="cuda")
        torch.cuda.synchronize()
        rend.render(pkg.camera_uniforms(bc.camera(pkg, cam), w, h), rgba.data_ptr())
        rend.synchronize()
        uv = rend.blend_backward(device(rng.standard_normal((h, w, 3)).astype(np.float32)), uv=True)["uv"]
        tiles, radius = rend.stage("tiles"), rend.stage("radius")
        assert rend.densify_stats(uv, stats) is stats
        dr.accumulate_stats(want, uv.cpu().numpy(), tiles, radius, w, h)
        seen += tiles != 0
        same_bits(stats["grad_sum"], want["grad_sum"], f"{cam} {w}x{h}: grad_sum")
        assert np.array_equal(stats["count"].cpu().numpy().view(np.uint32), want["count"]) and np.array_equal(stats["max_radius"].cpu().numpy(), want["max_radius"])
    assert (seen == 0).any() and (seen >= 2).any() and (want["max_radius"] > 2).any()
    assert (want["count"][seen == 0] == 3).all() and (want["grad_sum"][seen == 0] == 0.5).all() and (want["count"] == 3 + seen).all()
    rend.close()
    scene.close()


# ------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_of_the_header_leaves_inputs_outputs_and_scratch_untouched(pkg, gpu, _sort_path):
    once(_sort_path)
    n = 300
    sc = dr.scene(pkg, n, seed=2, k=15)
    params, state, stats, noise = upload(sc)
    p = dr.plan(pkg, sc["params"], sc["stats"], sc["rule"])
    b, L = pkg.binding, pkg.binding.lib()
    scratch = torch.full((2 * (n + 1),), 7, dtype=torch.int32, device="cuda")
    outs = {name: torch.full((p["n_out"],) + v.shape[1:], 9.0, device="cuda") for name, v in sc["params"].items()}
    out_m = {what: {name: torch.full_like(outs[name], 9.0) for name in outs} for what in ("exp_avg", "exp_avg_sq")}

    def structs():
        i, o = b.DensifyInput(), b.DensifyOutput()
        for g, name in enumerate(dr.NAMES):
            setattr(i.params, name, params[name].data_ptr())
            setattr(o.params, name, outs[name].data_ptr())
            o.exp_avg[g], o.exp_avg_sq[g] = state["exp_avg"][name].data_ptr(), state["exp_avg_sq"][name].data_ptr()
            o.out_exp_avg[g], o.out_exp_avg_sq[g] = out_m["exp_avg"][name].data_ptr(), out_m["exp_avg_sq"][name].data_ptr()
        i.params.sh_rest_coeffs = o.params.sh_rest_coeffs = 15
        i.grad_sum, i.count, i.max_radius = (stats[k].data_ptr() for k in ("grad_sum", "count", "max_radius"))
        i.scratch, i.rule = scratch.data_ptr(), b._densify_rule(sc["rule"])
        o.noise, o.n_noise, o.n_out = noise.data_ptr(), p["n_noise"], p["n_out"]
        return i, o

    tensors = list(params.values()) + [t for d in (state, out_m) for m in d.values() for t in m.values()] + list(stats.values()) + list(outs.values()) + [noise, scratch]
    was = [t.clone() for t in tensors]
    n_out, n_noise = C.c_uint64(0), C.c_uint64(0)
    plan = lambda i: L.gs_densify_plan(C.byref(i), C.c_uint64(n), 0, None, C.byref(n_out), C.byref(n_noise))      # noqa: E731
    apply = lambda i, o: L.gs_densify_apply(C.byref(i), C.c_uint64(n), C.byref(o), 0, None)                        # noqa: E731
    torch.cuda.synchronize()
    for label, word, bend in INPUT_REFUSALS + OUTPUT_REFUSALS:
        i, o = structs()
        if label.startswith("n_") or "n_noise" in label:       # (the host test's counts are those of its four rows)
            continue
        bend(i, o)
        codes = [apply(i, o)] + ([plan(i)] if (label, word, bend) in INPUT_REFUSALS else [])
        assert codes == [GS_ERR_INVALID] * len(codes), label
        assert word in L.gs_last_error().decode(), (label, L.gs_last_error().decode())
    for member, value in (("n_out", 2 * n + 1), ("n_noise", n + 1), ("n_noise", p["n_out"] // 2 + 1)):
        i, o = structs()
        setattr(o, member, value)
        assert apply(i, o) == GS_ERR_INVALID, (member, value)
    i, o = structs()
    assert apply(i, o) == GS_ERR_INVALID and "plan" in L.gs_last_error().decode()        # the scratch is not a plan's: 7s
    torch.cuda.synchronize()
    for t, old in zip(tensors, was):
        assert torch.equal(t.view(torch.uint8), old.view(torch.uint8))
    assert plan(i) == 0 and (n_out.value, n_noise.value) == (p["n_out"], p["n_noise"])          # ... and the good structs do run
    for member, value in (("n_out", p["n_out"] - 1), ("n_noise", p["n_noise"] - 1)):            # counts that are not this plan's
        i2, o2 = structs()
        setattr(o2, member, value)
        assert apply(i2, o2) == GS_ERR_INVALID and "plan" in L.gs_last_error().decode()
    assert all(torch.equal(t.view(torch.uint8), old.view(torch.uint8)) for t, old in zip(tensors[:-1], was[:-1]))
    assert apply(i, o) == 0
    want, want_m, _ = dr.apply(pkg, sc["params"], sc["moments"], p, sc["noise"])
    for name in want:
        same_bits(outs[name], want[name], name)
        same_bits(out_m["exp_avg_sq"][name], want_m["exp_avg_sq"][name], f"exp_avg_sq of {name}")


# ------------------------------------------------------------------------------------------------ end to end
def test_three_steps_a_densify_and_one_more_step_are_the_references_and_the_scene_is_a_fresh_ingest(pkg, gpu):
    """The loop of INTEGRATION.md 3l at 64 x 48 on the 200 Gaussians of the geometry descent: three iterations with the statistic,
    Adam.densify under a rule whose thresholds are quantiles of the statistic (so that some of each class clone, split and are
    pruned), a new renderer, one more step.  That step's parameters and moments are adam_step_reference.step of formulation (a)'s
    output under the frame's gradients, bit for bit: the survivors' moments were carried, the new rows' were zero."""
    n, w, h = comp.RENDER_SCENE
    rec, target_rec = comp.geometry_records(pkg.synth)
    u = pkg.camera_uniforms(bc.camera(pkg, comp.GEOMETRY_CAMERA), w, h)
    rgba = torch.zeros(h, w, 4, device="cuda")
    torch.cuda.synchronize()
    target_scene = pkg.Scene.from_records(target_rec)
    target_rend = pkg.Renderer(target_scene)
    target_rend.render(u, rgba.data_ptr())
    target_rend.synchronize()
    target = rgba[..., :3].clone()
    target_rend.close()
    target_scene.close()
    params = {name: device(a) for name, a in ar.cut(rec).items()}
    scene = pkg.Scene.from_tensors(**params)
    rend = pkg.Renderer(scene)
    opt = pkg.Adam(scene, params, lr=LR)

    def iteration(rend, stats):
        grads = {name: torch.zeros_like(t, dtype=torch.float64) for name, t in opt.params.items()}
        rend.render(u, rgba.data_ptr())
        rend.synchronize()
        frame = rgba.clone()
        sums = rend.blend_backward((2.0 * (rgba[..., :3] - target)).contiguous(), colour=True, opacity=True, conic=True, uv=True)
        if stats is not None:
            rend.densify_stats(sums["uv"], stats)
        rend.project_backward(out=grads, **sums)
        mask = rend.visible_mask()
        consumed = {name: g.cpu().numpy() for name, g in grads.items()}
        opt.step(grads, mask=mask)
        return frame, consumed, mask.cpu().numpy()

    stats = pkg.densify_stats_zeros(scene)
    for _ in range(3):
        iteration(rend, stats)
    host = lambda d: {k: v.cpu().numpy() for k, v in d.items()}           # noqa: E731
    h_stats = host(stats)
    h_stats["count"] = h_stats["count"].view(np.uint32)
    assert (h_stats["count"] == 3).any() and (h_stats["count"] == 0).any()
    q = dr.quantities(pkg, host(opt.params), h_stats)
    seen = h_stats["count"] != 0
    r = dr.rule(grad_threshold=float(np.quantile(q["avg"][seen], 0.6)), dense_extent=float(np.median(q["s"][seen])),
                min_opacity=float(np.quantile(q["o"], 0.1)), max_screen_radius=float(np.quantile(q["radius"][seen], 0.95)))
    noise = device(np.random.default_rng(9).standard_normal((n, 2, 3)).astype(np.float32))
    before = dict(params=host(opt.params), moments={what: host(opt.state[what]) for what in opt.state})
    # an all-keep densify: the new scene's frame is the old scene's frame
    rend.render(u, rgba.data_ptr())
    rend.synchronize()
    old_frame, old_scene, t_was = rgba.clone(), opt.scene, opt.t
    kept = opt.densify(dr.rule(grad_threshold=1e30, min_opacity=0.0), stats)
    assert kept is opt.scene and kept is not old_scene and opt.densify_info["n_out"] == n and opt.t == t_was
    kept_rend = pkg.Renderer(kept)
    kept_rend.render(u, rgba.data_ptr())
    kept_rend.synchronize()
    assert torch.equal(rgba.view(torch.int32), old_frame.view(torch.int32)), "an all-keep densify changed the frame"
    for name in before["params"]:
        same_bits(opt.params[name], before["params"][name], f"all-keep: {name}")
        same_bits(opt.state["exp_avg"][name], before["moments"]["exp_avg"][name], f"all-keep: exp_avg of {name}")
    kept_rend.close()
    rend.close()
    old_scene.close()
    # the real one
    new_scene = opt.densify(r, stats, noise=noise)
    info = opt.densify_info
    print({k: v for k, v in info.items() if not k.endswith("offset")})
    want, want_m, _, p = dr.densify(pkg, before["params"], before["moments"], h_stats, r, noise.cpu().numpy())
    assert info["n_out"] == p["n_out"] == new_scene.num_vertices and info["n_noise"] == p["n_noise"]
    assert min(info["parents_removed"], info["parents_cloned"], info["parents_split"], info["parents_single"]) > 0, "the rule does not do some of each"
    fresh = pkg.Scene.from_tensors(**opt.params)
    same(raw_blob(new_scene), raw_blob(fresh), "the new scene's blob")
    fresh.close()
    kept.close()
    new_rend = pkg.Renderer(new_scene)
    _, consumed, mask = iteration(new_rend, pkg.densify_stats_zeros(new_scene))
    assert mask.any() and not mask.all()
    ar.step(want, consumed, want_m["exp_avg"], want_m["exp_avg_sq"], LR, ar.BETAS, ar.EPS, opt.t, mask=mask)
    for name in want:
        same_bits(opt.params[name], want[name], f"after the step: {name}")
        same_bits(opt.state["exp_avg"][name], want_m["exp_avg"][name], f"after the step: exp_avg of {name}")
        same_bits(opt.state["exp_avg_sq"][name], want_m["exp_avg_sq"][name], f"after the step: exp_avg_sq of {name}")
    # the opacity reset
    others = {name: t.clone() for name, t in opt.params.items() if name != "opacity_logits"}
    logits = opt.params["opacity_logits"].cpu().numpy()
    opt.reset_opacity(0.4)                     # (the rule above pruned the faint ones: a ceiling the remaining opacities straddle)
    cap = np.float32(math.log(0.4 / 0.6))
    assert (logits > cap).any() and (logits < cap).any()
    same_bits(opt.params["opacity_logits"], np.minimum(logits, cap), "reset_opacity")
    assert not opt.state["exp_avg"]["opacity_logits"].any().item() and not opt.state["exp_avg_sq"]["opacity_logits"].any().item()
    assert opt.state["exp_avg"]["means"].any().item()
    assert all(torch.equal(t.view(torch.int32), opt.params[name].view(torch.int32)) for name, t in others.items())
    fresh = pkg.Scene.from_tensors(**opt.params)
    same(raw_blob(new_scene), raw_blob(fresh), "the scene after reset_opacity")
    fresh.close()
    new_rend.close()
    new_scene.close()
