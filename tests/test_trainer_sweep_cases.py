"""The drawn cases of tests/trainer_sweep_cases.py cover what the sweep is for, asserted on the oracle's frames with no GPU -- as
tests/test_limit_scenes.py does for tests/limit_scenes.py.  If a condition below is not met, the draw or the seed range changes,
not the condition.  Three things are pinned:

  COVERAGE    over the default seeds and WIDE: frames narrower and lower than a tile, a single Gaussian, frames with nearly none
              and with every Gaussian visible, a per-tile list beyond 8 chunks of 64, a Gaussian with more than 1024 blend terms,
              one listed in more than 20 tiles, both clamps binding, red at zero, every K, every switch in both positions, WIDE
              frames of 100 tiles and more.
  EXCLUSIONS  trainer_sweep_cases.ill_conditioned -- the one predicate by which the device comparison of project_backward and
              camera_backward may leave a Gaussian out -- removes at most 0.5 % of the sweep's visible Gaussians and none in at
              least 20 of the 24 default cases.
  TEETH       for each kernel error the sweep is meant to notice, some sweep case puts the reference bent that way outside the
              unbent reference's own bound by a factor of 10 or more; a device within one bound of the true reference then lies
              at least 9 bounds from the bent one."""
import numpy as np
import pytest

import backward_reference as bref
import camera_backward_reference as cref
import composed_reference as comp
import project_backward_reference as pref
import project_backward_scenes as psc
import trainer_sweep_cases as tsc

DEFAULT = [tsc.case(s) for s in range(tsc.DEFAULT_SEEDS)]
ALL = DEFAULT + list(tsc.WIDE)
FACTOR = 10.0
_cache = {}


def frame(pkg, oracle, c):
    """(vertices, uniforms, oracle stages) of a case's frame in its mode, on coefficients rounded to binary16 where the case
    stores them so: computed once."""
    key = ("frame", c["name"])
    if key not in _cache:
        verts = oracle.activate_records(tsc.records(pkg.synth, c))
        if c["sh16"]:
            verts["sh"] = verts["sh"].astype(np.float16).astype(np.float32)
        u = oracle.camera_uniforms(tsc.camera(oracle, c), c["width"], c["height"])
        _cache[key] = (verts, u, comp.frame(oracle, verts, u, c["antialiased"]))
    return _cache[key]


def blend(pkg, oracle, c):
    key = ("blend", c["name"])
    if key not in _cache:
        _, _, ref = frame(pkg, oracle, c)
        _cache[key] = bref.backward(oracle, ref, c["width"], c["height"], *tsc.grads(c))
    return _cache[key]


def sums(pkg, oracle, c):
    """The four input gradients of the projection: the blend's sums (WIDE: seeded random ones -- what the projection is asked
    here does not depend on them, and the blend's reference of a WIDE frame takes ten seconds)."""
    if c in tsc.WIDE:
        return psc.random_gradients(c["n"], seed=c["seed"])
    want = blend(pkg, oracle, c)
    return {name: want[name] for name in comp.INS}


def project(pkg, oracle, c, mutate=None):
    key = ("project", c["name"], mutate)
    if key not in _cache:
        verts, u, ref = frame(pkg, oracle, c)
        g = sums(pkg, oracle, c)
        _cache[key] = pref.backward(*pref.unpack_vertices(verts, sh16=c["sh16"]), u, ref["tiles"] != 0, ref["attr"]["color_radii"][:, 0] > 0,
                                    colour=g["colour"], opacity_grad=g["opacity"], conic=g["conic"], uv=g["uv"],
                                    antialiased=c["antialiased"], sh_rest_coeffs=c["k"], mutate=mutate)
    return _cache[key]


def camera(pkg, oracle, c, mutate=None):
    verts, u, ref = frame(pkg, oracle, c)
    g = sums(pkg, oracle, c)
    return cref.backward(*pref.unpack_vertices(verts, sh16=c["sh16"]), u, ref["tiles"] != 0, ref["attr"]["color_radii"][:, 0] > 0,
                         colour=g["colour"], opacity_grad=g["opacity"], conic=g["conic"], uv=g["uv"], antialiased=c["antialiased"],
                         mutate=mutate)


def by_cost(pkg, oracle, cases=DEFAULT):
    """The cases with a visible Gaussian, cheapest frame first."""
    seen = [c for c in cases if (frame(pkg, oracle, c)[2]["tiles"] != 0).any()]
    return sorted(seen, key=lambda c: len(frame(pkg, oracle, c)[2]["keys"]))


# ------------------------------------------------------------------------------------------------ the draw
def test_a_case_is_a_function_of_its_seed_alone_and_lies_in_the_stated_ranges():
    assert list(tsc.SEEDS)[:tsc.DEFAULT_SEEDS] == list(range(24)) and len(tsc.WIDE) == 3
    for c in DEFAULT:
        assert c == tsc.case(c["seed"])
        assert c["n"] in tsc.SIZES and 1 <= c["width"] <= 160 and 1 <= c["height"] <= 120 and c["kind"] in ("A", "T")
        assert -4.5 <= c["log_scale_mean"] <= -1.5 and -3 <= c["opacity_shift"] <= 4 and 25 <= c["fov"] <= 100
        assert max(abs(v) for v in c["position"]) <= 0.5 and abs(np.linalg.norm(c["rotation"]) - 1) < 1e-12
        assert 2 * np.degrees(np.arccos(min(1.0, abs(c["rotation"][0])))) < 35        # within about 30 degrees of the default view
        assert c["k"] in tsc.COEFFS and c["exp_mode"] in (2, 3) and c["in_flight"] in (1, 3) and c["channels"] in tsc.CHANNELS
        assert c["mask"] in tsc.MASKS and c["preload"] in tsc.PRELOADS
    for c in tsc.WIDE:
        assert (c["n"], c["width"], c["height"]) == tsc.WIDE_SIZE == (3000, 256, 144)
    assert len({(c["position"], c["rotation"], c["fov"]) for c in tsc.WIDE}) == 3
    assert len({tuple(c[s] for s in tsc.SWITCHES) + (c["exp_mode"], c["in_flight"], c["k"]) for c in tsc.WIDE}) == 3


def test_records_hold_no_sh_coefficient_beyond_k(pkg):
    for c in DEFAULT[:8]:
        planar = tsc.records(pkg.synth, c)[:, 9:54].reshape(c["n"], 3, 15)
        assert not planar[:, :, c["k"]:].any() and (c["k"] == 0 or planar[:, :, :c["k"]].any())


# ------------------------------------------------------------------------------------------------ coverage
def test_the_default_seeds_and_wide_cover_what_the_sweep_is_for(pkg, oracle):
    met = dict.fromkeys(("width < 16", "height < 16", "one Gaussian", "fewer than 4 visible", "every Gaussian visible", "no Gaussian visible",
                         "a list beyond 8 chunks", "more than 1024 blend terms", "listed in more than 20 tiles", "x clamp binds",
                         "y clamp binds", "red at zero"), False)
    for c in ALL:
        _, _, ref = frame(pkg, oracle, c)
        vis = ref["tiles"] != 0
        lists = ref["boundaries"].astype(np.int64).reshape(-1, 2)
        assert len(lists) == tsc.tiles_of(c)
        want = project(pkg, oracle, c)
        met["width < 16"] |= c["width"] < 16
        met["height < 16"] |= c["height"] < 16
        met["one Gaussian"] |= c["n"] == 1
        met["fewer than 4 visible"] |= vis.sum() < 4
        met["every Gaussian visible"] |= bool(vis.all())
        met["no Gaussian visible"] |= not vis.any()
        met["a list beyond 8 chunks"] |= int((lists[:, 1] - lists[:, 0]).max()) > 8 * 64
        met["listed in more than 20 tiles"] |= int(ref["tiles"].max()) > 20
        met["x clamp binds"] |= bool(want["binds"][:, 0].any())
        met["y clamp binds"] |= bool(want["binds"][:, 1].any())
        met["red at zero"] |= bool((vis & (ref["attr"]["color_radii"][:, 0] == 0)).any())
        if c not in tsc.WIDE:
            met["more than 1024 blend terms"] |= int(blend(pkg, oracle, c)["terms"]["colour"].max()) > 1024
    assert all(met.values()), [k for k, v in met.items() if not v]
    for c in tsc.WIDE:
        assert tsc.tiles_of(c) >= 100 and 4 * (frame(pkg, oracle, c)[2]["tiles"] != 0).sum() >= c["n"] // 2
    assert {c["k"] for c in ALL} == set(tsc.COEFFS)
    for switch in tsc.SWITCHES:
        assert {c[switch] for c in DEFAULT} == {False, True}, switch
    assert {c["exp_mode"] for c in DEFAULT} == {2, 3} and {c["in_flight"] for c in DEFAULT} == {1, 3}
    assert {c["graph"] for c in DEFAULT if c["in_flight"] == 3} == {False, True}          # a graph of one frame and of three
    assert {c["tile_cull"] for c in DEFAULT if c["one_pass"]} == {False, True}            # the cull acts on the one-pass level 1 only
    assert {c["mask"] for c in DEFAULT} == set(tsc.MASKS) and {c["preload"] for c in DEFAULT} == set(tsc.PRELOADS)
    assert len({c["channels"] for c in DEFAULT}) >= 6 and {c["kind"] for c in DEFAULT} == {"A", "T"}
    fovs = sorted(c["fov"] for c in ALL)
    assert fovs[0] < 30 and fovs[-1] > 85


# ------------------------------------------------------------------------------------------------ exclusions
def test_the_ill_conditioned_predicate_leaves_out_next_to_nothing(pkg, oracle):
    visible = excluded = clean = 0
    for c in ALL:
        want = project(pkg, oracle, c)
        ill = tsc.ill_conditioned(want) if c["antialiased"] else np.zeros(c["n"], bool)
        assert not (ill & ~want["visible"]).any()
        visible += int(want["visible"].sum())
        excluded += int(ill.sum())
        clean += int(c not in tsc.WIDE and not ill.any())
        if c["antialiased"] and want["visible"].any():
            print(f"{c['name']}: smallest visible det_raw {np.nanmin(want['det_raw']):.3g}, {int(ill.sum())} excluded")
    print(f"{excluded} of {visible} visible Gaussians excluded; {clean} of {len(DEFAULT)} default cases with none")
    assert visible > 5000 and excluded <= 0.005 * visible and clean >= 20
    # ... and the predicate is not vacuous: project_backward_scenes' needle, a splat without area, is what it names
    needle = psc.branch_records()
    verts = oracle.activate_records(needle)
    w, h = psc.BRANCH_FRAME
    u = oracle.camera_uniforms(oracle.default_camera(), w, h)
    ref = oracle.stages(verts, u)
    want = pref.backward(*pref.unpack_vertices(verts), u, ref["tiles"] != 0, ref["attr"]["color_radii"][:, 0] > 0, antialiased=True)
    ill = tsc.ill_conditioned(want)
    assert ill[psc.BRANCH_NEEDLE] and ill.sum() == 1


# ------------------------------------------------------------------------------------------------ teeth
def _first_beyond(pkg, oracle, miss, label, cases=None):
    """The first case, cheapest first, in which miss(case) -- the worst |bent - true| / bound of the true reference -- reaches FACTOR."""
    best = 0.0
    for c in (cases or by_cost(pkg, oracle)):
        ratio = miss(c)
        best = max(best, ratio)
        if ratio >= FACTOR:
            print(f"{label}: {c['name']} puts the bent reference {ratio:.3g} bounds from the true one")
            return c
    raise AssertionError(f"{label}: no sweep case moves the bent reference by {FACTOR:g} bounds (the most: {best:.3g})")


def _halve_conic_1(g):
    conic = g["conic"].copy()
    conic[:, 1] *= 0.5
    return dict(g, conic=conic)


def _swap_uv(g):
    return dict(g, uv=np.ascontiguousarray(g["uv"][:, ::-1]))


@pytest.mark.parametrize("bend", [_swap_uv, _halve_conic_1], ids=["d_uv swapped", "d_conic[1] halved"])
def test_a_slip_between_the_blends_sums_and_the_projection_is_beyond_the_bound(pkg, oracle, bend):
    def miss(c):
        verts, u, ref = frame(pkg, oracle, c)
        args = (oracle, verts, u, ref, *tsc.grads(c), c["antialiased"], False, c["sh16"], c["k"])
        want, spread, _ = comp.composed(*args)
        bent, _, _ = comp.composed(*args, bend=bend)
        return max(float((np.abs(bent[name] - want[name]) / np.maximum(pref.bound(want, name) + spread[name], 1e-300)).max())
                   for name in ("means", "log_scales", "quats"))
    _first_beyond(pkg, oracle, miss, bend.__name__)


def _only_tile(ref, t):
    """`ref` with every tile's list but tile t's emptied: the walk of tile t alone."""
    b = ref["boundaries"].copy().reshape(-1, 2)
    keep = b[t].copy()
    b[:, 1] = b[:, 0]
    b[t] = keep
    return dict(ref, boundaries=b.reshape(ref["boundaries"].shape))


def test_dropping_one_tiles_adds_of_a_gaussian_listed_in_several_is_beyond_the_bound(pkg, oracle):
    """Tiles are walked independently, so what tile t adds is the walk of tile t alone; without it a Gaussian's sum is short by
    exactly that."""
    def miss(c):
        _, _, ref = frame(pkg, oracle, c)
        want = blend(pkg, oracle, c)
        lists = ref["boundaries"].astype(np.int64).reshape(-1, 2)
        t = int(np.argmax(lists[:, 1] - lists[:, 0]))
        alone = bref.backward(oracle, _only_tile(ref, t), c["width"], c["height"], *tsc.grads(c))
        assert (alone["terms"]["colour"] <= want["terms"]["colour"]).all()
        several = ref["tiles"] > 1
        if not (several & (alone["terms"]["colour"] > 0)).any():
            return 0.0
        return max(float((np.abs(alone[name]) / np.maximum(bref.bound(want, name), 1e-300))[several].max()) for name in bref.OUTPUTS)
    _first_beyond(pkg, oracle, miss, "one tile's adds dropped")


def test_pixels_past_the_right_or_bottom_edge_of_a_partial_tile_are_beyond_the_bound(pkg, oracle):
    """The frame grown to whole tiles, the gradient maps continued with seeded values there (a kernel that walks those lanes reads
    whatever lies behind the row): the same lists, the same tile grid, more pixels."""
    def miss(c):
        w, h = c["width"], c["height"]
        if w % 16 == 0 and h % 16 == 0:
            return 0.0
        _, _, ref = frame(pkg, oracle, c)
        want = blend(pkg, oracle, c)
        W, H = (w + 15) // 16 * 16, (h + 15) // 16 * 16
        rng = np.random.default_rng(5)
        G, ga = tsc.grads(c)
        Gp, gap = rng.standard_normal((H, W, 3)).astype(np.float32), rng.standard_normal((H, W)).astype(np.float32)
        Gp[:h, :w], gap[:h, :w] = G, (0.0 if ga is None else ga)
        bent = bref.backward(oracle, ref, W, H, Gp, None if ga is None else gap)
        assert np.array_equal(bent["image"][:h, :w], want["image"])
        return max(float((np.abs(bent[name] - want[name]) / np.maximum(bref.bound(want, name), 1e-300)).max()) for name in bref.OUTPUTS)
    _first_beyond(pkg, oracle, miss, "pixels beyond the frame's edge")


@pytest.mark.parametrize("mutation", ["camera_at_origin", "view_transposed"])
def test_a_view_direction_from_p_and_a_transposed_view_matrix_are_beyond_the_projections_bound(pkg, oracle, mutation):
    def miss(c):
        want, bent = project(pkg, oracle, c), project(pkg, oracle, c, mutation)
        return max(float((np.abs(bent[name] - want[name]) / np.maximum(pref.bound(want, name), 1e-300)).max()) for name in ("means",))
    _first_beyond(pkg, oracle, miss, mutation)


@pytest.mark.parametrize("mutation", cref.MUTATIONS)
def test_each_mutation_of_the_camera_reference_is_beyond_its_bound(pkg, oracle, mutation):
    def miss(c):
        want, bent = camera(pkg, oracle, c), camera(pkg, oracle, c, mutation)
        return max(float((np.abs(bent[name] - want[name]) / np.maximum(cref.bound(want, name), 1e-300)).max()) for name in cref.OUTPUTS)
    _first_beyond(pkg, oracle, miss, mutation)
