"""gs_accumulate_densify_stats, gs_densify_plan and gs_densify_apply as far as a machine without a GPU can check them: the
yardstick's two formulations against each other (tests/densify_reference.py: the contract's bits in numpy, the trainers' sequence in
float32 torch), the threshold ties, the statistic against torch.autograd, the ABI's shape, and every refusal of the Python layer and
of the C ABI (they come before a device is touched)."""
import ctypes as C
import decimal
import os
import re

import numpy as np
import pytest

import densify_reference as dr
from helpers import FakeTensor as _Fake, forbid_c, hand_made_renderer, hand_made_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GS_ERR_INVALID = -1
U24 = 2.0 ** -24
MARGIN = 1e-3          # every decision quantity of a scene that two formulations are compared on stays this far from its threshold
SCENES = [dict(n=700, seed=3, k=15), dict(n=300, seed=4, k=3, r=dr.rule()), dict(n=300, seed=6, k=0, r=dr.rule(max_world_scale=0.7))]


# ------------------------------------------------------------------------------------------------ the ABI's shape
def test_the_symbols_are_declared_listed_and_exported_and_the_structures_have_the_headers_layout(pkg):
    with open(os.path.join(ROOT, "include", "gs3d_hip.h")) as f:
        text = f.read()
    header = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    L = pkg.binding.lib()
    for name in ("gs_accumulate_densify_stats", "gs_densify_plan", "gs_densify_apply"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in pkg.binding.SYMBOLS and hasattr(L, name)
    assert "gs_densify.hip" in pkg.binding.KERNEL_SOURCES
    with open(os.path.join(ROOT, "3dgs.cpp_amd", "csrc", "Makefile")) as f:
        assert re.search(r"^KERNELS\s*:=.*\bgs_densify\.hip\b", f.read(), flags=re.M)
    b = pkg.binding
    layouts = {"gs_densify_stats": (b.DensifyStats, ["d_uv", "grad_sum", "count", "max_radius"], [0, 8, 16, 24], 32),
               "gs_densify_rule": (b.DensifyRule, list(dr.RULE_NAMES), [0, 8, 16, 24, 32], 40),
               "gs_densify_input": (b.DensifyInput, ["params", "grad_sum", "count", "max_radius", "rule", "scratch"], [0, 56, 64, 72, 80, 120], 128),
               "gs_densify_output": (b.DensifyOutput, ["exp_avg", "exp_avg_sq", "noise", "n_noise", "n_out", "params", "out_exp_avg", "out_exp_avg_sq"],
                                     [0, 48, 96, 104, 112, 120, 176, 224], 272)}
    for name, (S, members, offsets, size) in layouts.items():
        assert [f[0] for f in S._fields_] == members, name
        assert [getattr(S, m).offset for m in members] == offsets and C.sizeof(S) == size, name
        end = header.index("} %s;" % name)
        body = header[header.rindex("typedef struct", 0, end):end]
        order = [re.search(r"\b%s\b" % m, body).start() for m in members]
        assert order == sorted(order), f"{name}: the header declares the members in another order"
    for macro, value in (("GS_DENSIFY_PARTITION", b.DENSIFY_PARTITION), ("GS_DENSIFY_BLOCK", b.DENSIFY_BLOCK)):
        assert int(re.search(r"#define\s+%s\s+(\d+)u" % macro, header).group(1)) == value == getattr(dr, macro[11:])
    literal = re.search(r"#define\s+GS_DENSIFY_LOG_1_6\s+(\S+)", header).group(1)
    assert float.fromhex(literal) == b.DENSIFY_LOG_1_6 == dr.LOG_1_6
    # ... and it is the binary64 nearest log(1.6): its neighbours are farther from a 60-digit value
    decimal.getcontext().prec = 60
    exact = decimal.Decimal("1.6").ln()
    near = [abs(decimal.Decimal(float(v)) - exact) for v in (np.nextafter(dr.LOG_1_6, 0), dr.LOG_1_6, np.nextafter(dr.LOG_1_6, 1))]
    assert near[1] < near[0] and near[1] < near[2]


# ------------------------------------------------------------------------------------------------ (a) against (b)
@pytest.mark.parametrize("spec", SCENES, ids=lambda s: f"n{s['n']}-k{s['k']}")
def test_the_contracts_rows_are_the_trainers_sequences_rows_and_the_split_children_agree_within_the_counted_roundings(pkg, spec):
    """(a), binary64 on binary32 inputs, against (b), float32 torch.  After (b)'s order "survivors, clones, splits" is brought into
    parent order (original before copy, child 0 before child 1) the two hold the same rows, every copied value and every moment bit
    for bit.  A split child's mean and log-scales differ by (b)'s float32 roundings, counted here with u = 2^-24 (one binary32
    rounding, relative) and first order:
      sigma_j   (b)'s exp is within 1 ulp = 2 u of the true value (torch's vectorised expf), (a)'s -- libm's -- within 0.51 ulp:  4 u
      sigma_j t_j   (b) rounds the product (a) holds exactly:                                                                  5 u
      q         both normalise in binary32.  (b): four squares (u), three adds of positives (<= 3 u in all), sqrt (half of that, + u), the
                division (u): 4 u on the norm's side.  (a): (e0^2 + e1^2) + (e2^2 + e3^2) 3 u, sqrtf 2.5 u, 1 / 3.5 u, the product 4.5 u.
                A component of one against the other's:                                                                  9 u
      R_ij      an entry is 2 (ab +- cd) or 1 - 2 (aa + bb).  Its terms are products of two components (18 u), rounded (u), added
                (u), taken from 1 (u) -- each RELATIVE TO THE TERMS' MAGNITUDES, which is what |R_ij| stands for below: 2 (|ab| + |cd|)
                off the diagonal, 1 + 2 (aa + bb) on it.  (An entry that cancels to nothing still carries its terms' roundings.)   21 u
      R_ij (sigma_j t_j)   21 + 5, the product's rounding:                                                                     27 u
      the sum over j   two adds (any order, fused or not), each at most u times the sum of the magnitudes:                       29 u
      m + ...   (b)'s add rounds to binary32, (a)'s result is rounded to binary32: 2 u on |m| + the sum:                        31 u
    |m'_(a) - m'_(b)| <= 31 * 2^-24 * (|m| + sum_j |R_ij| |sigma_j t_j|), c = 31; (a)'s own binary64 roundings are 2^-29 of one u and the
    neglected second-order terms less: the bound is widened by (1 + 2^-20).
    Log-scales: (b) takes log(exp(ls) / 1.6): exp (2 u relative), the division by the binary32 nearest 1.6 (u for the constant, u for
    the quotient -- or for a reciprocal and a product, one more): a relative 5 u of log's argument is an ABSOLUTE 5 u of its value;
    log itself within 1 ulp (2 u |ls'|); (a)'s one rounding u |ls'|:   |ls'_(a) - ls'_(b)| <= 2^-24 (5 + 3 |ls'|)."""
    pytest.importorskip("torch")
    sc = dr.scene(pkg, **spec)
    params, moments, stats, r = sc["params"], sc["moments"], sc["stats"], sc["rule"]
    p = dr.plan(pkg, params, stats, r)
    margins = dr.margins(p["q"], r)
    print("margins", {k: f"{v:.3g}" for k, v in margins.items()})
    assert min(margins.values()) >= MARGIN, f"a decision quantity sits within {MARGIN} of its threshold: a tie could hide a disagreement"
    assert (p["clone"] == (sc["classes"] == 1)).all() and (p["split"] == (sc["classes"] == 2)).all()
    for what, rows in (("clones", p["clone"]), ("splits", p["split"]), ("keeps", ~(p["clone"] | p["split"]))):
        assert {0, 2} <= set(p["rows"][rows].tolist()) or what == "keeps", f"the scene has no pruned and no surviving {what}"
    assert set(p["rows"][~p["split"]].tolist()) == {0, 1, 2} and (p["copy_only"].any() or not r["max_screen_radius"] > 0)
    noise = sc["noise"][p["noisy"]]                        # (a) numbers the draws by SURVIVING split parents, in parent order
    new, new_m, (parent, role) = dr.apply(pkg, params, moments, p, noise)
    tp, tm, t_parent, t_role = dr.trainer_sequence(params, moments, stats, r, sc["noise"])
    assert not (np.diff(t_role) < 0).any() or (t_role[:np.argmax(t_role > 0)] == 0).all()   # (b) is in ITS order: originals first
    order = np.lexsort((t_role, t_parent))
    assert np.array_equal(t_parent[order], parent) and np.array_equal(t_role[order], role)
    kids = role >= dr.CHILD0
    for name in params:
        got, want = tp[name][order], new[name]
        exact = np.ones(len(role), bool) if name not in ("means", "log_scales") else ~kids
        assert np.array_equal(got[exact].view(np.uint32), want[exact].view(np.uint32)), name
        for what in ("exp_avg", "exp_avg_sq"):
            if name in moments[what]:
                assert np.array_equal(tm[what][name][order].view(np.uint32), new_m[what][name].view(np.uint32)), (what, name)
                assert (new_m[what][name][role != dr.ORIGINAL].view(np.uint32) == 0).all()
    assert kids.sum() == 2 * p["n_noise"] > 0
    pk, c = parent[kids], role[kids] - dr.CHILD0
    _, _, qn = dr.activation(pkg, params["log_scales"][pk], quats=params["quats"][pk])
    w, x, y, z = (np.abs(qn[:, e].astype(np.float64)) for e in range(4))
    mag = np.empty((len(pk), 3, 3))
    mag[:, 0, 0], mag[:, 0, 1], mag[:, 0, 2] = 1 + 2 * (y * y + z * z), 2 * (x * y + w * z), 2 * (x * z + w * y)
    mag[:, 1, 0], mag[:, 1, 1], mag[:, 1, 2] = 2 * (x * y + w * z), 1 + 2 * (x * x + z * z), 2 * (y * z + w * x)
    mag[:, 2, 0], mag[:, 2, 1], mag[:, 2, 2] = 2 * (x * z + w * y), 2 * (y * z + w * x), 1 + 2 * (x * x + y * y)
    d = np.abs(p["q"]["sg"][pk].astype(np.float64) * noise[p["noise_offset"][pk].astype(int), c].astype(np.float64))
    bound = 31 * U24 * (np.abs(params["means"][pk].astype(np.float64)) + (mag * d[:, None, :]).sum(axis=2)) * (1 + 2.0 ** -20)
    err = np.abs(tp["means"][order][kids].astype(np.float64) - new["means"][kids])
    ls_err = np.abs(tp["log_scales"][order][kids].astype(np.float64) - new["log_scales"][kids])
    ls_bound = U24 * (5 + 3 * np.abs(new["log_scales"][kids].astype(np.float64)))
    print(f"worst |(a) - (b)| / bound: means {float((err / bound).max()):.3g}, log-scales {float((ls_err / ls_bound).max()):.3g}")
    assert (err <= bound).all() and (ls_err <= ls_bound).all()
    assert err.max() > 0, "the two formulations agree to the bit on every child: the comparison has no float32 in it?"


def test_rows_exactly_on_a_threshold_fall_on_the_side_the_header_writes(pkg):
    sc, want, labels = dr.tie_scene(pkg)
    p = dr.plan(pkg, sc["params"], sc["stats"], sc["rule"])
    for label, rows, got in zip(labels, want, p["rows"]):
        assert rows == got, label
    q, r = p["q"], sc["rule"]
    assert q["avg"][0] == r["grad_threshold"] and q["s"][0] == r["dense_extent"] and q["o"][3] == r["min_opacity"]
    assert q["radius"][6] == r["max_screen_radius"] and q["s"][9] == r["max_world_scale"]
    assert p["clone"][0] and p["split"][2] and p["copy_only"].nonzero()[0].tolist() == [8] and p["n_noise"] == 3
    _, _, (parent, role) = dr.apply(pkg, sc["params"], sc["moments"], p, sc["noise"])
    assert role[parent == 8].tolist() == [dr.COPY] and role[parent == 0].tolist() == [dr.ORIGINAL, dr.COPY]
    assert role[parent == 2].tolist() == [dr.CHILD0, dr.CHILD1]


def test_the_inputs_keep_their_bits_and_a_nan_reaches_its_own_parents_rows_only(pkg):
    sc = dr.scene(pkg, 200, seed=8, k=3)
    clean = dr.densify(pkg, sc["params"], sc["moments"], sc["stats"], sc["rule"], sc["noise"])
    p = clean[3]
    victim = int(np.nonzero(p["noisy"])[0][3])
    before = {k: v.copy() for k, v in sc["params"].items()}
    sc["params"]["means"][victim, 1] = np.nan
    sc["params"]["sh_dc"][victim + 1, 0] = np.nan
    dirty = dr.densify(pkg, sc["params"], sc["moments"], sc["stats"], sc["rule"], sc["noise"])
    parent = dirty[2][0]
    assert np.array_equal(parent, clean[2][0])
    for name in sc["params"]:
        same = ~np.isin(parent, (victim, victim + 1))
        assert np.array_equal(dirty[0][name][same].view(np.uint32), clean[0][name][same].view(np.uint32)), name
        if name not in ("means", "sh_dc"):
            assert sc["params"][name].tobytes() == before[name].tobytes()
    assert np.isnan(dirty[0]["means"][parent == victim][:, 1]).all() and np.isfinite(dirty[0]["means"][parent == victim][:, [0, 2]]).all()


# ------------------------------------------------------------------------------------------------ the statistic
def test_the_statistic_is_the_norm_of_the_ndc_gradient_torch_autograd_gives(pkg):
    """A hand-made frame: a loss that is a function of the pixel positions uv = ((ndc + 1) (W, H) - 1) / 2 of six Gaussians.  The
    Inria trainer thresholds the norm of d loss / d ndc; the statistic takes d loss / d uv -- what blend_backward sums -- times
    (W / 2, H / 2).  Both in binary64: equal up to the chain rule's one rounding per component and the norm's association."""
    torch = pytest.importorskip("torch")
    w, h, n = 37, 23, 6
    rng = np.random.default_rng(2)
    ndc = torch.tensor(rng.uniform(-1, 1, (n, 2)), dtype=torch.float64, requires_grad=True)
    uv = ((ndc + 1.0) * torch.tensor([w, h], dtype=torch.float64) - 1.0) * 0.5
    uv.retain_grad()
    weights = torch.tensor(rng.standard_normal((n, 2)))
    (torch.sin(uv * 0.3) * weights).sum().backward()
    tiles = np.array([1, 0, 3, 1, 0, 2])
    radius = rng.uniform(1, 9, n).astype(np.float32)
    stats = dr.zero_stats(n)
    stats["max_radius"][:] = 5.0
    for _ in range(2):
        dr.accumulate_stats(stats, uv.grad.numpy(), tiles, radius, w, h)
    seen = tiles != 0
    want = 2 * ndc.grad.norm(dim=1).numpy()
    assert np.allclose(stats["grad_sum"][seen], want[seen], rtol=8 * 2.0 ** -53, atol=0) and (stats["grad_sum"][seen] > 0).all()
    assert (stats["grad_sum"][~seen] == 0).all() and stats["count"].tolist() == [2, 0, 2, 2, 0, 2]
    assert np.array_equal(stats["max_radius"], np.where(seen, np.maximum(radius, np.float32(5)), np.float32(5)))


# ------------------------------------------------------------------------------------------------ the Python layer
SHAPES = dict(means=(100, 3), log_scales=(100, 3), quats=(100, 4), opacity_logits=(100,), sh_dc=(100, 3), sh_rest=(100, 15, 3))


def _stats(**change):
    s = dict(grad_sum=_Fake((100,), "torch.float64"), count=_Fake((100,), "torch.int32"), max_radius=_Fake((100,)))
    s.update(change)
    return s


def test_densify_checks_its_tensors_before_it_reaches_c(pkg, monkeypatch):
    forbid_c(pkg, monkeypatch)
    scene = hand_made_scene(pkg)
    rule = dr.rule()

    def state(**change):
        st = dict(exp_avg={k: _Fake(s) for k, s in SHAPES.items()}, exp_avg_sq={k: _Fake(s) for k, s in SHAPES.items()})
        for what, (name, tensor) in change.items():
            st[what][name] = tensor
        return st

    def params(**change):
        p = {k: _Fake(s) for k, s in SHAPES.items()}
        p.update(change)
        return p

    reached = pytest.raises(AssertionError, match="C library was reached")
    with reached:
        pkg.densify(scene, params(), rule, _stats(), state(), noise=_Fake((100, 2, 3)))
    with reached:                                             # no state, no sh_rest, a uint32 count, a rule as the structure
        pkg.densify(scene, params(sh_rest=None), pkg.binding.DensifyRule(2e-4, 0.05, 0.005, 0.0, 0.0), _stats(count=_Fake((100,), "torch.uint32")))
    with reached:                                             # moments for some groups only
        pkg.densify(scene, params(), rule, _stats(), dict(exp_avg=dict(means=_Fake((100, 3))), exp_avg_sq=dict(means=_Fake((100, 3)))))
    bad = [(dict(p=params(means=_Fake((100, 3), "torch.float64"))), TypeError, "means"), (dict(p=params(quats=_Fake((100, 3)))), ValueError, "quats"),
           (dict(p=params(log_scales=_Fake((99, 3)))), ValueError, "log_scales"), (dict(p=params(sh_rest=_Fake((100, 7, 3)))), ValueError, "sh_rest"),
           (dict(p=params(sh_dc=_Fake((100, 3), contiguous=False))), ValueError, "sh_dc"), (dict(p=params(means=_Fake((100, 3), device="cpu"))), ValueError, "means"),
           (dict(p=params(opacity_logits=None)), TypeError, "opacity_logits"), (dict(p=params(scales=_Fake((100, 3)))), TypeError, "unknown"),
           (dict(p={k: _Fake((50,) + s[1:]) for k, s in SHAPES.items()}), ValueError, "50 rows"),
           (dict(s=_stats(grad_sum=_Fake((100,)))), TypeError, "grad_sum"), (dict(s=_stats(count=_Fake((100,), "torch.int64"))), TypeError, "count"),
           (dict(s=_stats(max_radius=_Fake((101,)))), ValueError, "max_radius"), (dict(s=_stats(max_radius=None)), TypeError, "max_radius"),
           (dict(s=_stats(radius=_Fake((100,)))), TypeError, "unknown"), (dict(s=_stats(count=_Fake((100,), "torch.int32", device="cpu"))), ValueError, "count"),
           (dict(st=state(exp_avg=("means", _Fake((100, 3), "torch.float64")))), TypeError, "means"),
           (dict(st=state(exp_avg_sq=("quats", _Fake((100, 3))))), ValueError, "quats"), (dict(st=state(exp_avg=("sh_dc", None))), ValueError, "partial pair"),
           (dict(st=dict(exp_avg={})), TypeError, "state"), (dict(st=state(exp_avg=("scales", _Fake((100, 3))))), TypeError, "unknown"),
           (dict(p=params(sh_rest=None), st=state()), ValueError, "sh_rest: moments without"),
           (dict(noise=_Fake((100, 6))), ValueError, "noise"), (dict(noise=_Fake((100, 2, 3), "torch.float64")), TypeError, "noise"),
           (dict(r=dict(rule, threshold=1.0)), TypeError, "unknown"), (dict(r={k: v for k, v in rule.items() if k != "min_opacity"}), TypeError, "min_opacity"),
           (dict(r=dict(rule, dense_extent=float("nan"))), ValueError, "dense_extent")]
    for change, error, word in bad:
        with pytest.raises(error, match=word):
            pkg.densify(scene, change.get("p", params()), change.get("r", rule), change.get("s", _stats()), change.get("st", state()), noise=change.get("noise"))


def test_densify_stats_and_the_optimisers_methods_check_before_they_reach_c(pkg, monkeypatch):
    forbid_c(pkg, monkeypatch)
    rend = hand_made_renderer(pkg)
    f64 = "torch.float64"
    with pytest.raises(AssertionError, match="C library was reached"):
        rend.densify_stats(_Fake((100, 2), f64), _stats())
    for uv, error in ((_Fake((100, 2)), TypeError), (_Fake((100, 3), f64), ValueError), (_Fake((100, 2), f64, contiguous=False), ValueError),
                      (_Fake((100, 2), f64, device="cpu"), ValueError)):
        with pytest.raises(error, match="uv"):
            rend.densify_stats(uv, _stats())
    for change, error, word in ((dict(grad_sum=_Fake((100,))), TypeError, "grad_sum"), (dict(count=_Fake((99,), "torch.int32")), ValueError, "count"),
                                (dict(max_radius=None), TypeError, "max_radius"), (dict(extra=_Fake((100,))), TypeError, "unknown")):
        with pytest.raises(error, match=word):
            rend.densify_stats(_Fake((100, 2), f64), _stats(**change))
    assert callable(pkg.densify_stats_zeros) and callable(pkg.Adam.densify)
    opt = object.__new__(pkg.Adam)
    for ceiling in (0.0, 1.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="ceiling"):
            opt.reset_opacity(ceiling)


# ------------------------------------------------------------------------------------------------ the C ABI's refusals
def good_input(pkg, keep, n=4, k=15):
    """A gs_densify_input and a gs_densify_output over host memory (never dereferenced: every call that uses them must fail
    before a device is touched)."""
    b = pkg.binding
    width = dict(means=3, log_scales=3, quats=4, opacity_logits=1, sh_dc=3, sh_rest=3 * max(k, 1))
    inp, out = b.DensifyInput(), b.DensifyOutput()

    def array(count, dtype=np.float32):
        keep.append(np.zeros(max(count, 1), dtype))
        return keep[-1].ctypes.data

    for g, name in enumerate(dr.NAMES):
        setattr(inp.params, name, array(n * width[name]))
        setattr(out.params, name, array(2 * n * width[name]))
        out.exp_avg[g], out.exp_avg_sq[g] = array(n * width[name]), array(n * width[name])
        out.out_exp_avg[g], out.out_exp_avg_sq[g] = array(2 * n * width[name]), array(2 * n * width[name])
    inp.params.sh_rest_coeffs = out.params.sh_rest_coeffs = k
    inp.grad_sum, inp.count, inp.max_radius = array(n, np.float64), array(n, np.uint32), array(n)
    inp.scratch = array(2 * (n + 1), np.uint32)
    inp.rule = b.DensifyRule(2e-4, 0.05, 0.005, 20.0, 0.5)
    out.noise, out.n_noise, out.n_out = array(6 * n), 1, n + 1
    return inp, out


def _set(struct, member, value):
    return lambda i, o: setattr(struct(i, o), member, value(getattr(struct(i, o), member)) if callable(value) else value)


def _item(array, g, value):
    def bend(i, o):
        getattr(o, array)[g] = value(getattr(o, array)[g]) if callable(value) else value
    return bend


INPUT = lambda i, o: i                     # noqa: E731
PARAMS = lambda i, o: i.params             # noqa: E731
RULE = lambda i, o: i.rule                 # noqa: E731
OUTPUT = lambda i, o: o                    # noqa: E731
OUT_PARAMS = lambda i, o: o.params         # noqa: E731
INPUT_REFUSALS = [("means null", "means", _set(PARAMS, "means", None)), ("sh_rest null with k = 15", "sh_rest", _set(PARAMS, "sh_rest", None)),
                  ("quats off by 2", "4-byte", _set(PARAMS, "quats", lambda p: p + 2)), ("sh_rest_coeffs 7", "sh_rest_coeffs", _set(PARAMS, "sh_rest_coeffs", 7)),
                  ("grad_sum null", "statistic", _set(INPUT, "grad_sum", None)), ("count null", "statistic", _set(INPUT, "count", None)),
                  ("max_radius null", "statistic", _set(INPUT, "max_radius", None)), ("scratch null", "scratch", _set(INPUT, "scratch", None)),
                  ("grad_sum off by 4", "8-byte", _set(INPUT, "grad_sum", lambda p: p + 4)), ("count off by 1", "4-byte", _set(INPUT, "count", lambda p: p + 1)),
                  ("max_radius off by 2", "4-byte", _set(INPUT, "max_radius", lambda p: p + 2)), ("scratch off by 3", "4-byte", _set(INPUT, "scratch", lambda p: p + 3))]
INPUT_REFUSALS += [(f"{m} nan", m, _set(RULE, m, float("nan"))) for m in dr.RULE_NAMES]
OUTPUT_REFUSALS = [("n_out > 2 n", "n_out", _set(OUTPUT, "n_out", 9)), ("n_noise > n", "n_noise", _set(OUTPUT, "n_noise", 5)),
                   ("2 n_noise > n_out", "n_noise", _set(OUTPUT, "n_noise", 3)), ("noise null", "noise", _set(OUTPUT, "noise", None)),
                   ("noise off by 1", "4-byte", _set(OUTPUT, "noise", lambda p: p + 1)), ("out means null", "means", _set(OUT_PARAMS, "means", None)),
                   ("out sh_rest null", "sh_rest", _set(OUT_PARAMS, "sh_rest", None)), ("out quats off by 2", "4-byte", _set(OUT_PARAMS, "quats", lambda p: p + 2)),
                   ("out sh_rest_coeffs differs", "sh_rest_coeffs", _set(OUT_PARAMS, "sh_rest_coeffs", 8)),
                   ("a lone exp_avg", "some but not all", _item("exp_avg_sq", 2, None)), ("a lone out_exp_avg_sq", "some but not all", _item("out_exp_avg", 0, None)),
                   ("moments in without out", "some but not all", lambda i, o: (_item("out_exp_avg", 4, None)(i, o), _item("out_exp_avg_sq", 4, None)(i, o))),
                   ("exp_avg off by 2", "4-byte", _item("exp_avg", 1, lambda p: p + 2)), ("out_exp_avg_sq off by 1", "4-byte", _item("out_exp_avg_sq", 5, lambda p: p + 1))]


def test_the_c_calls_refuse_bad_arguments_before_they_touch_a_device(pkg):
    """device = -1 and host pointers: a call that got past its checks would fail otherwise (GS_ERR_DEVICE at the latest); every one
    of these is GS_ERR_INVALID and the message names the argument at fault.  (tests/test_gpu_densify.py repeats them on live tensors
    and checks that nothing moved.)"""
    L = pkg.binding.lib()
    keep = []
    n_out, n_noise = C.c_uint64(7), C.c_uint64(7)
    plan = lambda i, n=4: L.gs_densify_plan(C.byref(i), C.c_uint64(n), -1, None, C.byref(n_out), C.byref(n_noise))   # noqa: E731
    apply = lambda i, o, n=4: L.gs_densify_apply(C.byref(i), C.c_uint64(n), C.byref(o), -1, None)                     # noqa: E731
    for label, word, bend in INPUT_REFUSALS:
        for call in (plan, apply):
            i, o = good_input(pkg, keep)
            bend(i, o)
            assert (call(i) if call is plan else call(i, o)) == GS_ERR_INVALID, label
            assert word in L.gs_last_error().decode(), (label, L.gs_last_error().decode())
    for label, word, bend in OUTPUT_REFUSALS:
        i, o = good_input(pkg, keep)
        bend(i, o)
        assert apply(i, o) == GS_ERR_INVALID, label
        assert word in L.gs_last_error().decode(), (label, L.gs_last_error().decode())
    i, o = good_input(pkg, keep)
    assert plan(i, 2 ** 31) == GS_ERR_INVALID and "2^31" in L.gs_last_error().decode()
    assert apply(i, o, 2 ** 31) == GS_ERR_INVALID and "2^31" in L.gs_last_error().decode()
    assert L.gs_densify_plan(None, C.c_uint64(4), -1, None, C.byref(n_out), C.byref(n_noise)) == GS_ERR_INVALID
    assert L.gs_densify_plan(C.byref(i), C.c_uint64(4), -1, None, None, C.byref(n_noise)) == GS_ERR_INVALID and "null" in L.gs_last_error().decode()
    assert L.gs_densify_apply(C.byref(i), C.c_uint64(4), None, -1, None) == GS_ERR_INVALID and "null" in L.gs_last_error().decode()
    assert L.gs_densify_apply(None, C.c_uint64(4), C.byref(o), -1, None) == GS_ERR_INVALID
    # n == 0 is a success that touches no device: both counts 0, whatever the pointers
    empty = pkg.binding.DensifyInput()
    assert L.gs_densify_plan(C.byref(empty), C.c_uint64(0), -1, None, C.byref(n_out), C.byref(n_noise)) == 0 and n_out.value == n_noise.value == 0
    assert L.gs_densify_apply(C.byref(empty), C.c_uint64(0), C.byref(pkg.binding.DensifyOutput()), -1, None) == 0
    # ... and so is an apply of no output rows (the zero-row case returns before any launch)
    i, o = good_input(pkg, keep)
    o.n_out = o.n_noise = 0
    assert apply(i, o) == 0
    # the statistic
    st = pkg.binding.DensifyStats()
    arrays = [np.zeros(8, np.float64), np.zeros(4, np.float64), np.zeros(4, np.uint32), np.zeros(4, np.float32)]
    fake_renderer = C.c_void_p(keep[0].ctypes.data)          # (never dereferenced: the members are judged first)
    assert L.gs_accumulate_densify_stats(None, C.byref(st)) == GS_ERR_INVALID and "null" in L.gs_last_error().decode()
    assert L.gs_accumulate_densify_stats(fake_renderer, None) == GS_ERR_INVALID and "null" in L.gs_last_error().decode()
    for member in ("d_uv", "grad_sum", "count", "max_radius", None):
        for off, word in ((None, "null member"), (1, "aligned"), (4, "8-byte") if member in ("d_uv", "grad_sum") else (2, "4-byte")):
            st.d_uv, st.grad_sum, st.count, st.max_radius = (a.ctypes.data for a in arrays)
            if member is None:
                continue
            setattr(st, member, None if off is None else getattr(st, member) + off)
            assert L.gs_accumulate_densify_stats(fake_renderer, C.byref(st)) == GS_ERR_INVALID, (member, off)
            assert word in L.gs_last_error().decode(), (member, off, L.gs_last_error().decode())
