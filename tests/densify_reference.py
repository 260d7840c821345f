"""gs_accumulate_densify_stats, gs_densify_plan and gs_densify_apply restated: the yardstick of tests/test_densify_api.py (CPU)
and tests/test_gpu_densify.py.  Two independent formulations.

(a) THE CONTRACT'S BITS in numpy (stats, plan, apply), as include/gs3d_hip.h writes them.  numpy's float64 +, -, *, / and sqrt are
IEEE operations, one rounding each, never fused: the arrays below ARE the contract's bits.  The binary32 activation -- exp of the
log-scales, the sigmoid of the logits, the quaternion's normalisation -- is not restated: it is the host path's
(gs_activate_records), which the device-array ingest is pinned to bit for bit (tests/test_gpu_device_arrays.py).

    avg = count ? grad_sum / count : 0          s = sg_0; if sg_1 > s: s = sg_1; if sg_2 > s: s = sg_2          o = sigmoid(logit)
    grow = avg >= grad_threshold                clone = grow and s <= dense_extent       split = grow and s > dense_extent
    a row is pruned where o < min_opacity, or (max_screen_radius > 0 and) its own max_radius > max_screen_radius, or
    (max_world_scale > 0 and) its own s > max_world_scale; appended rows have no radius; a split child's s is that of ls - log 1.6

(b) THE TRAINERS' SEQUENCE, literally, in float32 torch on the CPU (trainer_sequence): boolean masks, cat of the clones, cat of
the split children (build_rotation, bmm, log(exp(ls) / 1.6)), removal of the split parents, the prune over the extended set.  Written
from the description in include/gs3d_hip.h, in the trainers' order "survivors, clones, splits"; every row carries (parent, role) so
that a test can bring it into (a)'s parent order."""
import numpy as np

import adam_step_reference as ar

NAMES = ar.NAMES
LOG_1_6 = float.fromhex("0x1.e148a1a2726cep-2")      # GS_DENSIFY_LOG_1_6
PARTITION, BLOCK = 2048, 256                         # GS_DENSIFY_PARTITION, GS_DENSIFY_BLOCK
ORIGINAL, COPY, CHILD0, CHILD1 = 0, 1, 2, 3          # a row's role
RULE_NAMES = ("grad_threshold", "dense_extent", "min_opacity", "max_screen_radius", "max_world_scale")


def rule(grad_threshold=2e-4, dense_extent=0.05, min_opacity=0.005, max_screen_radius=0.0, max_world_scale=0.0):
    return dict(grad_threshold=grad_threshold, dense_extent=dense_extent, min_opacity=min_opacity, max_screen_radius=max_screen_radius,
                max_world_scale=max_world_scale)


def zero_stats(n):
    return dict(grad_sum=np.zeros(n, np.float64), count=np.zeros(n, np.uint32), max_radius=np.zeros(n, np.float32))


# ------------------------------------------------------------------------------------------------ (a) the statistic
def accumulate_stats(stats, uv, tiles, radius, width, height):
    """IN PLACE, for the rows with tiles != 0 only: grad_sum += sqrt(((gx W/2) (gx W/2)) + ((gy H/2) (gy H/2))), count += 1,
    max_radius = the frame's radius where that is greater."""
    seen = np.asarray(tiles) != 0
    uv = np.asarray(uv, np.float64)
    a, b = uv[seen, 0] * (np.float64(width) / 2.0), uv[seen, 1] * (np.float64(height) / 2.0)
    with np.errstate(all="ignore"):
        stats["grad_sum"][seen] = stats["grad_sum"][seen] + np.sqrt((a * a) + (b * b))
        stats["count"][seen] = stats["count"][seen] + np.uint32(1)
        r, was = np.asarray(radius, np.float32)[seen], stats["max_radius"][seen]
        stats["max_radius"][seen] = np.where(r > was, r, was)


# ------------------------------------------------------------------------------------------------ (a) the decision
def activation(pkg, log_scales, logits=None, quats=None):
    """(scales (n, 3), opacity (n,), normalised quaternion (n, 4)): the ingest's binary32, by the host path."""
    n = len(log_scales)
    rec = np.zeros((n, 62), np.float32)
    rec[:, ar.COLUMNS["log_scales"]] = log_scales
    rec[:, ar.COLUMNS["quats"]] = (1, 0, 0, 0) if quats is None else quats
    if logits is not None:
        rec[:, 54] = np.asarray(logits, np.float32).reshape(n)
    with np.errstate(all="ignore"):
        v = pkg.activate_records(rec).reshape(n, 60)
    return v[:, 4:7].copy(), v[:, 7].copy(), v[:, 8:12].copy()


def largest(sg):
    s = sg[:, 0].copy()
    with np.errstate(invalid="ignore"):
        s = np.where(sg[:, 1] > s, sg[:, 1], s)
        s = np.where(sg[:, 2] > s, sg[:, 2], s)
    return s.astype(np.float64)


def quantities(pkg, params, stats):
    """What the rule compares, in binary64: avg, s, o, the radius, and s of a split's children; with the children's log-scales."""
    ls = np.asarray(params["log_scales"], np.float32)
    n = len(ls)
    cnt = np.asarray(stats["count"]).astype(np.uint32)
    with np.errstate(all="ignore"):
        avg = np.where(cnt != 0, np.asarray(stats["grad_sum"], np.float64) / np.where(cnt != 0, cnt, 1).astype(np.float64), 0.0)
        child_ls = (ls.astype(np.float64) - np.float64(LOG_1_6)).astype(np.float32)
    sg, o, _ = activation(pkg, ls, params["opacity_logits"])
    child_sg, _, _ = activation(pkg, child_ls)
    return dict(avg=avg, s=largest(sg), o=o.astype(np.float64), radius=np.asarray(stats["max_radius"], np.float32).astype(np.float64),
                child_s=largest(child_sg), child_ls=child_ls, sg=sg, n=n)


def plan(pkg, params, stats, r):
    """dict: clone, split (the classes), rows (0, 1, 2 per parent), noisy (a split parent whose children survive), copy_only (a
    clone whose original the radius pruned), row_offset, noise_offset (uint32, n + 1 each), n_out, n_noise, and q = quantities()."""
    q = quantities(pkg, params, stats)
    with np.errstate(invalid="ignore"):
        grow = q["avg"] >= r["grad_threshold"]
        clone, split = grow & (q["s"] <= r["dense_extent"]), grow & (q["s"] > r["dense_extent"])
        faint = q["o"] < r["min_opacity"]
        big = (q["s"] > r["max_world_scale"]) if r["max_world_scale"] > 0 else np.zeros(q["n"], bool)
        child_big = (q["child_s"] > r["max_world_scale"]) if r["max_world_scale"] > 0 else np.zeros(q["n"], bool)
        wide = (q["radius"] > r["max_screen_radius"]) if r["max_screen_radius"] > 0 else np.zeros(q["n"], bool)
    both = faint | big
    original = ~(both | wide)
    copy = clone & ~both
    noisy = split & ~(faint | child_big)
    rows = np.where(split, 2 * noisy, original.astype(int) + copy.astype(int)).astype(np.uint32)
    out = dict(clone=clone, split=split, rows=rows, noisy=noisy, copy_only=copy & ~original & ~split, q=q)
    out["row_offset"] = np.concatenate([[0], np.cumsum(rows, dtype=np.uint64)]).astype(np.uint32)
    out["noise_offset"] = np.concatenate([[0], np.cumsum(noisy, dtype=np.uint64)]).astype(np.uint32)
    out["n_out"], out["n_noise"] = int(rows.sum(dtype=np.uint64)), int(noisy.sum())
    return out


def rows_of(p):
    """(parent, role) of every output row, in output order."""
    n = len(p["rows"])
    parent = np.repeat(np.arange(n), p["rows"])
    k = np.arange(len(parent)) - p["row_offset"][parent].astype(np.int64)
    role = np.where(p["split"][parent], CHILD0 + k, np.where(p["rows"][parent] == 2, k, np.where(p["copy_only"][parent], COPY, ORIGINAL)))
    return parent, role.astype(np.int64)


# ------------------------------------------------------------------------------------------------ (a) the compaction
def rotation(qn):
    """The nine entries, binary64, of the normalised binary32 quaternions qn (n, 4) = w x y z, in the header's order."""
    w, x, y, z = (qn[:, e].astype(np.float64) for e in range(4))
    R = np.empty((len(qn), 3, 3), np.float64)
    R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = 1.0 - 2.0 * ((y * y) + (z * z)), 2.0 * ((x * y) - (w * z)), 2.0 * ((x * z) + (w * y))
    R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = 2.0 * ((x * y) + (w * z)), 1.0 - 2.0 * ((x * x) + (z * z)), 2.0 * ((y * z) - (w * x))
    R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = 2.0 * ((x * z) - (w * y)), 2.0 * ((y * z) + (w * x)), 1.0 - 2.0 * ((x * x) + (y * y))
    return R


def apply(pkg, params, moments, p, noise):
    """(new_params, new_moments, (parent, role)) from plan p: moments = dict(exp_avg={name: array}, exp_avg_sq={...}) or None (a name
    absent has none); noise (>= n_noise, 2, 3) float32."""
    parent, role = rows_of(p)
    new = {name: np.array(np.asarray(v, np.float32)[parent], np.float32, order="C") for name, v in params.items()}
    kids = role >= CHILD0
    if kids.any():
        pk, c = parent[kids], role[kids] - CHILD0
        j = p["noise_offset"][pk].astype(np.int64)
        with np.errstate(all="ignore"):
            _, _, qn = activation(pkg, np.asarray(params["log_scales"], np.float32)[pk], quats=np.asarray(params["quats"], np.float32)[pk])
            R = rotation(qn)
            d = p["q"]["sg"][pk].astype(np.float64) * np.asarray(noise, np.float32)[j, c].astype(np.float64)
            m = np.asarray(params["means"], np.float32)[pk].astype(np.float64)
            moved = m + (((R[:, :, 0] * d[:, None, 0]) + (R[:, :, 1] * d[:, None, 1])) + (R[:, :, 2] * d[:, None, 2]))
            new["means"][kids] = moved.astype(np.float32)
        new["log_scales"][kids] = p["q"]["child_ls"][pk]
    new_moments = None
    if moments is not None:
        new_moments = {what: {name: np.array(np.asarray(v, np.float32)[parent], np.float32, order="C") for name, v in moments[what].items()}
                       for what in ("exp_avg", "exp_avg_sq")}
        for what in new_moments:
            for v in new_moments[what].values():
                v[role != ORIGINAL] = 0.0
    return new, new_moments, (parent, role)


def densify(pkg, params, moments, stats, r, noise):
    p = plan(pkg, params, stats, r)
    return (*apply(pkg, params, moments, p, noise), p)


# ------------------------------------------------------------------------------------------------ (b) the trainers' sequence
def build_rotation(torch, r):
    norm = torch.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2] + r[:, 3] * r[:, 3])
    q = r / norm[:, None]
    R = torch.zeros((q.size(0), 3, 3), dtype=r.dtype)
    r_, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R[:, 0, 0] = 1 - 2 * (y * y + z * z)
    R[:, 0, 1] = 2 * (x * y - r_ * z)
    R[:, 0, 2] = 2 * (x * z + r_ * y)
    R[:, 1, 0] = 2 * (x * y + r_ * z)
    R[:, 1, 1] = 1 - 2 * (x * x + z * z)
    R[:, 1, 2] = 2 * (y * z - r_ * x)
    R[:, 2, 0] = 2 * (x * z - r_ * y)
    R[:, 2, 1] = 2 * (y * z + r_ * x)
    R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def trainer_sequence(params, moments, stats, r, noise_by_parent):
    """float32 torch, CPU.  params, moments: numpy, as apply() takes them; noise_by_parent (n, 2, 3): the draws of parent i's two
    children should it split.  Returns (new_params, new_moments, parent, role) as numpy, in the TRAINERS' order."""
    import torch
    t = {k: torch.tensor(np.asarray(v, np.float32)) for k, v in params.items()}
    mom = {what: {k: torch.tensor(np.asarray(v, np.float32)) for k, v in moments[what].items()} for what in ("exp_avg", "exp_avg_sq")}
    n = len(t["means"])
    parent, role = torch.arange(n), torch.zeros(n, dtype=torch.int64)
    cnt = torch.tensor(np.asarray(stats["count"]).astype(np.int64))
    # (a trainer's accumulator of a Gaussian no frame saw is 0, and 0 / 0 = NaN -> 0; the scenes here put arbitrary bits there,
    # which the contract does not read)
    accum = torch.tensor(np.where(np.asarray(stats["count"]) != 0, np.asarray(stats["grad_sum"], np.float64), 0.0))
    avg = (accum / cnt).float()
    avg[avg.isnan()] = 0.0
    radii = torch.tensor(np.asarray(stats["max_radius"], np.float32))
    z = torch.tensor(np.asarray(noise_by_parent, np.float32))

    def extend(rows, roles, changed):
        nonlocal parent, role, radii
        for k in t:
            t[k] = torch.cat([t[k], changed.get(k, t[k][rows])])
            for what in mom:
                if k in mom[what]:
                    mom[what][k] = torch.cat([mom[what][k], torch.zeros_like(mom[what][k][rows])])
        parent, role = torch.cat([parent, parent[rows]]), torch.cat([role, roles])
        radii = torch.cat([radii, torch.zeros(len(roles))])

    def keep(mask):
        nonlocal parent, role, radii
        for k in t:
            t[k] = t[k][mask]
            for what in mom:
                if k in mom[what]:
                    mom[what][k] = mom[what][k][mask]
        parent, role, radii = parent[mask], role[mask], radii[mask]

    # 1. clone
    scale_max = torch.exp(t["log_scales"]).max(dim=1).values
    grow = avg >= r["grad_threshold"]
    clone = torch.nonzero(grow & (scale_max <= r["dense_extent"])).reshape(-1)
    extend(clone, torch.full((len(clone),), COPY), {})
    # 2. split (the appended rows have no gradient)
    grow = torch.cat([grow, torch.zeros(len(clone), dtype=torch.bool)])
    scale_max = torch.exp(t["log_scales"]).max(dim=1).values
    split = grow & (scale_max > r["dense_extent"])
    rows = torch.nonzero(split).reshape(-1)
    stds = torch.exp(t["log_scales"][rows]).repeat(2, 1)
    samples = stds * torch.cat([z[parent[rows], 0], z[parent[rows], 1]])
    rots = build_rotation(torch, t["quats"][rows]).repeat(2, 1, 1)
    means = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + t["means"][rows].repeat(2, 1)
    log_scales = torch.log(torch.exp(t["log_scales"][rows].repeat(2, 1)) / 1.6)
    twice = torch.cat([rows, rows])
    extend(twice, torch.cat([torch.full((len(rows),), CHILD0), torch.full((len(rows),), CHILD1)]), dict(means=means, log_scales=log_scales))
    keep(~torch.cat([split, torch.zeros(2 * len(rows), dtype=torch.bool)]))
    # 3. prune over the extended set
    prune = torch.sigmoid(t["opacity_logits"].reshape(-1)) < r["min_opacity"]
    if r["max_screen_radius"] > 0:
        prune = prune | (radii > r["max_screen_radius"])
    if r["max_world_scale"] > 0:
        prune = prune | (torch.exp(t["log_scales"]).max(dim=1).values > r["max_world_scale"])
    keep(~prune)
    return ({k: v.numpy() for k, v in t.items()}, {what: {k: v.numpy() for k, v in mom[what].items()} for what in mom}, parent.numpy(), role.numpy())


# ------------------------------------------------------------------------------------------------ scenes
def scene(pkg, n, seed=1, k=15, classes=None, pruned=None, with_moments=NAMES, r=None):
    """A model of n rows, its moments, statistics, rule and noise, with the classes set BY CONSTRUCTION: classes (n,) of 0 keep,
    1 clone, 2 split (None: a random mix); pruned (n,) of 0 no, 1 by opacity, 2 by screen radius, 3 by world scale (None: a random
    tenth each; 2 and 3 only where the rule has them on).  Every decision quantity lies at least a relative 1e-2 from its threshold
    (margins() measures it)."""
    rng = np.random.default_rng(seed)
    r = rule(max_screen_radius=20.0, max_world_scale=0.5) if r is None else r
    params = ar.cut(pkg.synth.synth_records(max(n, 1), seed=seed, kind="A")[:n], k)
    if k == 0:
        del params["sh_rest"]
    classes = rng.integers(0, 3, n) if classes is None else np.asarray(classes)
    pruned = np.where(rng.random(n) < 0.3, rng.integers(1, 4, n), 0) if pruned is None else np.asarray(pruned)
    if not r["max_screen_radius"] > 0:
        pruned = np.where(pruned == 2, 0, pruned)
    if not r["max_world_scale"] > 0:
        pruned = np.where(pruned == 3, 0, pruned)
    ext, top = r["dense_extent"], (r["max_world_scale"] if r["max_world_scale"] > 0 else 64 * r["dense_extent"])
    # the largest scale: small in [ext / 8, ext / 1.05], large in [1.05 ext, top / 1.05] (a child, / 1.6, is then clear of `top`), pruned
    # by the world scale in [1.7, 3] top (a child is then beyond 1.06 top).  A row that large and growing is a split by the rule.
    if r["max_world_scale"] > 0:
        classes = np.where((pruned == 3) & (classes == 1), 2, classes)
    small = np.exp(rng.uniform(np.log(ext / 8), np.log(ext / 1.05), n))
    large = np.exp(rng.uniform(np.log(1.05 * ext), np.log(top / 1.05), n))
    s = np.where((classes == 2) | ((classes == 0) & (rng.random(n) < 0.5)), large, small)
    s = np.where(pruned == 3, rng.uniform(1.7, 3.0, n) * top, s)
    ratios = rng.uniform(0.2, 1.0, (n, 3))
    ratios[np.arange(n), rng.integers(0, 3, n)] = 1.0
    params["log_scales"] = np.log(s[:, None] * ratios).astype(np.float32)
    o = np.where(pruned == 1, rng.uniform(0.1, 0.9, n) * r["min_opacity"], rng.uniform(1.1 * r["min_opacity"], 0.99, n))
    params["opacity_logits"] = np.log(o / (1 - o)).astype(np.float32)
    stats = zero_stats(n)
    stats["count"][:] = rng.integers(0, 4, n)
    stats["count"][classes != 0] = np.maximum(stats["count"][classes != 0], 1)
    avg = np.where(classes != 0, rng.uniform(1.1, 50.0, n), rng.uniform(0.0, 0.9, n)) * r["grad_threshold"]
    stats["grad_sum"][:] = np.where(stats["count"] != 0, avg * stats["count"], rng.uniform(0, 100, n))   # (unread where count == 0)
    if r["max_screen_radius"] > 0:
        stats["max_radius"][:] = np.where(pruned == 2, rng.uniform(1.05, 4.0, n), rng.uniform(0.0, 0.9, n)) * r["max_screen_radius"]
    else:
        stats["max_radius"][:] = rng.uniform(0, 100, n)
    moments = dict(exp_avg={}, exp_avg_sq={})
    for name in with_moments:
        if name in params:
            moments["exp_avg"][name] = rng.standard_normal(params[name].shape).astype(np.float32)
            moments["exp_avg_sq"][name] = (rng.standard_normal(params[name].shape) ** 2 + 1e-3).astype(np.float32)
    noise = rng.standard_normal((n, 2, 3)).astype(np.float32)
    return dict(params=params, moments=moments, stats=stats, rule=r, noise=noise, classes=classes, pruned=pruned)


def margins(q, r):
    """The smallest relative distance of every decision quantity from its threshold: avg, s (from the extent; with its children
    from the world scale), o, the radius."""
    def rel(v, thr):
        v = np.asarray(v, np.float64)
        return float(np.abs(v / thr - 1.0).min()) if len(v) and thr > 0 else np.inf
    out = dict(avg=rel(q["avg"], r["grad_threshold"]), extent=rel(q["s"], r["dense_extent"]), opacity=rel(q["o"], r["min_opacity"]))
    if r["max_screen_radius"] > 0:
        out["radius"] = rel(q["radius"], r["max_screen_radius"])
    if r["max_world_scale"] > 0:
        out["world"] = min(rel(q["s"], r["max_world_scale"]), rel(q["child_s"], r["max_world_scale"]))
    return out


def tie_scene(pkg):
    """Rows that sit EXACTLY on each threshold, and a binary32 / binary64 step off it: pins >= (avg), <= and > (extent), < (opacity),
    > (radius, world scale).  Returns (scene dict as scene() does, the expected rows per parent, a label per parent)."""
    f32 = np.float32
    ls_small, ls_big, ls_huge = f32(-4.0), f32(-1.0), f32(1.0)
    up = lambda v: np.nextafter(f32(v), f32(np.inf))   # noqa: E731
    sg, _, _ = activation(pkg, np.array([[ls_small] * 3, [up(ls_small)] * 3, [ls_huge] * 3, [up(ls_huge)] * 3], f32))
    ext, above_ext, world, above_world = (float(v) for v in sg[:, 0])
    assert ext < above_ext < world < above_world
    logit = f32(-3.0)
    _, o, _ = activation(pkg, np.zeros((2, 3), f32), np.array([logit, np.nextafter(logit, f32(-np.inf))], f32))
    min_o = float(o[0])
    assert float(o[1]) < min_o
    thr, radius = 2e-4, f32(20.0)
    r = rule(grad_threshold=thr, dense_extent=ext, min_opacity=min_o, max_screen_radius=float(radius), max_world_scale=world)
    hi, lo = f32(2.0), f32(-4.5)                      # an opacity well above the threshold; a scale below the extent
    #        label                                   log-scale       logit  grad_sum            count  radius        rows
    rows = [("avg == threshold grows (>=), s == extent clones (<=)", ls_small, hi, 2 * thr, 2, 0.0, 2),
            ("avg one step below the threshold keeps", ls_small, hi, np.nextafter(thr, 0.0), 1, 0.0, 1),
            ("s one step above the extent splits (>)", up(ls_small), hi, thr, 1, 0.0, 2),
            ("o == min_opacity is not pruned (<)", lo, logit, 0.0, 1, 0.0, 1),
            ("o one step below min_opacity is pruned", lo, np.nextafter(logit, f32(-np.inf)), 0.0, 1, 0.0, 0),
            ("a clone on min_opacity keeps both", lo, logit, thr, 1, 0.0, 2),
            ("radius == max_screen_radius is not pruned (>)", lo, hi, 0.0, 1, radius, 1),
            ("radius one step above is pruned", lo, hi, 0.0, 1, up(radius), 0),
            ("a clone whose original the radius prunes leaves its copy", lo, hi, thr, 1, up(radius), 1),
            ("s == max_world_scale is not pruned (>)", ls_huge, hi, 0.0, 1, 0.0, 1),
            ("s one step above max_world_scale is pruned", up(ls_huge), hi, 0.0, 1, 0.0, 0),
            ("a split is judged by its children's scale: the parent's is beyond, theirs is not", up(ls_huge), hi, thr, 1, 0.0, 2),
            ("a split parent's radius prunes nothing", ls_big, hi, 2 * thr, 2, up(radius), 2),
            ("count == 0: grad_sum is not read", lo, hi, np.inf, 0, 0.0, 1),
            ("a NaN average keeps", lo, hi, np.nan, 1, 0.0, 1)]
    n = len(rows)
    sc = scene(pkg, n, seed=5, k=3, classes=np.zeros(n, int), pruned=np.zeros(n, int), r=r)
    for i, (_, ls, lg, gsum, cnt, rad, _) in enumerate(rows):
        sc["params"]["log_scales"][i] = (ls, ls - f32(1), ls - f32(2))
        sc["params"]["opacity_logits"][i] = lg
        sc["stats"]["grad_sum"][i], sc["stats"]["count"][i], sc["stats"]["max_radius"][i] = gsum, cnt, rad
    return sc, np.array([row[-1] for row in rows], np.uint32), [row[0] for row in rows]
