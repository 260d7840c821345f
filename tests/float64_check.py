"""One checker of a frame's outputs -- the C oracle's, the reference text's, or the HIP path's stage taps -- against the
independent float64 restatement (np_reference.py), under the shaders' rules or a perturbation of them.

  * discrete outputs (visibility, radius, tile box, tiles, lists, ranges): every mismatch must be EXPLAINED -- the float64
    value that feeds the decision lies within the binary32 evaluation's uncertainty of the threshold or integer boundary;
  * continuous outputs (conic, opacity, uv, depth, rgb): per-Gaussian bounds; the conic's scales with the 2D covariance's
    condition number (its determinant is a cancelling difference);
  * the image: every pixel off by more than ULP noise is within the first-order bound of the inputs' uncertainty, or an
    entry of its list lies within that uncertainty of one of the blend's decisions (power > 0, the alpha cut, the T cut);
    such "explained" pixels are counted and capped per frame;
  * the lists and ranges are restated (np_reference.tile_lists) from the outputs' own boxes and depths, and must be equal.

The uncertainty model: every binary32 quantity carries a few ULP of its inputs' magnitude (EPS x K_*), which is what one
evaluation of the shader's arithmetic in binary32 can differ from the exact value by."""
import numpy as np

import np_reference as npr

EPS = 2.0 ** -24
K_COV = 8.0       # 2D covariance entries: K_COV ulp of |J W|^2 |Sigma| (the magnitude of the products J W Sigma W^T J^T)
K_UV = 16.0       # uv: K_UV ulp of |uv| + W + H, plus the view transform's error through the focal length
K_DEPTH = 4.0     # depth, when binary32 cannot hold the view matrix's row: K_DEPTH ulp of the terms (else: exact rounding count)
K_RGB = 2.0       # rgb: K_RGB ulp of 1 + 3 x the sum of |SH coefficients| (the SH polynomial's terms are smaller)
K_OPACITY = 2.0   # opacity: the logistic in binary32
K_POWER = 4.0     # power: rounding of its three terms, relative to their magnitude
K_EXP = 4.0       # exp() and the product with the opacity, relative
SLACK = 2.0       # every decision margin and continuous bound is SLACK x the modelled uncertainty.  The constants are set so
                  # that the largest error seen on any case is about half its bound (printed per case by the CPU test)
ULP_NOISE = 1e-5  # an image pixel within this of float64 needs no explanation (a blend of binary32 roundings)


def outputs_from_oracle(oracle, st):
    """The common form of a frame's outputs from oracle.stages() (also the reference text's gs_ref.stages())."""
    a = st["attr"]
    return dict(tiles=st["tiles"], depth=a["depth"], radius=a["color_radii"][:, 3], aabb=a["aabb"].astype(np.int64),
                conic=a["conic_opacity"][:, :3], opacity=a["conic_opacity"][:, 3], uv=a["uv"], rgb=a["color_radii"][:, :3],
                sorted_tile=(st["sorted_keys"] >> np.uint64(32)).astype(np.int64), sorted_gid=st["sorted_payload"],
                ranges=st["boundaries"], image=st["image"])


def outputs_from_hip(rend, u, image=None, bgra=None):
    """The same from the HIP path's stage taps of the renderer's last frame."""
    co = rend.stage("conic_opacity").reshape(-1, 4)
    uv_rg = rend.stage("uv_rg").reshape(-1, 4)
    rgb = np.concatenate([uv_rg[:, 2:4], rend.stage("b")[:, None]], axis=1)
    return dict(tiles=rend.stage("tiles"), depth=rend.stage("depth"), radius=rend.stage("radius"),
                aabb=rend.stage("aabb").reshape(-1, 4).astype(np.int64), conic=co[:, :3], opacity=co[:, 3], uv=uv_rg[:, :2],
                rgb=rgb, sorted_tile=rend.stage("sorted_tile").astype(np.int64), sorted_gid=rend.stage("sorted_gid"),
                ranges=rend.stage("ranges", u), image=image, bgra=bgra)


class Mismatch(AssertionError):
    pass


def _check(cond, msg):
    if not cond:
        raise Mismatch(msg)


def reference(frame, rules=None):
    """The float64 frame under `rules`: preprocess (with the near cut) and the attributes of every Gaussian in front of
    the camera (the near cut lowered: what a Gaussian the outputs kept at the cut is compared with), and the uncertainty
    model of each Gaussian's binary32 attributes."""
    R = npr.rules_with(rules)
    # the near cut is a binary32 constant (p_view.z <= 0.2f): float64 decides against that value, not against 0.2
    R = dict(R, near=float(np.float32(R["near"])))
    scene = npr.activate(frame.records, sh16=frame.sh16)
    cam = frame.camera64()
    pre = npr.preprocess(scene, cam, R)
    full = npr.preprocess(scene, cam, dict(R, near=1e-12))
    W, H = frame.width, frame.height
    a, b, c = full["cov2d"].T
    half = np.sqrt((0.5 * (a - c)) ** 2 + b * b)
    lmax = full["mid"] + half
    lmin = np.maximum(full["mid"] - half, 1e-300)
    pmag = np.linalg.norm(scene["pos"], axis=1) + np.linalg.norm(cam["cam"])
    tz = np.maximum(np.abs(full["depth"]), 1e-30)
    focal = W / (2 * cam["tan_fovx"]) + H / (2 * cam["tan_fovy"])
    cov_err = K_COV * EPS * np.maximum(full["cov_scale"], lmax)
    cmax = np.abs(full["conic"]).max(axis=1)
    err = dict(
        # per conic entry, absolute: the inverse amplifies the covariance's error by its condition number, counted against
        # the terms' magnitude -- cov_err / lambda_min of the 2D covariance (its determinant cancels)
        conic=SLACK * (cov_err / lmin) * cmax,
        # uv: the projection's own rounding (relative) and the view transform's absolute error seen through the focal length
        uv=SLACK * K_UV * EPS * (np.abs(full["uv"]).max(axis=1) + W + H + focal * pmag / tz),
        depth=SLACK * _depth_err(scene["pos"], cam["view"][2]),
        rgb=SLACK * K_RGB * EPS * (1.0 + 3.0 * np.abs(scene["sh"]).sum(axis=1).max(axis=1)),
        opacity=SLACK * K_OPACITY * EPS * scene["opacity"],
        # lambda = mid + sqrt(max(floor, mid^2 - det)): relative uncertainty (the cancelling mid^2 - det)
        lam=SLACK * (cov_err / np.maximum(full["lam"], 1e-300)) * (1.0 + full["mid"] / np.sqrt(np.maximum(max(R["floor"], 1e-300), full["mid"] ** 2 - full["det"]))),
    )
    return dict(R=R, pre=pre, full=full, err=err, W=W, H=H)


def _depth_err(pos, row):
    """p_view.z = v20 x + v21 y + v22 z + v23 in binary32.  A row that binary32 holds exactly (an axis-aligned camera at a
    representable position: its inverse is exact too) rounds only where a product by a non-power-of-two or a sum of two
    non-zero terms rounds -- with the identity camera at the origin, p_view.z = -z exactly, and the error is 0.  Any other
    row carries K_DEPTH ulp of the terms' magnitude."""
    terms = np.abs(np.concatenate([pos * row[:3], np.full((len(pos), 1), row[3])], axis=1))
    mag = terms.sum(axis=1)
    if not np.array_equal(row, row.astype(np.float32).astype(np.float64)):
        return K_DEPTH * EPS * mag
    m, _ = np.frexp(row)
    inexact = (m != 0) & (np.abs(m) != 0.5)                   # products that round
    nonzero = (terms > 0).sum(axis=1)
    return EPS * ((terms * inexact).sum(axis=1) + np.maximum(nonzero - 1, 0) * mag)


def _coord_range(args, tol, W, H, R):
    """The box coordinates the binary32 evaluation may produce: int() of any value within tol of the float64 argument."""
    lo, hi = npr.box_coords(args - tol, W, H, R), npr.box_coords(args + tol, W, H, R)
    return np.minimum(lo, hi), np.maximum(lo, hi)


def assert_matches_float64(out, frame, rules=None, image=True, label=None):
    """Raises Mismatch unless `out` (outputs_from_oracle / outputs_from_hip) is the float64 frame of `frame` under `rules`
    up to explained decisions and bounded rounding.  Returns a report: counts of explained mismatches per output, the
    largest continuous error relative to its bound, and the number of explained image pixels."""
    label = label or frame.label
    ref = reference(frame, rules)
    R, pre, full, err, W, H = ref["R"], ref["pre"], ref["full"], ref["err"], ref["W"], ref["H"]
    rep = {}
    tiles = np.asarray(out["tiles"]).astype(np.int64)
    ovis, fvis = tiles > 0, pre["tiles"] > 0
    obs_r = np.zeros(len(tiles))
    obs_r[ovis] = np.asarray(out["radius"])[ovis]           # (what a pipeline leaves in a culled Gaussian's slot is not read)
    obs_box = np.asarray(out["aabb"], np.int64)

    # ---- radius (where both keep the Gaussian): ceil(R sqrt(lambda)) within the uncertainty of an integer
    both = ovis & fvis
    v = R["radius"] * np.sqrt(np.maximum(full["lam"], 0))
    bad = both & (obs_r != full["radius"])
    dv = 0.5 * err["lam"] * v + 1e-12                       # what binary32 can move R sqrt(lambda) by
    ok = (obs_r >= np.ceil(v - dv)) & (obs_r <= np.ceil(v + dv))  # the outputs' radius is the ceiling of a value within it
    _check(not (bad & ~ok).any(), f"{label}: radius differs from float64 without a rounding explanation at Gaussians "
                                  f"{np.nonzero(bad & ~ok)[0][:8]} (binary32 {obs_r[bad & ~ok][:4]}, float64 {full['radius'][bad & ~ok][:4]}, "
                                  f"{R['radius']} sqrt(lambda) = {v[bad & ~ok][:4]})")
    rep["radius_explained"] = int(bad.sum())

    # ---- tile box, from the float64 uv and the outputs' own radius (a radius flip is explained above).  A mismatching
    # coordinate is explained only if int() of some value within the argument's uncertainty -- clamped to the grid, as
    # the shader clamps -- gives the outputs' coordinate: a coordinate that the clamp or a saturating conversion pins
    # is never explained, however large its argument's uncertainty.
    r_used = np.where(ovis, obs_r, full["radius"])
    args = npr.box_args(full["uv"], r_used, R)
    fbox = npr.box_coords(args, W, H, R)
    r_flip = np.ceil(v - dv) != np.ceil(v + dv)                # where binary32 may round the radius to the next integer
    arg_tol = (err["uv"] + r_flip)[:, None] / 16 + SLACK * 4 * EPS * np.abs(args)
    lo, hi = _coord_range(args, arg_tol, W, H, R)
    bad = both[:, None] & (obs_box != fbox)
    can = (lo != hi) & (obs_box >= lo) & (obs_box <= hi)
    _check(not (bad & ~can).any(), f"{label}: tile box differs from float64 where no rounding can move it, at Gaussians "
                                   f"{np.nonzero((bad & ~can).any(axis=1))[0][:8]}")
    rep["box_explained"] = int(bad.any(axis=1).sum())
    _check(np.array_equal(tiles[ovis], ((obs_box[:, 2] - obs_box[:, 0]) * (obs_box[:, 3] - obs_box[:, 1]))[ovis]),
           f"{label}: tiles != the box's area")

    # ---- visibility: the near cut within the depth's uncertainty, or a box that the coordinates' ranges can make both
    # empty and non-empty (its tile count in uint32 arithmetic, as preprocess.comp:169 forms it)
    flip = ovis != fvis
    near_ok = np.abs(full["depth"] - R["near"]) <= err["depth"]
    counts = [npr.box_tiles(np.stack([x0, y0, x1, y1], axis=1), R)
              for x0 in (lo[:, 0], hi[:, 0]) for y0 in (lo[:, 1], hi[:, 1])
              for x1 in (lo[:, 2], hi[:, 2]) for y1 in (lo[:, 3], hi[:, 3])]
    counts = np.stack(counts, axis=1)
    box_ok = (counts == 0).any(axis=1) & (counts != 0).any(axis=1)
    _check(not (flip & ~near_ok & ~box_ok).any(),
           f"{label}: visibility differs from float64 without a threshold explanation at Gaussians "
           f"{np.nonzero(flip & ~near_ok & ~box_ok)[0][:8]} (depth {full['depth'][flip & ~near_ok & ~box_ok][:4]}, kept by the "
           f"outputs: {ovis[flip & ~near_ok & ~box_ok][:4]})")
    rep["visibility_explained"] = int(flip.sum())

    # ---- continuous attributes of every Gaussian the outputs keep
    k = ovis
    worst = {}

    def bounded(name, got, want, tol):
        d = np.abs(np.asarray(got)[k].astype(np.float64) - want[k])
        t = np.asarray(tol, np.float64)[k]
        r = d / np.maximum(t[:, None] if d.ndim > 1 else t, 1e-300)
        worst[name] = float(r.max()) if r.size else 0.0
        badg = np.nonzero((r > 1.0).reshape(len(r), -1).any(axis=1))[0] if r.size else []
        _check(len(badg) == 0, f"{label}: {name} beyond its float64 bound at {len(badg)} Gaussian(s), e.g. id "
                               f"{np.nonzero(k)[0][badg[:4]]}: got {np.asarray(got)[k][badg[:2]]}, float64 {want[k][badg[:2]]}, "
                               f"bound {np.asarray(t)[badg[:2]]}")

    bounded("conic", out["conic"], full["conic"], err["conic"])
    bounded("opacity", out["opacity"], full["opacity"], err["opacity"])
    bounded("uv", out["uv"], full["uv"], err["uv"])
    bounded("depth", out["depth"], full["depth"], err["depth"])
    bounded("rgb", out["rgb"], full["rgb"], err["rgb"])
    rep["worst_bound_ratio"] = worst

    # ---- binning and depth order, restated from the outputs' own boxes and depths
    obs_depth = np.asarray(out["depth"], np.float32)
    tile, gid, ranges = npr.tile_lists(dict(tiles=tiles, box=obs_box, depth=obs_depth), W, H, R)
    _check(len(out["sorted_gid"]) == len(gid), f"{label}: {len(out['sorted_gid'])} list entries, float64 restatement {len(gid)}")
    _check(np.array_equal(np.asarray(out["sorted_tile"], np.int64), tile), f"{label}: tile of the list entries differs")
    badl = np.nonzero(np.asarray(out["sorted_gid"], np.int64) != gid)[0]
    _check(len(badl) == 0, f"{label}: list order differs at {len(badl)} entries, first {badl[:4]}: got "
                           f"{np.asarray(out['sorted_gid'])[badl[:4]]}, expected {gid[badl[:4]]}")
    _check(np.array_equal(np.asarray(out["ranges"], np.int64), ranges), f"{label}: ranges differ")

    if not image or out.get("image") is None:
        return rep
    img, dec = _image(ref, tiles, gid, ranges)
    rep.update(assert_image_matches(out["image"], img, dec, frame, label))
    if out.get("bgra") is not None:
        rep.update(assert_bgra_matches(out["bgra"], out["image"], img, label))
    return rep


def _image(ref, tiles, gid, ranges):
    full, err, R = ref["full"], ref["err"], ref["R"]
    att = dict(uv=full["uv"], conic=full["conic"], opacity=full["opacity"], rgb=full["rgb"])
    e = dict(conic=err["conic"], uv=err["uv"], rel=np.full(len(tiles), SLACK * K_POWER * EPS),
             alpha=SLACK * K_EXP * EPS + err["opacity"] / np.maximum(full["opacity"], 1e-30), rgb=err["rgb"])
    return npr.blend(att, gid, ranges, ref["W"], ref["H"], R, e)


def assert_image_matches(got, img, dec, frame, label):
    d = np.abs(np.asarray(got, np.float64)[..., :3] - img[..., :3]).max(axis=2)
    within = d <= ULP_NOISE + dec["cancel"]
    decided = (dec["alpha"] == 0) | (dec["T"] == 0) | (dec["power"] == 0)
    bad = ~within & ~decided
    if bad.any():
        ys, xs = np.nonzero(bad)
        i = int(np.argmax(d[ys, xs]))
        y, x = ys[i], xs[i]
        raise Mismatch(f"{label}: {len(ys)} pixel(s) differ from float64 beyond their bound with no decision within rounding; "
                       f"worst (x, y) = ({x}, {y}): |d| = {d[y, x]:.3g}, bound {ULP_NOISE + dec['cancel'][y, x]:.3g}, distances "
                       f"alpha {dec['alpha'][y, x]:.3g} T {dec['T'][y, x]:.3g} power {dec['power'][y, x]:.3g}")
    explained = int((~within & decided).sum())
    _check(explained <= frame.max_explained, f"{label}: {explained} pixels explained by a decision within rounding "
                                             f"(allowed {frame.max_explained})")
    _check(np.all(np.asarray(got)[..., 3] == 1), f"{label}: alpha channel != 1")
    rest = np.where(within, d, 0.0)
    return dict(explained_pixels=explained, image_max_abs=float(d.max()) if d.size else 0.0,
                image_max_over_bound=float((rest / (ULP_NOISE + dec["cancel"])).max()) if d.size else 0.0)


def assert_bgra_matches(bgra, got_img, img, label):
    """BGRA8 against the float64 image's quantisation: a byte may differ only where the rounding boundary lies between the
    float64 value and the outputs' own binary32 value (whose difference the image check has bounded) -- and the bytes must be
    the quantisation of the outputs' own image, but for binary32 ties of x * 255."""
    got_img = np.asarray(got_img, np.float64)
    own = npr.bgra8(got_img)
    tie = npr.bgra8_tie(got_img, 2.0 * EPS)
    badown = (own != bgra) & ~tie
    _check(not badown.any(), f"{label}: BGRA8 is not the quantisation of the frame's own image at "
                             f"{np.argwhere(badown.any(axis=-1))[:4].tolist()}")
    q64 = npr.bgra8(img)
    gap = np.abs(got_img - img)
    between = npr.bgra8_tie(img, gap + 2.0 * EPS)                 # a rounding boundary within |binary32 - float64|
    bad = (q64 != bgra) & ~between
    _check(not bad.any(), f"{label}: BGRA8 differs from the float64 image's quantisation at "
                          f"{np.argwhere(bad.any(axis=-1))[:4].tolist()}")
    _check(np.abs(q64.astype(int) - bgra.astype(int)).max(initial=0) <= 1, f"{label}: BGRA8 off by more than one step")
    return dict(bgra_explained=int((q64 != bgra).any(axis=-1).sum()))


def exercise(frame, mutation):
    """How many Gaussians, list entries and pixels the float64 reference decides differently under `mutation` than under
    the shaders' rules (on this frame)."""
    a, b = reference(frame), reference(frame, mutation)
    pa, pb = a["pre"], b["pre"]
    W, H = frame.width, frame.height
    g = (pa["tiles"] != pb["tiles"]) | (pa["radius"] != pb["radius"]) | (pa["box"] != pb["box"]).any(axis=1)
    for key in ("conic", "uv", "rgb"):
        tol = a["err"][key] if key != "rgb" else a["err"]["rgb"]
        d = np.abs(pa[key] - pb[key])
        g |= (pa["tiles"] > 0) & (d > (tol[:, None] if np.ndim(tol) else tol)).any(axis=1)
    if max(pa["tiles"].sum(), pb["tiles"].sum()) > 50_000_000:   # a wrapped tile count: the Gaussians tell it already
        return dict(gaussians=int(g.sum()), entries=0, pixels=0)
    ta, ga, ra = npr.tile_lists(pa, W, H, a["R"])
    tb, gb, rb = npr.tile_lists(pb, W, H, b["R"])
    entries = int((ga != gb).sum()) if len(ga) == len(gb) else abs(len(ga) - len(gb))
    ia, _ = _image(a, pa["tiles"], ga, ra)
    ib, _ = _image(b, pb["tiles"], gb, rb)
    pixels = int((np.abs(ia - ib)[..., :3].max(axis=2) > ULP_NOISE).sum())
    return dict(gaussians=int(g.sum()), entries=entries, pixels=pixels)
